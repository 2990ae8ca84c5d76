"""CPU-only: the reference of the error counts (tests/edit_distance_reference.py) against a memoised brute force and hand cases,
and the argument refusals of the C entries, which need no device."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import edit_distance_reference as R
from nntoolkitcore_amd import capi


def brute(h, r):
    """the best (distance, S, D, I) of the stated recursion, by memoised recursion from (m, n): the candidates in the stated order, a
    later one only on a strictly smaller distance"""
    @functools.lru_cache(maxsize=None)
    def go(i, j):
        if i == 0:
            return (j, 0, j, 0)
        if j == 0:
            return (i, 0, 0, i)
        s = int(h[i - 1] != r[j - 1])
        a, b, c = go(i - 1, j - 1), go(i, j - 1), go(i - 1, j)
        best = (a[0] + s, a[1] + s, a[2], a[3])
        if b[0] + 1 < best[0]:
            best = (b[0] + 1, b[1], b[2] + 1, b[3])
        if c[0] + 1 < best[0]:
            best = (c[0] + 1, c[1], c[2], c[3] + 1)
        return best
    return go(len(h), len(r))


def all_sequences(max_len):
    for n in range(max_len + 1):
        yield from itertools.product((0, 1), repeat=n)


def test_reference_equals_brute_force_on_every_binary_pair_up_to_length_5():
    seqs = list(all_sequences(5))
    assert len(seqs) == 63
    for h in seqs:
        for r in seqs:
            want = brute(h, r)
            assert R.counts(h, r) == want, (h, r)
            assert R.counts_fast(h, r) == want, (h, r)


def test_fast_reference_equals_the_plain_one_on_random_pairs():
    rng = np.random.default_rng(3)
    for _ in range(40):
        m, n = rng.integers(0, 40, 2)
        h, r = rng.integers(0, 3, m).tolist(), rng.integers(0, 3, n).tolist()
        assert R.counts_fast(h, r) == R.counts(h, r)


A, B_, C_ = 1, 2, 3


@pytest.mark.parametrize("h,r,want", [
    ([A, B_], [B_, A], (2, 2, 0, 0)),
    ([], [A, B_, C_], (3, 0, 3, 0)),
    ([A, B_, C_], [], (3, 0, 0, 3)),
    ([A, B_, C_], [A, B_, C_], (0, 0, 0, 0)),
    ([], [], (0, 0, 0, 0)),
    ([A, C_], [A, B_, C_], (1, 0, 1, 0)),
    ([A, B_, C_], [A, C_], (1, 0, 0, 1)),
])
def test_hand_cases(h, r, want):
    assert R.counts(h, r) == want
    assert R.counts_fast(h, r) == want


def test_word_splitting_drops_empty_words():
    sep = 0
    assert R.split_words([0, 0, 5, 6, 0, 0, 7, 0], sep) == [(5, 6), (7,)]
    assert R.split_words([0, 0, 0], sep) == []
    assert R.split_words([], sep) == []
    assert R.split_words([5], sep) == [(5,)]
    # leading, double and trailing separators change nothing
    hyp = np.array([[[0, 5, 6, 0, 0, 7, 0, 0]]], np.int32)
    got, units = R.batch_counts(hyp, [[7]], [[5, 6, 0, 8, 0, 9]], sep=sep)
    assert units.tolist() == [3]
    assert got[0, 0].tolist() == [2, 1, 1, 0]          # "56 7" against "56 8 9": 8 deleted, 7 -> 9 substituted


def test_batch_rules_no_hypothesis_and_clamped_length():
    hyp = np.array([[[1, 2, 3], [1, 2, 3]]], np.int32)
    got, units = R.batch_counts(hyp, [[-1, 9]], [[1, 2, 3]])
    assert got[0, 0].tolist() == [-1] * 4 and got[0, 1].tolist() == [0] * 4 and units.tolist() == [3]


def test_mwer_reference_matches_the_definition_by_hand():
    risk, grad = R.mwer([[0.0, 0.0]], [[0, 2]])
    assert risk[0] == 0.0 and np.allclose(grad[0], [-0.5, 0.5])
    risk, grad = R.mwer([[np.log(0.75), np.log(0.25), 0.0]], [[0, 4, -1]])
    assert np.isclose(risk[0], 0.75 * -2 + 0.25 * 2) and grad[0, 2] == 0.0 and abs(grad[0].sum()) < 1e-15
    risk, grad = R.mwer([[-np.inf, -np.inf], [0.0, 0.0]], [[1, 2], [-1, -1]])
    assert not risk.any() and not grad.any()


# ---- the C entries' refusals: made on the host before anything is enqueued, so they need no device ----
def _ints(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(capi.ip)


def _device_call(L, **kw):
    """nntk_edit_distance_device on made-up (never dereferenced) device addresses; kw overrides an argument"""
    refs, refs_p = _ints([[1, 2, 3], [4, 5, 6]])
    rl, rl_p = _ints([3, 2])
    a = dict(d_hyp=C.c_void_p(0x10000), d_hyp_lengths=C.c_void_p(0x20000), batch=2, n_hyp=3, max_hyp_len=8, refs=refs_p, ref_lengths=rl_p,
             max_ref_len=3, sep=-1, d_counts=C.c_void_p(0x30000), d_ref_units=C.c_void_p(0x40000), d_workspace=C.c_void_p(0x50000))
    a.update(kw)
    return L.nntk_edit_distance_device(a["d_hyp"], a["d_hyp_lengths"], a["batch"], a["n_hyp"], a["max_hyp_len"], a["refs"],
                                       a["ref_lengths"], a["max_ref_len"], a["sep"], a["d_counts"], a["d_ref_units"], a["d_workspace"])


@pytest.mark.parametrize("kw,word", [
    (dict(d_hyp=None), "NULL"), (dict(d_hyp_lengths=None), "NULL"), (dict(d_counts=None), "NULL"), (dict(d_workspace=None), "NULL"),
    (dict(refs=None), "NULL"), (dict(ref_lengths=None), "NULL"),
    (dict(max_ref_len=4001), "4000"), (dict(max_hyp_len=32768), "32767"), (dict(max_hyp_len=-1), "32767"),
    (dict(n_hyp=0), "n_hyp"), (dict(batch=-1), "batch"),
    (dict(d_workspace=C.c_void_p(0x50004)), "16-byte"),
])
def test_device_entry_refusals_need_no_device(built_lib, kw, word):
    assert _device_call(built_lib, **kw) == -1
    err = capi.last_error()
    assert err.startswith("nntk_edit_distance_device") and word in err, err


@pytest.mark.parametrize("lengths", [[3, 4], [-1, 2]])
def test_reference_length_outside_its_range_is_refused(built_lib, lengths):
    rl, rl_p = _ints(lengths)
    assert _device_call(built_lib, ref_lengths=rl_p) == -1
    assert "ref_lengths" in capi.last_error() and "[0, 3]" in capi.last_error()


def test_host_entry_refuses_the_same_and_writes_nothing(built_lib):
    hyp, hyp_p = _ints(np.zeros((2, 3, 8)))
    hl, hl_p = _ints(np.zeros((2, 3)))
    refs, refs_p = _ints([[1, 2, 3], [4, 5, 6]])
    rl, rl_p = _ints([3, 9])
    counts, counts_p = _ints(np.full((2, 3, 4), 77))
    L = built_lib
    assert L.nntk_edit_distance(hyp_p, hl_p, 2, 3, 8, refs_p, rl_p, 3, -1, counts_p, None) == -1
    assert capi.last_error().startswith("nntk_edit_distance:") and (counts == 77).all()
    rl[1] = 1
    assert L.nntk_edit_distance(hyp_p, hl_p, 2, 3, 8, refs_p, rl_p, 4001, -1, counts_p, None) == -1 and "4000" in capi.last_error()
    assert L.nntk_edit_distance(None, hl_p, 2, 3, 8, refs_p, rl_p, 3, -1, counts_p, None) == -1 and "NULL" in capi.last_error()
    assert (counts == 77).all()


def test_empty_batch_needs_no_device(built_lib):
    L = built_lib
    assert L.nntk_edit_distance_device(None, None, 0, 1, 8, None, None, 3, -1, None, None, None) == 0 and capi.last_error() == ""
    assert L.nntk_edit_distance(None, None, 0, 1, 8, None, None, 3, -1, None, None) == 0 and capi.last_error() == ""
    assert L.nntk_mwer_device(None, None, 4, 0, 8, None, None) == 0 and capi.last_error() == ""
    assert L.nntk_row_scale_device(None, None, 0, 5, None) == 0 and capi.last_error() == ""


def test_mwer_and_row_scale_refusals_need_no_device(built_lib):
    L, p = built_lib, C.c_void_p(0x10000)
    assert L.nntk_mwer_device(None, p, 4, 2, 3, p, p) == -1 and "NULL" in capi.last_error()
    assert L.nntk_mwer_device(p, p, 0, 2, 3, p, p) == -1 and "err_stride" in capi.last_error()
    assert L.nntk_mwer_device(p, p, 4, 2, 0, p, p) == -1 and "n_hyp" in capi.last_error()
    assert L.nntk_mwer_device(p, p, 4, 2, 3, None, None) == -1 and "NULL" in capi.last_error()
    assert L.nntk_row_scale_device(p, None, 2, 3, p) == -1 and "NULL" in capi.last_error()
    assert L.nntk_row_scale_device(p, p, -1, 3, p) == -1 and "rows" in capi.last_error()


def test_workspace_size_grows_with_every_argument(built_lib):
    f = built_lib.nntk_edit_distance_workspace_floats
    base = f(4, 2, 100, 50)
    assert base >= 4 + 4 * 50 and base % 4 == 0
    assert f(8, 2, 100, 50) > base and f(4, 4, 100, 50) > base and f(4, 2, 200, 50) > base and f(4, 2, 100, 100) > base
    assert f(100000, 8, 32767, 4000) > 2 ** 32        # 64-bit arithmetic
