"""CTC prefix beam search (csrc/hip/ctc_beam.hip) against a float64 restatement of its semantics, and against the CTC loss.

Reference: ``ref_row`` of ctc_reference.py -- dicts of label tuples, linear space, float64 (which holds these sizes without scaling),
the same candidate cells, merge order and canonical-index tie rule as INTEGRATION.md "CTC prefix beam search".

Premise of every parity case, asserted in float64 on the reference: at every frame the relative gap between the W-th and the (W+1)-th
candidate total, and after the last frame between adjacent hypotheses up to the one behind the last reported, is at least
16 * T * 2^-24.  A frame applies at most four roundings of 2^-24 to a sum of positive terms, so 4 * T * 2^-24 bounds the first-order
relative error of a float32 total: at four times that no rounding can flip a selection.  The seeds are fixed and meet the premise.

Score tolerance where the labels match: |score - ref| <= 8 * T * 2^-24 + 4 * ulp_f32(|ref|)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ctc_reference import (assert_scores as _assert_scores, ctc_loss64 as _ctc_loss64, decode as _run, ref_row as _ref_row, reference,
                           softmax as _softmax, tol as _tol)
from nntoolkitcore_amd import capi, layers as NL

pytestmark = pytest.mark.gpu


def _reference(p, lens, blank, W, cutoff, nbest):
    """the acoustic search: without the flag of the fused search's end-of-sentence step"""
    return reference(p, lens, blank, W, cutoff, nbest)[:4]


# name: (seed, B, T, C, W, cutoff, nbest, blank, lengths)
PARITY = {
    "small": (0, 2, 12, 5, 4, 0, 4, 4, None),
    "ragged": (0, 5, 40, 9, 8, 0, 3, 8, [40, 0, 1, 17, 39]),
    "blank7": (0, 3, 64, 33, 16, 0, 4, 7, None),
    "class_cut": (0, 2, 48, 300, 8, 6, 2, 299, None),
    "full_width": (1, 2, 24, 40, 128, 0, 8, 39, None),
    "cell_limit": (0, 1, 8, 128, 128, 0, 4, 127, None),
    # the kernel's other paths: the frame's probabilities (or cut pairs) do not fit in LDS beside the cells and are read from global
    # memory inside the frame, without and with a class cut; they fit but are more than a lane carries in registers (> 1024 words)
    "unstaged": (0, 1, 8, 12000, 1, 0, 1, 11999, None),
    "unstaged_cut": (0, 1, 8, 9000, 2, 8000, 2, 8999, None),
    "staged_wide": (0, 2, 8, 2000, 4, 0, 2, 1999, [8, 5]),
    "staged_wide_cut": (0, 1, 8, 3000, 4, 1500, 2, 2999, None),
}


@functools.lru_cache(maxsize=None)
def _parity_case(name):
    seed, B, T, Cc, W, cutoff, nbest, blank, lens = PARITY[name]
    p = _softmax(seed, B, T, Cc)
    lens = [T] * B if lens is None else lens
    return p, lens, _reference(p, lens, blank, W, cutoff, nbest)


@pytest.mark.parametrize("name", list(PARITY))
def test_parity_with_the_float64_reference(gpu, name):
    """case 1: labels, lengths and padding equal, scores within the tolerance"""
    seed, B, T, Cc, W, cutoff, nbest, blank, _ = PARITY[name]
    p, lens, (lab, n, sc, gap) = _parity_case(name)
    print("%s: smallest relative gap %.3g, premise %.3g" % (name, gap, 16 * T * 2.0 ** -24))
    assert gap >= 16 * T * 2.0 ** -24, "the premise does not hold for this seed"
    got_lab, got_n, got_sc = _run(gpu, p, lens, blank, W, cutoff, nbest)
    np.testing.assert_array_equal(got_n, n)
    np.testing.assert_array_equal(got_lab, lab)
    _assert_scores(name, T, got_sc, sc)


def test_exhaustive_beam_equals_the_ctc_loss(gpu):
    """case 2: nothing is ever pruned, so every score is minus the CTC loss of its labelling and the scores sum to one"""
    T, Cc, W, blank = 5, 3, 128, 2
    p = _softmax(3, 1, T, Cc)
    beam, _ = _ref_row(p[0].astype(np.float64), blank, W, 0)
    nbest = len(beam)
    assert 20 < nbest <= 63
    lab, n, sc = _run(gpu, p, [T], blank, W, 0, nbest)
    assert (n[0] >= 0).all() and len({tuple(lab[0, k, :n[0, k]]) for k in range(nbest)}) == nbest
    want = np.array([-_ctc_loss64(p[0], lab[0, k, :n[0, k]], blank) for k in range(nbest)])
    _assert_scores("exhaustive", T, sc[0], want)
    assert abs(np.exp(sc[0].astype(np.float64)).sum() - 1.0) <= 1e-5


def test_exact_ties_and_zeros(gpu):
    """case 3: uniform posteriors (exact arithmetic: the canonical-index tie rule alone decides), and one-hot posteriors"""
    T, Cc, W, blank = 6, 4, 4, 3
    p = np.full((1, T, Cc), 0.25, np.float32)
    lab, n, sc, _ = _reference(p, [T], blank, W, 0, 4)
    got_lab, got_n, got_sc = _run(gpu, p, [T], blank, W, 0, 4)
    np.testing.assert_array_equal(got_n, n)
    np.testing.assert_array_equal(got_lab, lab)
    _assert_scores("uniform", T, got_sc, sc)
    path = [3, 1, 1, 3, 1, 2, 2, 0, 3, 3]
    q = np.zeros((1, len(path), Cc), np.float32)
    q[0, np.arange(len(path)), path] = 1.0
    got_lab, got_n, got_sc = _run(gpu, q, None, blank, W, 0, 4)
    np.testing.assert_array_equal(got_n, [[4, -1, -1, -1]])
    np.testing.assert_array_equal(got_lab[0, 0], [1, 1, 2, 0] + [-1] * 6)
    assert (got_lab[0, 1:] == -1).all()
    assert got_sc[0, 0] == 0.0 and np.isneginf(got_sc[0, 1:]).all()


def test_exact_ties_beyond_the_survivor_list(gpu):
    """case 3 at W * C = 512: from frame 1 on about 500 cells tie exactly at the W-th total (powers of 1/64 times small integers, exact
    in float32), more than the 256 survivors the kernel ranks: the threshold search ends at a single key and the list is cut by index"""
    T, Cc, W, blank = 6, 64, 8, 63
    p = np.full((2, T, Cc), 1.0 / 64, np.float32)
    lens = [T, 2]
    lab, n, sc, _ = _reference(p, lens, blank, W, 0, W)
    got_lab, got_n, got_sc = _run(gpu, p, lens, blank, W, 0, W)
    np.testing.assert_array_equal(got_n, n)
    np.testing.assert_array_equal(got_lab, lab)
    _assert_scores("uniform 64", T, got_sc, sc)


def test_agrees_with_the_best_path_on_peaked_posteriors(gpu):
    """case 4: with the winning class at 0.9 or more per frame the best labelling is the best path's"""
    rng = np.random.default_rng(4)
    B, T, Cc, W, blank = 8, 100, 29, 8, 0
    paths = np.repeat(rng.integers(0, Cc, (B, T // 2)), 2, axis=1)
    p = rng.uniform(0.0, 0.1 / Cc, (B, T, Cc)).astype(np.float32)
    np.put_along_axis(p, paths[:, :, None], 0.9 + 0.01 * rng.integers(0, 9, (B, T, 1)).astype(np.float32), axis=2)
    lens = [100, 77, 0, 100, 1, 100, 53, 100]
    x = torch.from_numpy(p).to(gpu)
    want, wn = NL.ctc_greedy_decode_device(x, lens, blank)
    lab, n, sc = NL.ctc_beam_decode_device(x, lens, blank, W, 0, 1)
    torch.cuda.synchronize()
    assert int(wn.max()) > 20
    np.testing.assert_array_equal(n.cpu().numpy()[:, 0], wn.cpu().numpy())
    np.testing.assert_array_equal(lab.cpu().numpy()[:, 0], want.cpu().numpy())


def test_pruned_scores_are_lower_bounds(gpu):
    """case 5: no premise here; pruning can only lose mass"""
    B, T, Cc, W, nbest, blank = 4, 200, 33, 32, 4, 32
    p = _softmax(5, B, T, Cc)
    lens = [200, 163, 200, 90]
    lab, n, sc = _run(gpu, p, lens, blank, W, 0, nbest)
    for b in range(B):
        assert (np.diff(sc[b]) <= 0).all(), b
        assert (n[b] >= 0).all() and (n[b] <= lens[b]).all(), b
        hyps = [tuple(lab[b, k, :n[b, k]]) for k in range(nbest)]
        assert len(set(hyps)) == nbest, b
        for k, h in enumerate(hyps):
            assert (lab[b, k, n[b, k]:] == -1).all()
            full = -_ctc_loss64(p[b, :lens[b]], h, blank)
            print("row %d hypothesis %d: score %.6f, full labelling %.6f" % (b, k, sc[b, k], full))
            assert sc[b, k] <= full + _tol(T, np.array([full]))[0], (b, k)


def test_determinism_and_row_independence(gpu):
    """case 6"""
    B, T, Cc, W, nbest, blank = 4, 40, 9, 8, 3, 8
    p = _softmax(6, B, T, Cc)
    lens = [40, 23, 31, 0]
    one = _run(gpu, p, lens, blank, W, 0, nbest)
    two = _run(gpu, p, lens, blank, W, 0, nbest)
    for a, c in zip(one, two):
        assert a.tobytes() == c.tobytes()
    alone = _run(gpu, p[2:3].copy(), lens[2:3], blank, W, 0, nbest)
    for a, c in zip(one, alone):
        assert a[2].tobytes() == c[0].tobytes()
    q = p.copy()
    for b in range(B):
        q[b, lens[b]:] = np.nan
    for a, c in zip(one, _run(gpu, q, lens, blank, W, 0, nbest)):
        assert a.tobytes() == c.tobytes()
    for cutoff in (Cc - 1, Cc + 5):
        for a, c in zip(one, _run(gpu, p, lens, blank, W, cutoff, nbest)):
            assert a.tobytes() == c.tobytes(), cutoff


def test_argument_errors_write_nothing(gpu):
    """case 7: -1, a message, the outputs and the head of the workspace as they were"""
    L = capi.load()
    B, T, Cc = 2, 6, 5
    x = torch.full((B, T, Cc), 0.2, device=gpu)
    dp = lambda t: C.c_void_p(t.data_ptr())
    good = dict(il=[6, 4], blank=4, W=4, nbest=2, cut=0, C=Cc)
    bad = [dict(il=[7, 4]), dict(il=[6, -1]), dict(blank=5), dict(blank=-1), dict(W=0), dict(W=129, nbest=1), dict(nbest=0), dict(nbest=5),
           dict(cut=-1), dict(W=128, C=130, nbest=1), dict(misalign=1)]
    xl = torch.full((B, T, 130), 1.0 / 130, device=gpu)
    for change in bad:
        a = dict(good, **change)
        nb = max(a["nbest"], 1)
        lab = torch.full((B, nb, T), 7, dtype=torch.int32, device=gpu)
        n = torch.full((B, nb), 7, dtype=torch.int32, device=gpu)
        sc = torch.full((B, nb), 7.0, device=gpu)
        ws = torch.full((4096 + L.nntk_ctc_beam_workspace_floats(B, T, a["C"], 128, 0),), 7.0, device=gpu)
        il = np.asarray(a["il"], np.int32)
        wsp = C.c_void_p(ws.data_ptr() + 4 * a.get("misalign", 0))
        rc = L.nntk_ctc_beam_decode_device(dp(xl if a["C"] == 130 else x), B, T, a["C"], il.ctypes.data_as(capi.ip), a["blank"], a["W"],
                                           a["cut"], a["nbest"], dp(lab), dp(n), dp(sc), wsp)
        assert rc == -1 and capi.last_error() != "", change
        torch.cuda.synchronize()
        assert (lab == 7).all() and (n == 7).all() and (sc == 7.0).all() and (ws[:4096] == 7.0).all(), change


def test_host_form_equals_the_device_form(gpu):
    """case 8, on the ragged parity case"""
    seed, B, T, Cc, W, cutoff, nbest, blank, _ = PARITY["ragged"]
    p, lens, _ = _parity_case("ragged")
    dev = _run(gpu, p, lens, blank, W, cutoff, nbest)
    host = NL.ctc_beam_decode(p, lens, blank, W, cutoff, nbest)
    for a, c in zip(dev, host):
        assert a.tobytes() == c.tobytes()
