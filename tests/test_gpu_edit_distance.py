"""GPU: nntk_edit_distance_device against the table-and-backtrace reference (tests/edit_distance_reference.py).  Every count is compared
as an exact integer.  The alphabet has 3 symbols, so equal distances are everywhere and the preference order decides the counts."""
import numpy as np
import pytest
import torch

import edit_distance_reference as R
from nntoolkitcore_amd import layers as NL

pytestmark = pytest.mark.gpu

INT_MIN = -2 ** 31
SEP = 0


def _pack(rows, L=None, pad=-1, garbage=None):
    """rows: per batch row a list of hypotheses (a list of tokens, or None = no hypothesis) -> (hyp [B,n,L] int32, lengths [B,n]);
    behind every hypothesis pad, or values drawn from `garbage` by a fixed generator"""
    B, n = len(rows), len(rows[0])
    L = max([1] + [len(h) for r in rows for h in r if h is not None]) if L is None else L
    hyp = np.full((B, n, L), pad, np.int32)
    if garbage is not None:
        hyp[:] = np.random.default_rng(99).choice(np.array(garbage, np.int64), size=hyp.shape).astype(np.int32)
    lens = np.zeros((B, n), np.int32)
    for b, r in enumerate(rows):
        assert len(r) == n
        for k, h in enumerate(r):
            if h is None:
                lens[b, k] = -1
            else:
                lens[b, k] = len(h)
                hyp[b, k, :len(h)] = h
    return hyp, lens


def _run(gpu, hyp, lens, refs, sep=-1, max_ref_len=None):
    if max_ref_len is not None:
        lab = np.zeros((len(refs), max_ref_len), np.int32)
        for b, r in enumerate(refs):
            lab[b, :len(r)] = r
        refs_arg, rl = lab, np.array([len(r) for r in refs], np.int32)
    else:
        refs_arg, rl = refs, None
    counts, units = NL.edit_distance_device(torch.from_numpy(hyp).to(gpu), torch.from_numpy(lens).to(gpu), refs_arg, rl, sep=sep)
    torch.cuda.synchronize()
    return counts.cpu().numpy(), units.cpu().numpy()


def _check(gpu, rows, refs, sep=-1, **kw):
    hyp, lens = _pack(rows, **kw)
    got, units = _run(gpu, hyp, lens, refs, sep)
    want, want_units = R.batch_counts(hyp, lens, refs, sep, fast=True)
    bad = np.argwhere((got != want).any(axis=2))
    assert bad.size == 0, (bad[:5].tolist(), got[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
    assert np.array_equal(units, want_units)
    return got


def _seq(rng, n, lo=1, hi=4):
    return rng.integers(lo, hi, n).tolist()


# (hypothesis length, reference length): the trivial ones, then the lengths around a wavefront (64 lanes), around the workgroup
# (256 lanes, and the most units one wavefront takes) against an equal length, a much shorter one and 300
EDGES = [63, 64, 65, 255, 256, 257]
PAIR_LENGTHS = [(0, 0), (0, 5), (5, 0), (1, 1)] + [p for L in EDGES for p in ((L, L), (L, 3), (3, L), (L, 300), (300, L))]


def _edge_pairs():
    rng = np.random.default_rng(11)
    rows, refs = [], []
    for m, n in PAIR_LENGTHS:
        r = _seq(rng, n)
        h = _seq(rng, m)
        k = min(m, n) // 2                       # half of the shorter side copied: hits, runs of ties and all three operations
        h[:k] = r[:k]
        rows.append([h])
        refs.append(r)
    return rows, refs


def test_lengths_around_the_wavefront_and_the_workgroup_short_and_long_pairs_in_one_launch(gpu):
    rows, refs = _edge_pairs()
    got = _check(gpu, rows, refs)
    assert got[0, 0].tolist() == [0, 0, 0, 0] and got[1, 0].tolist() == [5, 0, 5, 0] and got[2, 0].tolist() == [5, 0, 0, 5]


def test_a_pairs_counts_depend_on_nothing_but_the_pair(gpu):
    rows, refs = _edge_pairs()
    hyp, lens = _pack(rows)
    base, base_units = _run(gpu, hyp, lens, refs)
    # every odd row replaced by something else, the tensors padded further out
    rng = np.random.default_rng(12)
    rows2 = [r if b % 2 == 0 else [_seq(rng, 40 + b)] for b, r in enumerate(rows)]
    refs2 = [r if b % 2 == 0 else _seq(rng, 17 + b) for b, r in enumerate(refs)]
    hyp2, lens2 = _pack(rows2, L=hyp.shape[2] + 139)
    got, units = _run(gpu, hyp2, lens2, refs2, max_ref_len=1000)
    assert np.array_equal(got[0::2], base[0::2]) and np.array_equal(units[0::2], base_units[0::2])
    want, _ = R.batch_counts(hyp2, lens2, refs2, fast=True)
    assert np.array_equal(got, want)
    # a pair alone in its launch: batch x n_hyp = 1
    for b in (7, len(rows) - 1):
        alone, _ = _run(gpu, *_pack([rows[b]]), [refs[b]])
        assert np.array_equal(alone[0], base[b])


def test_the_longest_reference_against_3_and_against_1100(gpu):
    rng = np.random.default_rng(13)
    r0, r1 = _seq(rng, 4000), _seq(rng, 4000)
    h1 = list(r1[:1100])
    for i in rng.integers(0, 1100, 300):
        h1[i] = int(rng.integers(1, 4))
    got = _check(gpu, [[_seq(rng, 3)], [h1]], [r0, r1])
    assert got[0, 0, 0] >= 3997 and got[1, 0, 2] >= 2900


def test_seven_rows_of_three_with_empty_slots(gpu):
    rng = np.random.default_rng(14)
    refs = [_seq(rng, n) for n in (5, 0, 70, 12, 300, 1, 64)]
    rows = [[_seq(rng, int(rng.integers(0, 2 * len(r) + 3))) for _ in range(3)] for r in refs]
    rows[0][2] = None
    rows[3] = [None, None, None]
    rows[4][1] = None
    rows[6][0] = None
    got = _check(gpu, rows, refs)
    assert (got[0, 2] == -1).all() and (got[3] == -1).all() and (got[4, 1] == -1).all() and (got[6, 0] == -1).all()
    assert (got[0, :2] >= 0).all()


@pytest.mark.parametrize("sep", [-1, SEP])
def test_what_stands_behind_a_hypothesis_is_not_read(gpu, sep):
    rng = np.random.default_rng(15)
    refs = [_seq(rng, n, 0) for n in (9, 70, 280, 0)]
    rows = [[_seq(rng, int(rng.integers(0, len(r) + 9)), 0) for _ in range(2)] for r in refs]
    rows[1][1] = None
    L = 330
    clean = _run(gpu, *_pack(rows, L=L), refs, sep)
    dirty_hyp, lens = _pack(rows, L=L, garbage=[SEP, INT_MIN, 1, 2, 3, -1])
    assert (dirty_hyp[1, 1] != -1).any()
    dirty = _run(gpu, dirty_hyp, lens, refs, sep)
    assert np.array_equal(clean[0], dirty[0]) and np.array_equal(clean[1], dirty[1])
    want, units = R.batch_counts(dirty_hyp, lens, refs, sep, fast=True)
    assert np.array_equal(dirty[0], want) and np.array_equal(dirty[1], units)


def test_a_length_above_max_hyp_len_is_read_as_max_hyp_len(gpu):
    rng = np.random.default_rng(16)
    refs = [_seq(rng, 20), _seq(rng, 290)]
    hyp, lens = _pack([[_seq(rng, 24)], [_seq(rng, 24)]])
    lens[:, 0] = [25, 32767]
    got, _ = _run(gpu, hyp, lens, refs)
    lens[:, 0] = 24
    want, _ = R.batch_counts(hyp, lens, refs)
    assert np.array_equal(got, want)


def test_two_calls_give_the_same_bits(gpu):
    rows, refs = _edge_pairs()
    hyp, lens = _pack(rows)
    a, b = _run(gpu, hyp, lens, refs), _run(gpu, hyp, lens, refs)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    a, b = _run(gpu, hyp, lens, refs, SEP + 1), _run(gpu, hyp, lens, refs, SEP + 1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_word_mode_separators_and_exact_word_equality(gpu):
    s = SEP
    refs = [
        [5, 6, s, 7, s, 8, 9],                  # three words
        [5, 6, s, 7, s, 8, 9],
        [s, s, s],                              # no words
        [1, 2, 3, s, 4, 4],
        [5, 5, s, 6],
        [],
        [3, 1, 2],
    ]
    rows = [
        [[s, 5, 6, s, s, 7, s, 8, 9, s, s], [5, 6, 7, 8, 9]],           # separators leading, repeated, trailing: the same words | one word
        [[s, s], [7]],                                                   # separators only: 0 words | one word of the three
        [[s], [4, s, 4]],                                                # both sides empty | two insertions
        [[1, 2, 4, s, 4, 4], [1, 2, 3, s, 4]],                           # words that differ only in their last token | in their length
        [[5, 5, 5, s, 6], [5, s, 6]],                                    # the same repeated content at another length
        [[], [s, 2, s]],
        [[3, 1, 2, s], [2, 1, 3]],
    ]
    got = _check(gpu, rows, refs, sep=s)
    assert got[0, 0].tolist() == [0, 0, 0, 0] and got[0, 1].tolist() == [3, 1, 2, 0]
    assert got[1, 0].tolist() == [3, 0, 3, 0] and got[1, 1].tolist() == [2, 0, 2, 0]
    assert got[2, 0].tolist() == [0, 0, 0, 0] and got[2, 1].tolist() == [2, 0, 0, 2]
    assert got[3, 0].tolist() == [1, 1, 0, 0] and got[3, 1].tolist() == [1, 1, 0, 0]
    assert got[4, 0].tolist() == [1, 1, 0, 0] and got[4, 1].tolist() == [1, 1, 0, 0]
    # the same tensors in unit mode: the separator is a token like any other, and the units are the tokens
    hyp, lens = _pack(rows)
    unit, units = _run(gpu, hyp, lens, refs)
    assert units.tolist() == [len(r) for r in refs]
    assert np.array_equal(unit, R.batch_counts(hyp, lens, refs)[0])


def test_word_mode_beyond_one_wavefronts_units(gpu):
    """more than 256 words on a side: the workgroup form of the sweep over word records, mixed with short pairs"""
    rng = np.random.default_rng(17)

    def sentence(words):
        out = []
        for _ in range(words):
            out += _seq(rng, int(rng.integers(1, 4))) + [SEP] * int(rng.integers(1, 3))
        return out

    refs = [sentence(300), sentence(40), sentence(257), sentence(256)]
    rows = [[list(refs[0]), sentence(290)], [sentence(300), sentence(3)], [sentence(256), list(refs[2][:-1])], [sentence(256), []]]
    for i in rng.integers(0, len(rows[0][0]), 60):
        if rows[0][0][i] != SEP:
            rows[0][0][i] = int(rng.integers(1, 4))
    got = _check(gpu, rows, refs, sep=SEP)
    assert got[2, 1].tolist() == [0, 0, 0, 0]


def test_ctc_beam_search_outputs_go_straight_in(gpu):
    rng = np.random.default_rng(18)
    B, T, Cc = 5, 12, 6
    x = rng.standard_normal((B, T, Cc)) * 2.0
    p = np.exp(x - x.max(-1, keepdims=True))
    probs = torch.from_numpy((p / p.sum(-1, keepdims=True)).astype(np.float32)).to(gpu)
    labels, lengths, _ = NL.ctc_beam_decode_device(probs, input_lengths=[12, 12, 7, 1, 0], blank=0, beam_width=8, nbest=4)
    refs = [rng.integers(1, Cc, n).tolist() for n in (6, 3, 5, 0, 2)]
    for sep in (-1, 3):
        counts, units = NL.edit_distance_device(labels, lengths, refs, sep=sep)
        torch.cuda.synchronize()
        want, want_units = R.batch_counts(labels.cpu().numpy(), lengths.cpu().numpy(), refs, sep)
        assert np.array_equal(counts.cpu().numpy(), want) and np.array_equal(units.cpu().numpy(), want_units)
    assert (lengths.cpu().numpy() < 0).any() and (lengths.cpu().numpy() > 0).any()
    # the greedy decoder's [B, T] / [B] outputs: n_hyp = 1
    gl, gn = NL.ctc_greedy_decode_device(probs, blank=0)
    counts, units = NL.edit_distance_device(gl, gn, refs)
    torch.cuda.synchronize()
    want, _ = R.batch_counts(gl.cpu().numpy(), gn.cpu().numpy(), refs)
    assert np.array_equal(counts.cpu().numpy(), want)
    rate = NL.error_rate(counts, units)
    assert rate == want[:, 0, 0].sum() / sum(len(r) for r in refs)


def test_transducer_beam_search_outputs_go_straight_in(gpu):
    import rnnt_beam_cases as K
    from rnnt_beam_device import decoder, to_device
    c = K.case("awkward")
    dec = decoder(gpu, c)
    labels, lengths = dec.beam_decode(to_device(gpu, c["enc"]), c["n"], c["W"], c["nbest"], K.ml(c))[:2]
    rng = np.random.default_rng(19)
    refs = [rng.integers(1, c["m"]["V"], n).tolist() for n in (7, 2, 0)]
    counts, units = NL.edit_distance_device(labels, lengths, refs)
    torch.cuda.synchronize()
    dec.destroy()
    want, want_units = R.batch_counts(labels.cpu().numpy(), lengths.cpu().numpy(), refs)
    assert labels.shape[1] == c["nbest"] and (lengths.cpu().numpy() > 0).any()
    assert np.array_equal(counts.cpu().numpy(), want) and np.array_equal(units.cpu().numpy(), want_units)


@pytest.mark.parametrize("sep", [-1, SEP])
def test_host_form_equals_device_form(gpu, sep):
    rng = np.random.default_rng(20)
    refs = [_seq(rng, n, 0) for n in (30, 270, 0)]
    rows = [[_seq(rng, int(rng.integers(0, len(r) + 20)), 0) for _ in range(2)] for r in refs]
    rows[2][1] = None
    hyp, lens = _pack(rows, garbage=[SEP, INT_MIN, 7])
    dev = _run(gpu, hyp, lens, refs, sep)
    host = NL.edit_distance(hyp, lens, refs, sep=sep)
    assert np.array_equal(host[0], dev[0]) and np.array_equal(host[1], dev[1])
    assert np.array_equal(host[0], R.batch_counts(hyp, lens, refs, sep, fast=True)[0])
