"""CTC prefix beam search (csrc/hip/ctc_beam.hip) beyond one staged block of frames: one-shot, with an n-gram model, and streamed, at the
lengths the stack emits (1000 frames an utterance), where the earlier files (test_gpu_ctc_beam.py, test_gpu_ctc_beam_lm.py,
test_gpu_ctc_stream.py: T * W <= 8192 everywhere) run the block loops of ctc_beam_backtrack_kernel<FIN> and ctc_beam_commit_kernel<FIN>
exactly once, never see a prefix longer than 255 labels (a record packs length << 8 | parent rank) and never reach the stride loop of
ctc_beam_cut_kernel (more than 16384 workgroups x 4 frames).

The cases, their seeds (found on the CPU; nothing about them comes from a device) and the block arithmetic live in
tests/ctc_long_cases.py; tests/test_ctc_long_premises.py checks them without a device.  No tolerance is new: ``tol`` and the gap
premise are test_gpu_ctc_beam.py's, ``tol_lm`` and its count of roundings test_gpu_ctc_beam_lm.py's; everything else is equality of
labels, lengths and score bits (``eq``), or a one-sided bound.

  case                                        what only it reaches                                       tied to the reference by
  1 parity[w128_T96, w100_T90 (W no power of  backtrack<false>: two blocks, rank and pos carried over    the float64 search itself
    two), w16_T560, w8_T1100 (880 labels)]    the seam; len and pos above 255                            (gap premise asserted)
  2 utterance, B 3, T 1000, rows of 2 / 2 /   backtrack<FIN> over forder across the seam; streams of     one-shot = streamed (different code,
    1 blocks (488+512, 1+512, 512), acoustic  16 pushes whose strings pass 255 labels; commit<FIN>        same beam); score <= ln likelihood
    and with the trigram model                                                                           of the reported string (float64)
  3 one push of 96 frames at W = 128,         commit<false> and commit<FIN>: two blocks, `gained`        = the one-shot call = case 1
    acoustic and with the trigram model       carried over the seam                                      (acoustic); = one-shot (model)
  4 class cut, 1200 x 56 = 67200 frames       ctc_beam_cut_kernel's second stride round                  = 12 calls of 100 rows (no stride)

Why (b) of case 2 notices a string damaged at the seam: on these peaked posteriors (scale 8) pruning loses little -- in the float64
search the likelihood of a reported string exceeds its score by 0.6 to 1.3 nats (acoustic; 0.3 to 2.1 with the model) -- while
replacing ONE label of a row's best string by its neighbour class costs 10 to 16 nats of acoustic likelihood, and a rank lost at the
seam replaces a whole block of them.

Measured on the MI355X (wall time of the test with its share of the CPU reference; no defect was found in the kernels):

  test                                 largest score error / smallest allowance                          time
  parity[w128_T96]                     9.45e-07 / 5.34e-05                                               0.71 s
  parity[w100_T90]                     9.38e-07 / 5.05e-05                                               0.36 s
  parity[w16_T560]                     3.19e-06 / 2.98e-04                                               0.13 s
  parity[w8_T1100]                     8.65e-06 / 5.86e-04                                               0.19 s
  utterance[acoustic]                  every score >= 0.64 below its bound (allowed: 5.38e-04 above)     0.31 s
  utterance[trigram]                   every score >= 0.333 below its bound (allowed: 1.68e-03 above)    0.21 s
  one_push[acoustic], [trigram]        bit equality                                                      0.02 s, 0.03 s
  class_cut_beyond_its_grid            bit equality                                                      0.02 s
  the whole file                                                                                         4.5 s
"""
import numpy as np
import pytest

import ctc_long_cases as K
from ctc_reference import assert_scores as _assert_scores, ctc_loss64 as _ctc_loss64, decode, drive, eq, rounds as _rounds, tol, tol_lm
from nntoolkitcore_amd import layers as NL

pytestmark = pytest.mark.gpu


def _lm(Cc, blank):
    return NL.NgramLm.from_arrays(alpha=K.LM["alpha"], beta=K.LM["beta"], **K.lm_table(Cc, blank))


@pytest.mark.parametrize("name", list(K.PARITY))
def test_parity_across_a_block_seam(gpu, name):
    """case 1: labels, lengths and padding equal the float64 reference's, scores within tol(T, ref)"""
    seed, scale, T, Cc, W, nbest, want_blocks = K.PARITY[name]
    assert K.blocks(T, W) == want_blocks and len(want_blocks) == 2
    lab, n, sc, gap = K.parity_premise(name)
    got_lab, got_n, got_sc = decode(gpu, K.parity_probs(name), [T], Cc - 1, W, 0, nbest)
    np.testing.assert_array_equal(got_n, n)
    np.testing.assert_array_equal(got_lab, lab)
    _assert_scores(name, T, got_sc, sc)
    if name == "w8_T1100":
        assert got_n[0, 0] > 255


def _assert_nbest_is_sound(tag, got, lens, nbest, T, bound, allow):
    """(c) distinct strings, non-increasing scores, -1 padding; (b) every score is at most the float64 bound of its string + allow"""
    lab, n, sc = got
    worst = np.inf
    for b, Tb in enumerate(lens):
        assert (n[b] >= 0).all() and (n[b] <= Tb).all() and np.isfinite(sc[b]).all(), (tag, b)
        assert (np.diff(sc[b]) <= 0).all(), (tag, b)
        hyps = [tuple(lab[b, k, :n[b, k]]) for k in range(nbest)]
        assert len(set(hyps)) == nbest, (tag, b)
        for k, h in enumerate(hyps):
            assert (lab[b, k, n[b, k]:] == -1).all() and min(h) >= 0, (tag, b, k)
            full = bound(b, h)
            worst = min(worst, full - float(sc[b, k]))
            assert sc[b, k] <= full + allow(np.array([full]))[0], (tag, b, k, sc[b, k], full)
    print("%s: a score is at least %.3g below its string's float64 bound (allowed: %.3g above); lengths %s"
          % (tag, worst, allow(np.array([float(sc.min())]))[0], n[:, 0].tolist()))


@pytest.mark.parametrize("model", ["acoustic", "trigram"])
def test_utterance_length_one_shot_equals_streamed_and_scores_are_lower_bounds(gpu, model):
    """case 2"""
    c = K.UTT
    B, T, Cc, W, nbest, blank, lens, mf = (c[k] for k in ("B", "T", "C", "W", "nbest", "blank", "lens", "mf"))
    assert [len(K.blocks(n, W)) for n in lens] == [2, 2, 1] and mf * W <= K.BT_RECORDS
    p = K.utt_probs()
    lm = _lm(Cc, blank) if model == "trigram" else None
    one = decode(gpu, p, lens, blank, W, 0, nbest, lm) if lm else decode(gpu, p, lens, blank, W, 0, nbest)
    dec = NL.CtcBeamStream(B, mf, Cc, blank, W, 0, nbest, max_labels=T, lm=lm)
    streamed = drive(gpu, dec, p, K.largest(lens, mf), mf)
    dec.close()
    eq(one, streamed, "one-shot against %d pushes of %d frames" % (len(K.largest(lens, mf)), mf))
    assert one[1][0, 0] > 255 and one[1][1, 0] > 255                                 # strings beyond the record's low byte
    if lm:
        bound = lambda b, h: -_ctc_loss64(p[b, :lens[b]], h, blank) + lm.score(h, with_final=True)
        allow = lambda ref: tol_lm(_rounds(T, K.LM["D"]), ref)
    else:
        bound = lambda b, h: -_ctc_loss64(p[b, :lens[b]], h, blank)
        allow = lambda ref: tol(T, ref)
    _assert_nbest_is_sound(model, one, lens, nbest, T, bound, allow)
    if lm:
        lm.close()


@pytest.mark.parametrize("model", ["acoustic", "trigram"])
def test_one_push_longer_than_a_block(gpu, model):
    """case 3: the commit of a single push of 96 frames stages 32 + 64; three pushes of 32 stage one block each"""
    name, long_mf, short_mf = K.PUSH["name"], K.PUSH["long_mf"], K.PUSH["short_mf"]
    seed, scale, T, Cc, W, nbest, want_blocks = K.PARITY[name]
    assert K.blocks(long_mf, W) == want_blocks and len(K.blocks(short_mf, W)) == 1
    p, blank = K.parity_probs(name), Cc - 1
    lm = _lm(Cc, blank) if model == "trigram" else None
    one = decode(gpu, p, [T], blank, W, 0, nbest, lm) if lm else decode(gpu, p, [T], blank, W, 0, nbest)
    if not lm:                                                                       # the one-shot call is case 1's
        lab, n, sc, gap = K.parity_premise(name)
        np.testing.assert_array_equal(one[1], n)
        np.testing.assert_array_equal(one[0], lab)
    assert (one[1] > 0).all()
    for mf in (long_mf, short_mf):
        dec = NL.CtcBeamStream(1, mf, Cc, blank, W, 0, nbest, max_labels=T, lm=lm)
        got = drive(gpu, dec, p, [[mf]] * (T // mf), mf)
        dec.close()
        eq(got, one, "%d frames a push" % mf)
    if lm:
        lm.close()


def test_class_cut_beyond_its_grid(gpu):
    """case 4: 67200 frames in one call against the same rows in 12 calls of 5600 frames"""
    c = K.CUT
    B, T, Cc, W, nbest, blank, cutoff, part = (c[k] for k in ("B", "T", "C", "W", "nbest", "blank", "cutoff", "part"))
    assert B * T > K.CUT_GRID_CAP * K.CUT_FRAMES_PER_WG >= part * T
    p, lens = K.cut_case()
    whole = decode(gpu, p, lens, blank, W, cutoff, nbest)
    parts = [decode(gpu, p[i:i + part].copy(), lens[i:i + part], blank, W, cutoff, nbest) for i in range(0, B, part)]
    eq(whole, tuple(np.concatenate([q[k] for q in parts]) for k in range(3)), "1200 rows against 12 x 100")
    lab, n, sc = whole
    empty = np.array(lens) == 0
    assert (n[empty, 0] == 0).all() and (sc[empty, 0] == 0.0).all() and (n[~empty, 0] >= 0).all() and np.isfinite(sc[~empty, 0]).all()
    assert n[B - 1, 0] > 0 and (lab[B - 1, 0, :n[B - 1, 0]] >= 0).all()                # a row of the stride loop's second round decodes
