"""RNN-Transducer beam search on the device (csrc/hip/rnnt_beam.hip) beyond one pass of the workgroup: the widths between the toy models of
tests/test_gpu_rnnt_beam.py and the advertised limits (H, J <= 1024, V <= 8192, beam width <= 32), against tests/rnnt_beam_reference.py.

The rules are those of test_gpu_rnnt_beam.py: labels and lengths are compared for EQUALITY with the float64 reference, on inputs where
the reference is unambiguous (cut_gap and order_gap >= GAP = 1e-3, the float32 restatement returns the same labels, a live row's n-best
holds labels).  The cases, their seeds (chosen on the CPU; nothing about them comes from a device) and these premises live in
tests/rnnt_wide_cases.py; tests/test_rnnt_decode_wide_premises.py checks them without a device, and every test here asserts them again
before it trusts the comparison.

The widest beam (b4): seeds 0 .. 359 of the wide_identity family (H = J = 33, V 70, T 4, max_symbols_per_frame 3, label_bias -1.5,
out_scale 3) were searched on the CPU at beam width 32; 105 of them have cut_gap and order_gap >= GAP, and seed 125 has the largest
smaller-of-the-two (cut 5.8e-3, order 5.7e-3).  So the case runs at NNTK_RNNT_BEAM_MAX_W itself; its B holds up to 128 entries.

Score tolerance, from the CPU alone: 4 x the largest |float32 restatement - float64| score over the cases of this file
(rnnt_wide_cases.beam_score_tol; 4 because the device's summation order differs).  Measured: largest float32 error 5.682e-6 (b3, the
limits), so the tolerance is 2.273e-5; the device's largest error on these cases is 1.503e-6 (b4, over all 32 survivors; 1.211e-6 within
the n-best, b1) and is printed by every test that compares scores.

Which test reaches which branch (the constants are mirrored in rnnt_wide_cases.py; each case asserts its side, beam_thresholds):

  branch of rnnt_beam_kernel<R> / nntk_shim_rnnt_beam                      test                            proof it is on that side
  step_group's gate loop beyond one pass (4H > 1024)                        passes_and_the_groups_opt_in    1024 < 4H = 1040; also b2, b3
  rd_matvec in groups of four (J > 4) together with V > 1024                passes_and_the_groups_opt_in    J = 260, 2048 < V = 2300 < 3072
  LDS opt-in for the group of four                                          passes_and_the_groups_opt_in    beam_group answers 4; float part 49280 > 49152
  ... the same bits one by one                                              passes_and_the_groups_opt_in    beam_group answers 1 while pinned
  automatic fall-back to R = 1 at beam width > 1                            automatic_fall_back             beam_group(4, ...) answers 1, nothing pinned
  the model at the limits                                                   the_limits                      beam_fits answers 1 at 1024 / 1024 / 8192
  merge scan `e < nB; e += 64` beyond one pass                              the_widest_beam                 the reference's largest |B| (128) > 64, merges > 0
  beam width 32: eight groups of four a depth, 32 selection rounds          the_widest_beam                 W == 32, 32 survivors a row
  state save / restore `i < nA * SF; i += 1024` beyond one pass             wide_stream                     nA (2H + J) = 8 * 780 > 1024
"""
import numpy as np
import pytest

import rnnt_wide_cases as K
from nntoolkitcore_amd import capi, layers as NL
from rnnt_beam_device import assert_equals_reference, decoder as _decoder, host as _host, same as _same, to_device as _t

pytestmark = pytest.mark.gpu


def _decode(gpu, dec, c, n=None):
    return _host(dec.beam_decode(_t(gpu, c["enc"]), c["n"] if n is None else n, c["W"], c["nbest"], c["max_labels"]))


def _premise(name):
    """the CPU premises again, and what the shims answer with nothing pinned"""
    L = capi.load()
    r64 = K.beam_premise(name)
    W, H, J, V = K.beam_thresholds(name)
    L.nntk_shim_rnnt_beam_set_group(0)
    assert L.nntk_shim_rnnt_beam_fits(H, J, V) == 1 and L.nntk_shim_rnnt_beam_group(W, H, J, V) == K.beam_expected_group(name), name
    return r64


def _check(gpu, name):
    r64 = _premise(name)
    c = K.beam_case(name)
    dec = _decoder(gpu, c)
    got = _decode(gpu, dec, c)
    dec.destroy()
    assert_equals_reference(name, got, r64, c["nbest"], K.beam_score_tol)
    return c, r64, got


def test_passes_and_the_groups_opt_in(gpu):
    L = capi.load()
    r64 = _premise("b1")
    c = K.beam_case("b1")
    m = c["m"]
    dec = _decoder(gpu, c)
    try:
        auto = _decode(gpu, dec, c)
        L.nntk_shim_rnnt_beam_set_group(1)
        assert L.nntk_shim_rnnt_beam_group(c["W"], m["H"], m["J"], m["V"]) == 1
        single = _decode(gpu, dec, c)
    finally:
        L.nntk_shim_rnnt_beam_set_group(0)
        dec.destroy()
    assert_equals_reference("b1", auto, r64, c["nbest"], K.beam_score_tol)
    assert _same(auto, single)


def test_automatic_fall_back(gpu):
    c, _, _ = _check(gpu, "b2")
    assert c["W"] == 4


def test_the_limits(gpu):
    c, _, _ = _check(gpu, "b3")
    assert c["W"] == 2 and c["m"]["H"] == c["m"]["J"] == K.MAX_WIDTH and c["m"]["V"] == K.MAX_V


def test_the_widest_beam(gpu):
    c, r64, got = _check(gpu, "b4")
    assert c["W"] == K.BEAM_MAX_W and r64["max_b"].max() > K.WAVE and r64["merges"].sum() > 0
    # every survivor, not the n-best alone: the 32-way selection against the reference's final set (as a set: order_gap vouches for
    # the order of the first nbest + 1 only, cut_gap for who survives)
    dec = _decoder(gpu, c)
    labels, lengths, scores = _host(dec.beam_decode(_t(gpu, c["enc"]), c["n"], c["W"], c["W"], c["max_labels"]))
    dec.destroy()
    worst = 0.0
    for b, final in enumerate(r64["final"]):
        assert len(final) == c["W"]
        have = {tuple(labels[b, k, :lengths[b, k]].tolist()): float(scores[b, k]) for k in range(c["W"])}
        assert sorted(have) == sorted(tuple(r[0]) for r in final), b
        assert all(scores[b, k] >= scores[b, k + 1] for k in range(c["W"] - 1)), b
        worst = max([worst] + [abs(have[tuple(r[0])] - float(r[1])) for r in final])
    print("b4, all 32 survivors: largest device score error %.3e (tolerance %.3e)" % (worst, K.beam_score_tol()))
    assert worst <= K.beam_score_tol()


def test_wide_stream(gpu):
    """b1's model with a state handle: after every push the result equals the one-shot call on the frames so far, bit for bit"""
    _premise("b1")
    c = K.beam_case("b1")
    B, T, J = c["enc"].shape
    SF = 2 * c["m"]["H"] + c["m"]["J"]
    carried = [len(f) for f in K.beam_stream_reference()["final"]]
    assert all(nA * SF > K.LANES for nA in carried), (carried, SF)                    # the copy loops run more than one pass
    dec = _decoder(gpu, c)
    s = NL.RnntBeamStream(dec, B, c["W"], c["nbest"], c["max_labels"])
    seen = [0] * B
    for split in (K.B5_FIRST, [n - f for n, f in zip(c["n"], K.B5_FIRST)]):
        chunk = np.full((B, max(max(split), 1), J), np.nan, np.float32)
        for b in range(B):
            chunk[b, :split[b]] = c["enc"][b, seen[b]:seen[b] + split[b]]
            seen[b] += split[b]
        got = _host(s.push(_t(gpu, chunk), split))
        assert _same(got, _decode(gpu, dec, c, n=seen)), seen
    assert seen == c["n"]
    assert_equals_reference("b1 streamed", got, K.beam_reference("b1")[0], c["nbest"], K.beam_score_tol)
    s.close(); dec.destroy()
