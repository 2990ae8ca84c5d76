"""Greedy RNN-Transducer decoding on the device (csrc/hip/rnnt_decode.hip) beyond one pass of the workgroup: the widths between the toy
models of tests/test_gpu_rnnt_decode.py and the advertised limits (H, J <= 1024, V <= 8192), against tests/rnnt_decode_reference.py.

The rules are those of test_gpu_rnnt_decode.py: labels, frames and lengths are compared for EQUALITY with the float64 reference, on
inputs where the reference is unambiguous (smallest gap between the best and the second-best logit >= GAP = 1e-3, the float32
restatement decodes identically, the output holds blanks and labels).  The cases, their seeds (chosen on the CPU; nothing about them
comes from a device) and these premises live in tests/rnnt_wide_cases.py; tests/test_rnnt_decode_wide_premises.py checks them without a
device, and every test here asserts them again before it trusts the comparison.

Score tolerance, from the CPU alone: 4 x the largest |float32 restatement - float64| score over the cases of this file
(rnnt_wide_cases.greedy_score_tol; 4 because the device's summation order differs).  Measured: largest float32 error 8.186e-6 (g3, the
limits: sums over 1024 and 8192 terms), so the tolerance is 3.274e-5; the device's largest error on these cases is 3.388e-6 (g1) and is
printed by every test that compares scores.

Which test reaches which branch (the constants are mirrored in rnnt_wide_cases.py; each case asserts its side, greedy_thresholds):

  branch of rnnt_greedy_kernel<R> / nntk_shim_rnnt_greedy                  test                            proof it is on that side
  gate loop `n < G; n += 1024` beyond one pass (4H > 1024)                  passes[g1], [g2], limits        1024 < 4H (1040, 1204, 4096)
  logits loop / rd_wave_sum_exp with V > 1024, a partial last pass         passes[g1] (3 passes), [g2] (2)  2048 < V < 3072, V % 1024 != 0
  argmax winner in a later pass of the lane scan                            passes[g1]                      labels < 1024, in [1024, 2048), >= 2048
  sh_buf's pitch Wp taken from V, not 4H                                    passes[g1], limits, g4, g5      V > 4H
  ... and from 4H with V > 1024                                             passes[g2]                      4H > V > 1024
  rd_matvec: K % 4 = 2 (J 258), K % 4 = 1 (H = J = 301)                      passes[g1], passes[g2]          J % 4 == 2; H % 4 == 1
  the model at the limits; LDS opt-in for <1>                               limits                          shim answers 1; float part (48 KiB) + red_sum > 48 KiB
  LDS opt-in for <NNTK_RNNT_DEC_GROUP>                                      grouped_with_the_opt_in         shim answers 4; float part 49984 > 49152
  batch > 512 where four rows do not fit: fall-back to one row              grouping_refused_by_the_lds     shim answers 1 at batch 513; float part > 152 KiB
  st_f / st_i load and store with R = 4; fresh, started and frameless rows  stream_under_grouping           shim answers 4 at batch 518
"""
import numpy as np
import pytest
import torch

import rnnt_wide_cases as K
from nntoolkitcore_amd import capi, layers as NL

pytestmark = pytest.mark.gpu


def _t(gpu, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _decoder(gpu, c):
    m = c["m"]
    return NL.RnntDecoder(_t(gpu, m["embed"]), _t(gpu, m["lstm"]), _t(gpu, m["proj"]), _t(gpu, m["out"]), blank=m["blank"],
                          joint_activation=c["act"], max_symbols_per_frame=c["ms"])


def _host(outs):
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in outs)


def _rows_per_group(c):
    m = c["m"]
    return capi.load().nntk_shim_rnnt_dec_rows_per_group(c["batch"], m["H"], m["J"], m["V"])


def _premise(name):
    r64 = K.greedy_premise(name)
    K.greedy_thresholds(name)
    assert _rows_per_group(K.greedy_case(name)) == K.greedy_expected_rows_per_group(name), name
    return r64


def _assert_equals_reference(name, got, r64, rows):
    """got: the device's (labels, frames, lengths, scores) of a batch; row rows[i] of it is the reference's row i"""
    labels, frames, lengths, scores = got
    for i, b in enumerate(rows):
        k = len(r64["labels"][i])
        assert lengths[b] == k, (name, b, lengths[b], k)
        assert labels[b, :k].tolist() == r64["labels"][i] and (labels[b, k:] == -1).all(), (name, b, labels[b], r64["labels"][i])
        assert frames[b, :k].tolist() == r64["frames"][i] and (frames[b, k:] == -1).all(), (name, b)
    err = np.abs(scores[rows].astype(np.float64) - r64["scores"]).max()
    print("%s: largest device score error %.3e (tolerance %.3e); scores %s" % (name, err, K.greedy_score_tol(), r64["scores"]))
    assert err <= K.greedy_score_tol(), (name, err, K.greedy_score_tol())


def _decode_sparse(gpu, dec, c, batch, rows):
    """the case's live rows at `rows` of a batch; every other row has no frames (NaN where no frame is)"""
    T, J = c["enc"].shape[1:]
    enc = np.full((batch, T, J), np.nan, np.float32)
    n = np.zeros(batch, np.int32)
    for i, b in enumerate(rows):
        enc[b, :c["n"][i]] = c["enc"][i, :c["n"][i]]
        n[b] = c["n"][i]
    return _host(dec.decode(_t(gpu, enc), n, c["ms"] * T))


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_more_than_one_pass_of_the_gates_and_the_classes(gpu, name):
    r64 = _premise(name)
    c = K.greedy_case(name)
    dec = _decoder(gpu, c)
    got = _decode_sparse(gpu, dec, c, c["batch"], c["rows"])
    dec.destroy()
    _assert_equals_reference(name, got, r64, c["rows"])
    if name == "g1":
        labels = [v for row in r64["labels"] for v in row]
        assert any(K.LANES <= v < 2 * K.LANES for v in labels) and max(labels) >= 2 * K.LANES      # winners of a lane's second and third pass
        assert got[2][2] == 0 and got[3][2] == 0.0                                               # the row without frames


def test_the_limits(gpu):
    r64 = _premise("g3")
    c = K.greedy_case("g3")
    dec = _decoder(gpu, c)
    got = _decode_sparse(gpu, dec, c, c["batch"], c["rows"])
    again = _decode_sparse(gpu, dec, c, c["batch"], c["rows"])
    dec.destroy()
    _assert_equals_reference("g3", got, r64, c["rows"])
    assert all(np.array_equal(x, y) for x, y in zip(got, again))


def _grouped_and_alone(gpu, name):
    """a batch above the grouping batch with a handful of live rows (the others have no frames: one pass over U and out), against the
    float64 reference and, bit for bit, against the same rows in a batch that is never grouped"""
    r64 = _premise(name)
    c = K.greedy_case(name)
    m = c["m"]
    rpg = capi.load().nntk_shim_rnnt_dec_rows_per_group
    assert rpg(len(c["rows"]), m["H"], m["J"], m["V"]) == 1
    dec = _decoder(gpu, c)
    big = _decode_sparse(gpu, dec, c, c["batch"], c["rows"])
    small = _decode_sparse(gpu, dec, c, len(c["rows"]), list(range(len(c["rows"]))))
    dec.destroy()
    _assert_equals_reference(name, big, r64, c["rows"])
    for x, y in zip(big, small):
        assert np.array_equal(x[c["rows"]].view(np.int32), y.view(np.int32)), name
    idle = np.setdiff1d(np.arange(c["batch"]), c["rows"])
    assert (big[2][idle] == 0).all() and (big[3][idle] == 0.0).all() and (big[0][idle] == -1).all()


def test_grouped_with_the_opt_in(gpu):
    _grouped_and_alone(gpu, "g4")


def test_grouping_refused_by_the_lds(gpu):
    _grouped_and_alone(gpu, "g5")


def test_stream_under_grouping(gpu):
    """the small stream model at a batch that is grouped: pushes with ragged cuts equal the one-shot call bit for bit; then some rows
    are reset in mid-stream, so that every group of four holds a fresh row with frames, a fresh row without, a started row with frames
    and a started row without, in the same push"""
    r64 = _premise("g6")
    c = K.greedy_case("g6")
    B, (_, T, J) = c["batch"], c["enc"].shape
    ML = c["ms"] * T
    kind = np.arange(B) % 3                                                          # row b carries the case's row b % 3
    enc, n = c["enc"][kind], np.asarray(c["n"], np.int32)[kind]
    dec = _decoder(gpu, c)
    one = _host(dec.decode(_t(gpu, enc), n, ML))
    _assert_equals_reference("g6", one, r64, [0, 1, 2])
    for b in range(3, B):
        assert all(np.array_equal(o[b], o[b % 3]) for o in one), b
    # per push the frames a row of each kind brings: push 1 leaves the third kind fresh without frames; push 2 mixes, in every group,
    # started rows with frames, a started row without, and the row that push 1 started without frames
    cuts = np.array([[5, 3, 0], [0, 4, 3], [7, 5, 4]])
    assert cuts.sum(0).tolist() == c["n"]
    s = NL.RnntGreedyStream(dec, B, ML)
    seen = np.zeros(B, int)

    def push(w):
        """every row brings its next w[b] frames"""
        chunk = np.full((B, max(w.max(), 1), J), np.nan, np.float32)
        for b in range(B):
            chunk[b, :w[b]] = enc[b, seen[b]:seen[b] + w[b]]
            seen[b] += w[b]
        return _host(s.push(_t(gpu, chunk), w))

    same = lambda x, y, rows: all(np.array_equal(p[rows].view(np.int32), q[rows].view(np.int32)) for p, q in zip(x, y))
    every = np.arange(B)
    for cut in cuts:
        got = push(cut[kind])
    assert (seen == n).all() and same(got, one, every)
    # again up to the second push; then rows 1, 5, 9, ... restart and bring their whole input, rows 2, 6, 10, ... restart and bring
    # nothing, rows 0, 4, 8, ... go on with the rest of their frames and rows 3, 7, 11, ... bring nothing in this push: every group of
    # four holds a fresh row with frames, a fresh row without, a started row with frames and a started row without
    s.reset()
    seen[:] = 0
    for cut in cuts[:2]:
        push(cut[kind])
    full, empty, late = every[1::4], every[2::4], every[3::4]
    s.reset(np.concatenate([full, empty]))
    seen[full] = seen[empty] = 0
    w = cuts[2][kind]
    w[full], w[empty], w[late] = n[full], 0, 0
    got = push(w)
    done = np.setdiff1d(every, np.concatenate([empty, late]))
    assert (seen[done] == n[done]).all() and same(got, one, done)                    # the reset rows: the one-shot result on their input
    labels, frames, lengths, scores = got
    assert (lengths[empty] == 0).all() and (scores[empty] == 0.0).all() and (labels[empty] == -1).all() and (frames[empty] == -1).all()
    w = np.zeros(B, np.int64)
    w[late] = cuts[2][kind][late]
    got2 = push(w)                                                                   # the late rows finish; every other row keeps its bits
    assert same(got2, got, np.setdiff1d(every, late)) and same(got2, one, np.setdiff1d(every, empty))
    s.close(); dec.destroy()
