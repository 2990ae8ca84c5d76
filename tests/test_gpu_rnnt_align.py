"""RNN-Transducer forced alignment (csrc/hip/rnnt_align.hip) on stored scores and on the joiner's inputs, against
tests/rnnt_align_reference.py.

Reference: the float64 log-space Viterbi with the contract's tie-break (pinned to enumeration by tests/test_rnnt_align_host.py, which
also asserts every premise of the cases used here without a device).

Score, judged as tests/test_gpu_rnnt.py judges the loss, measured and not fixed in advance: per row the device score's error against
float64, relative to |score|, is at most FACTOR = 4 x the error of the float32 torch restatement, or FLOOR = 16 * 2^-24 where that is
smaller (the restatement can be exact where the device rounds once per lattice step).

Path: label_frames and frame_labels equal the reference's for every row whose smallest decision gap exceeds
8 (T_b + U_b + 2) 2^-24 (rnnt_align_reference.gap_threshold); at most a quarter of a case's rows may fall below it, none in the
per-instantiation cases -- and none does in any case here (the host test asserts it).  Every row's path, compared exactly or not, is
checked for validity: monotone frames, frame_labels consistent with label_frames, the logp arrays equal to the float64 log-softmax at
the path's cells, their sum equal to the score.  LOGP_TOL: the emission's mantissa comes from a float32 exp2 (2 ulp of 2^-23 in p, that
much absolute in ln p), lse from float32 exponentials summed in double (one more), and the result is rounded to float32: 4 * 2^-23 +
|logp| 2^-23.

Tie-break on flat scores: the issue's text expects every label in the LAST frame; the recursion it makes part of the contract (the
blank move into a cell wins ties) gives every label in frame 0 -- the walk back from (T_b-1, U_b) takes blanks down to frame 0 -- and
enumeration with that tie-break agrees (test_rnnt_align_host.py).  The test asserts what the contract gives."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import rnnt_align_reference as A
import rnnt_cases as K
import rnnt_reference as R
from nntoolkitcore_amd import capi, layers as NL

pytestmark = pytest.mark.gpu

SENT_I, SENT_F = -77, 7.5                            # what the outputs are prefilled with: every element has to be written


def _logp_tol(v):
    return 4 * 2.0 ** -23 + abs(v) * 2.0 ** -23


def _outputs(gpu, B, T, maxL):
    return dict(label_frames=torch.full((B, maxL), SENT_I, dtype=torch.int32, device=gpu),
                frame_labels=torch.full((B, T), SENT_I, dtype=torch.int32, device=gpu),
                label_logp=torch.full((B, maxL), SENT_F, device=gpu), frame_logp=torch.full((B, T), SENT_F, device=gpu),
                scores=torch.full((B,), SENT_F, device=gpu))


def _run(gpu, x, labels, lens, blank):
    d = torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    B, T, U1, _ = x.shape
    outs = NL.rnnt_align_device(d, labels, input_lengths=lens, blank=blank, **_outputs(gpu, B, T, U1 - 1))
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in outs)


def _run_fused(gpu, enc, pred, out, labels, lens, blank, kind):
    e, p, o = (torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (enc, pred, out))
    outs = NL.rnnt_fused_align_device(e, p, o, labels, input_lengths=lens, blank=blank, activation=kind,
                                      **_outputs(gpu, enc.shape[0], enc.shape[1], pred.shape[1] - 1))
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in outs)


def _assert_valid(tag, got, lp_rows, labels, lens, blank):
    """every row's path is a path, whatever the reference's is; lp_rows: per row the float64 log-softmax of its live cells"""
    lf, fl, llp, flp, sc = got
    for b, (n, lab) in enumerate(zip(lens, labels)):
        U = len(lab)
        assert (lf[b, U:] == -1).all() and (fl[b, n:] == -1).all() and not llp[b, U:].any() and not flp[b, n:].any(), (tag, b)
        if sc[b] == -math.inf:
            assert (lf[b] == -1).all() and (fl[b] == -1).all() and not llp[b].any() and not flp[b].any(), (tag, b)
            continue
        f = lf[b, :U]
        assert (f >= 0).all() and (f < n).all() and (np.diff(f) >= 0).all(), (tag, b, f)
        assert fl[b, :n].tolist() == [int((f <= t).sum()) for t in range(n)], (tag, b)
        lp = lp_rows[b]
        for i in range(U):
            want = lp[f[i], i, lab[i]]
            assert abs(llp[b, i] - want) <= _logp_tol(want), (tag, b, i, llp[b, i], want)
        for t in range(n):
            want = lp[t, fl[b, t], blank]
            assert abs(flp[b, t] - want) <= _logp_tol(want), (tag, b, t, flp[b, t], want)
        total = llp[b].astype(np.float64).sum() + flp[b].astype(np.float64).sum()
        # the score is the ln of a product rounded once per move (2^-24 each, absolute in ln); each of the n + U terms and the score
        # itself are rounded to float32 (at most |score| 2^-24 each)
        assert abs(total - sc[b]) <= (n + U + 2) * 2.0 ** -24 * (2.0 + abs(float(sc[b]))), (tag, b, total, sc[b])


def _assert_matches(tag, got, rows, s32, lens, labels, allow_left_out=0.25):
    lf, fl, _, _, sc = got
    out = 0
    for b, r in enumerate(rows):
        U, n = len(labels[b]), lens[b]
        if r["score"] == -math.inf:
            assert sc[b] == -math.inf, (tag, b)
            continue
        assert np.isfinite(sc[b]), (tag, b)
        e, e32 = abs(sc[b] - r["score"]) / abs(r["score"]), abs(s32[b] - r["score"]) / abs(r["score"])
        print("%s row %d score %.9g: err %.2e, torch f32 err %.2e, gap %.2e" % (tag, b, r["score"], e, e32, r["gap"]))
        assert e <= max(K.FACTOR * e32, K.FLOOR), (tag, b, e, e32)
        if r["gap"] > A.gap_threshold(n, U):
            assert lf[b, :U].tolist() == r["label_frames"].tolist() and fl[b, :n].tolist() == r["frame_labels"].tolist(), (tag, b)
        else:
            out += 1
    assert out <= allow_left_out * len(rows), (tag, out)


def _check(gpu, name, allow_left_out=0.25, nan_padding=True):
    c = A.case(name)
    rows, s32 = A.reference(name)
    got = _run(gpu, K.with_nan_padding(c) if nan_padding else c["x"], c["labels"], c["lens"], c["blank"])
    lps = [R.log_softmax(c["x"][b, :n, :len(lab) + 1]) for b, (n, lab) in enumerate(zip(c["lens"], c["labels"]))]
    _assert_valid(name, got, lps, c["labels"], c["lens"], c["blank"])
    _assert_matches(name, got, rows, s32, c["lens"], c["labels"], allow_left_out)
    return c, got


@pytest.mark.parametrize("name", ["ragged", "ragged_V64", "ragged_V5", "ragged_V257", "random", "long"])
def test_matches_float64(gpu, name):
    """the small ragged batch (blank 2, NaN in all padding cells), VEC (V = 64) and non-VEC (V = 5, 257) emission reads, the random
    batch, longer free paths"""
    _check(gpu, name)


@pytest.mark.parametrize("T,maxL", list(A.INSTANTIATIONS))
def test_every_instantiation_of_the_viterbi_kernel(gpu, T, maxL):
    _check(gpu, "inst_%d_%d" % (T, maxL), allow_left_out=0.0)


def test_backtrace_across_staged_blocks(gpu):
    c, got = _check(gpu, "two_blocks", allow_left_out=0.0)
    assert c["lens"][0] + len(c["labels"][0]) > A.BT_DIAGS


def test_tie_break_on_flat_scores(gpu):
    """every path ties exactly (equal emissions multiplied in the same order); the blank move wins every tie: all labels in frame 0"""
    c, (lf, fl, llp, flp, sc) = _check(gpu, "flat", allow_left_out=1.0)      # gap 0 everywhere: the exact expectation is stated here
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):
        assert lf[b, :len(lab)].tolist() == [0] * len(lab) and fl[b, :n].tolist() == [len(lab)] * n, b
        assert abs(sc[b] + (n + len(lab)) * math.log(4.0)) <= 1e-5


def test_against_the_loss(gpu):
    c, (lf, _, _, _, sc) = _check(gpu, "peaked")
    d = torch.from_numpy(K.with_nan_padding(c)).to(gpu)
    loss, _ = NL.rnnt_loss_device(d, c["labels"], input_lengths=c["lens"], blank=c["blank"], want_grad=False)
    loss = loss.cpu().numpy()
    for b, lab in enumerate(c["labels"]):
        assert lf[b, :len(lab)].tolist() == c["paths"][b]
        assert abs(sc[b] + loss[b]) <= K.FLOOR * max(1.0, abs(float(loss[b]))) + 1e-9, (b, sc[b], loss[b])
    c, (_, _, _, _, sc) = _check(gpu, "random")
    loss, _ = NL.rnnt_loss_device(torch.from_numpy(c["x"]).to(gpu), c["labels"], input_lengths=c["lens"], blank=c["blank"], want_grad=False)
    loss = loss.cpu().numpy()
    assert (sc <= -loss + K.FLOOR * np.abs(loss)).all()


def test_range(gpu):
    c, (lf, _, _, _, sc) = _check(gpu, "range")
    assert np.isfinite(sc[0]) and -2780.0 < sc[0] < -2750.0 and lf[0].tolist() == c["paths"][0]


def test_minus_infinity_scores(gpu):
    c, (lf, fl, llp, flp, sc) = _check(gpu, "forced", nan_padding=False)
    assert lf[0].tolist() == [0, 0, 0] and np.isfinite(sc[0]) and np.isfinite(sc[2])
    assert sc[1] == -math.inf and (lf[1] == -1).all() and (fl[1] == -1).all() and not llp[1].any() and not flp[1].any()


def test_against_greedy_decoding(gpu):
    """aligning the greedy decoder's own labels on teacher-forced logits of the same weights returns the decoder's frames"""
    import rnnt_decode_reference as D
    m = A.greedy_model()
    g = D.greedy_decode(m["embed"], m["lstm"], m["proj"], m["out"], m["enc"], n_frames=m["n"], blank=m["blank"], activation="tanh",
                        max_symbols_per_frame=100)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    dec = NL.RnntDecoder(t(m["embed"]), t(m["lstm"]), t(m["proj"]), t(m["out"]), blank=m["blank"], joint_activation="tanh",
                         max_symbols_per_frame=100)
    labels, frames, lengths, _ = (o.cpu().numpy() for o in dec.decode(t(m["enc"]), m["n"], None))
    dec.destroy()
    assert [labels[b, :lengths[b]].tolist() for b in range(3)] == g["labels"]
    maxL = int(lengths.max())
    x = A.teacher_forced_logits(m, g["labels"], maxL).astype(np.float32)
    lf = _run(gpu, x, g["labels"], m["n"], m["blank"])[0]
    for b in range(3):
        assert lf[b, :lengths[b]].tolist() == frames[b, :lengths[b]].tolist() == g["frames"][b], b


# ---- the fused form ----

def _check_fused(gpu, name, kind):
    c = A.fused_case(name)
    x64, rows, s32 = A.fused_reference(name, kind)
    enc, pred = K.with_nan_padding(c)
    got = _run_fused(gpu, enc, pred, c["out"], c["labels"], c["lens"], c["blank"], kind)
    plain = _run(gpu, x64.astype(np.float32), c["labels"], c["lens"], c["blank"])
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1]), (name, kind)
    tag = "fused %s %s" % (name, kind)
    for b, r in enumerate(rows):
        assert r["gap"] > A.FUSED_GAP
        U, n = len(c["labels"][b]), c["lens"][b]
        assert got[0][b, :U].tolist() == r["label_frames"].tolist() and got[1][b, :n].tolist() == r["frame_labels"].tolist(), (tag, b)
        e, e32 = abs(got[4][b] - r["score"]) / abs(r["score"]), abs(s32[b] - r["score"]) / abs(r["score"])
        print("%s row %d score %.9g: err %.2e, torch f32 err %.2e" % (tag, b, r["score"], e, e32))
        assert e <= max(K.FACTOR * e32, K.FLOOR), (tag, b, e, e32)
    # validity against the float64 logits; the fused logits are a float32 chain over J: J 2^-24 max |logit| on top of LOGP_TOL
    lf, fl, llp, flp, sc = got
    J = c["enc"].shape[2]
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):
        lp = R.log_softmax(x64[b, :n, :len(lab) + 1])
        extra = 2 * J * 2.0 ** -24 * np.abs(x64[b, :n, :len(lab) + 1]).max()
        for i in range(len(lab)):
            want = lp[lf[b, i], i, lab[i]]
            assert abs(llp[b, i] - want) <= _logp_tol(want) + extra, (tag, b, i)
        for t_ in range(n):
            want = lp[t_, fl[b, t_], c["blank"]]
            assert abs(flp[b, t_] - want) <= _logp_tol(want) + extra, (tag, b, t_)
        assert not llp[b, len(lab):].any() and not flp[b, n:].any() and (lf[b, len(lab):] == -1).all() and (fl[b, n:] == -1).all()
    return c, got


@pytest.mark.parametrize("kind", A.FUSED_KINDS)
@pytest.mark.parametrize("J,V,blank", A.FUSED_RAGGED)
def test_fused_ragged(gpu, J, V, blank, kind):
    _check_fused(gpu, "ragged_%d_%d_%d" % (J, V, blank), kind)


@pytest.mark.parametrize("T,U", A.FUSED_CELLS)
def test_fused_cell_counts_around_one_tile(gpu, T, U):
    assert T * (U + 1) in (20, 32, 33)
    _check_fused(gpu, "cells_%d_%d" % (T, U), "tanh")


def test_fused_wide_lattice(gpu):
    _check_fused(gpu, "wide", "tanh")


# ---- structure, in both forms ----

def _equal(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_structure(gpu):
    """every element written (the sentinels are gone), the same bits over two calls, a row's bits independent of its position in the
    batch and of the T / max_label_len padding"""
    c = A.case("ragged")
    x = K.with_nan_padding(c)
    got = _run(gpu, x, c["labels"], c["lens"], c["blank"])
    assert not any((o == SENT_I).any() for o in got[:2]) and not any((o == SENT_F).any() for o in got[2:])
    assert _equal(got, _run(gpu, x, c["labels"], c["lens"], c["blank"]))
    order = [5, 2, 7, 0, 3, 6, 1, 4]
    perm = _run(gpu, x[order], [c["labels"][b] for b in order], [c["lens"][b] for b in order], c["blank"])
    assert _equal([o[order] for o in got], perm)
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):
        u = len(lab)
        one = _run(gpu, np.ascontiguousarray(x[b:b + 1, :n, :u + 1]), [lab], [n], c["blank"])
        assert _equal([got[0][b:b + 1, :u], got[1][b:b + 1, :n], got[2][b:b + 1, :u], got[3][b:b + 1, :n], got[4][b:b + 1]], one), b


def test_fused_structure(gpu):
    c = A.fused_case("ragged_67_257_100")
    args = (c["out"], c["labels"], c["lens"], c["blank"], "tanh")
    got = _run_fused(gpu, c["enc"], c["pred"], *args)
    assert not any((o == SENT_I).any() for o in got[:2]) and not any((o == SENT_F).any() for o in got[2:])
    assert _equal(got, _run_fused(gpu, c["enc"], c["pred"], *args))
    order = [2, 0, 1]
    perm = _run_fused(gpu, c["enc"][order], c["pred"][order], c["out"], [c["labels"][b] for b in order], [c["lens"][b] for b in order],
                      c["blank"], "tanh")
    assert _equal([o[order] for o in got], perm)
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):
        u = len(lab)
        one = _run_fused(gpu, c["enc"][b:b + 1, :n], c["pred"][b:b + 1, :u + 1], c["out"], [lab], [n], c["blank"], "tanh")
        assert _equal([got[0][b:b + 1, :u], got[1][b:b + 1, :n], got[2][b:b + 1, :u], got[3][b:b + 1, :n], got[4][b:b + 1]], one), b


def _raw_args(gpu, fused):
    """(call, leading arguments, trailing int arguments, B, T, maxL, workspace) for the C entry points"""
    L = capi.load()
    ip = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(capi.ip)
    dp = lambda t: C.c_void_p(t.data_ptr())
    if fused:
        c = A.fused_case("ragged_5_5_2")
        B, T, J = c["enc"].shape
        maxL, V = c["pred"].shape[1] - 1, 5
        keep = [torch.from_numpy(a).to(gpu) for a in (c["enc"], c["pred"], c["out"])]
        ws = torch.empty(L.nntk_rnnt_fused_align_workspace_floats(B, T, maxL, J, V), device=gpu)
        head = [dp(t) for t in keep] + [B, T, J, V, 1]
        fn = L.nntk_rnnt_fused_align_device
    else:
        c = A.case("ragged")
        B, T, U1, V = c["x"].shape
        maxL = U1 - 1
        keep = [torch.from_numpy(c["x"]).to(gpu)]
        ws = torch.empty(L.nntk_rnnt_align_workspace_floats(B, T, maxL), device=gpu)
        head = [dp(keep[0]), B, T, V]
        fn = L.nntk_rnnt_align_device
    lab = np.zeros((B, maxL), np.int32)
    for b, r in enumerate(c["labels"]):
        lab[b, :len(r)] = r
    ints = dict(il=c["lens"], lab=lab, ll=[len(r) for r in c["labels"]], blank=c["blank"])

    def call(outs, **change):
        a = dict(ints, **change)
        return fn(*head, ip(a["il"]), ip(a["lab"]), ip(a["ll"]), maxL, a["blank"], *[None if o is None else dp(o) for o in outs], dp(ws))

    return call, keep, B, T, maxL


@pytest.mark.parametrize("fused", [False, True])
def test_null_optional_outputs_in_every_combination(gpu, fused):
    call, keep, B, T, maxL = _raw_args(gpu, fused)
    full = list(_outputs(gpu, B, T, maxL).values())
    assert call(full) == 0, capi.last_error()
    torch.cuda.synchronize()
    for mask in range(16):
        outs = list(_outputs(gpu, B, T, maxL).values())
        given = [o if mask >> k & 1 else None for k, o in enumerate(outs[:4])] + [outs[4]]
        assert call(given) == 0, (mask, capi.last_error())
        torch.cuda.synchronize()
        for k in range(5):
            if given[k] is not None:
                assert torch.equal(given[k], full[k]), (mask, k)


@pytest.mark.parametrize("fused", [False, True])
def test_refusals_write_nothing(gpu, fused):
    call, keep, B, T, maxL = _raw_args(gpu, fused)
    bad_len = [T + 1] + [1] * (B - 1)
    for change in (dict(il=bad_len), dict(il=[0] * B), dict(ll=[maxL + 1] * B), dict(blank=-1), dict(blank=99)):
        outs = list(_outputs(gpu, B, T, maxL).values())
        rc = call(outs, **change)
        torch.cuda.synchronize()
        assert rc == -1 and capi.last_error() != "", change
        assert all((o == SENT_I).all() for o in outs[:2]) and all((o == SENT_F).all() for o in outs[2:]), change


def test_host_forms_equal_the_device_forms(gpu):
    c = A.case("ragged")
    got = _run(gpu, c["x"], c["labels"], c["lens"], c["blank"])
    assert _equal(got, NL.rnnt_align(c["x"], c["labels"], input_lengths=c["lens"], blank=c["blank"]))
    c = A.fused_case("ragged_5_5_2")
    got = _run_fused(gpu, c["enc"], c["pred"], c["out"], c["labels"], c["lens"], c["blank"], "relu")
    assert _equal(got, NL.rnnt_fused_align(c["enc"], c["pred"], c["out"], c["labels"], input_lengths=c["lens"], blank=c["blank"],
                                           activation="relu"))
