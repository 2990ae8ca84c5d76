"""Token-and-duration forced alignment (csrc/hip/rnnt_tdt_align.hip) against the float64 Viterbi of tests/rnnt_tdt_align_reference.py, which
tests/test_rnnt_tdt_align_host.py pins to enumeration; that file also asserts every row's gap and which rows have no path.  Score: at
most FACTOR x the float32 restatement's error, or FLOOR.  Path: the reference's for every row whose smallest decision gap exceeds
16 (T_b + U_b + 2) 2^-24, which is every row of every case here (asserted: none is left out).  Every row's
path is also walked from (0, 0) to (T_b, U_b): see _assert_valid.  NaN in all padding cells; outputs prefilled with sentinels.
DESIGN.md, "Token-and-duration forced alignment", has the cases' reasons: why `underflow` expects another path than the planted one,
and why `blocks` (T = 300, 299 labels: three staged blocks of 218 diagonals) crosses every block edge by a jump."""
import math

import numpy as np
import pytest
import torch

import rnnt_cases as K
import rnnt_tdt_align_reference as A
from rnnt_reference import log_softmax
from nntoolkitcore_amd import layers as NL

pytestmark = pytest.mark.gpu

SENT_I, SENT_F = -77, 7.5                            # what the outputs are prefilled with: every element has to be written
CASES = ["ragged_5_0_0", "ragged_64_63_0", "ragged_257_100_0", "ragged_5_2_0.05", "d12", "d12_short", "d02", "d018", "underflow",
         "U300", "U512", "long", "blocks"]
INTS = ["label_frames", "label_durations", "frame_labels", "frame_durations"]


def _logp_tol(v):
    return 2 * 4 * 2.0 ** -23 + abs(v) * 2.0 ** -23


def _run(gpu, c, x=None, only_scores=False):
    x = K.with_nan_padding(c) if x is None else x
    d = torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    B, T, U1, _ = x.shape
    shapes = [(B, U1 - 1), (B, U1 - 1), (B, T), (B, T), (B, U1 - 1), (B, T), (B,)]
    outs = [torch.full(s, SENT_I if k < 4 else SENT_F, dtype=torch.int32 if k < 4 else torch.float32, device=gpu) for k, s in enumerate(shapes)]
    given = [False] * 6 + outs[6:] if only_scores else outs
    NL.rnnt_tdt_align_device(d, c["labels"], c["durs"], input_lengths=c["lens"], blank=c["blank"], sigma=c["sigma"],
                             **dict(zip(INTS + ["label_logp", "frame_logp", "scores"], given)))
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _assert_valid(tag, c, got):
    """the moves are a path with durations of the table; each logp within LOGP_TOL of the float64 log_softmax values of both heads (the
    classic test's bound, its fixed term doubled: a move multiplies two emissions); their sum the score, per-move term doubled"""
    lf, ld, fl, fd, llp, flp, sc = got
    assert not any((o == SENT_I).any() for o in got[:4]) and not any((o == SENT_F).any() for o in got[4:]), tag
    V, durs = c["x"].shape[3] - len(c["durs"]), list(c["durs"])
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):
        U = len(lab)
        assert (lf[b, U:] == -1).all() and (ld[b, U:] == -1).all() and (fl[b, n:] == -1).all() and (fd[b, n:] == -1).all(), (tag, b)
        assert not llp[b, U:].any() and not flp[b, n:].any(), (tag, b)
        if sc[b] == -math.inf:
            assert all((o[b] == -1).all() for o in got[:4]) and not llp[b].any() and not flp[b].any(), (tag, b)
            continue
        x = c["x"][b, :n, :U + 1].astype(np.float64)
        lt, ldp = log_softmax(x[..., :V]) - c["sigma"], log_softmax(x[..., V:])
        assert (np.diff(lf[b, :U]) >= 0).all(), (tag, b)
        t = u = blanks = 0
        while (t, u) != (n, U):                      # the move out of (t, u): label u if it is emitted here, else the frame's blank
            y = u < U and lf[b, u] == t
            assert y or fl[b, t] == u, (tag, b, t, u)
            d, lp, want = (ld[b, u], llp[b, u], lt[t, u, lab[u]]) if y else (fd[b, t], flp[b, t], lt[t, u, c["blank"]])
            assert d in durs and (y or d > 0), (tag, b, t, u, d)
            want += ldp[t, u, durs.index(d)]
            assert abs(lp - want) <= _logp_tol(want), (tag, b, t, u, lp, want)
            t, u, blanks = t + d, u + y, blanks + (not y)
            assert t < n or (t, u) == (n, U), (tag, b, t, u)
        assert (fl[b] >= 0).sum() == blanks and ((fl[b] >= 0) == (fd[b] >= 0)).all() and not flp[b][fl[b] < 0].any(), (tag, b)
        total = llp[b].astype(np.float64).sum() + flp[b].astype(np.float64).sum()
        assert abs(total - sc[b]) <= (n + U + 2) * 2.0 ** -24 * (4.0 + abs(float(sc[b]))), (tag, b, total, sc[b])


def _check(gpu, name):
    c, (rows, s32) = A.case(name), A.reference(name)
    got = _run(gpu, c)
    _assert_valid(name, c, got)
    for b, r in enumerate(rows):
        if r["score"] == -math.inf:
            assert got[6][b] == -math.inf and b in c["inf"], (name, b)
            continue
        e, e32 = abs(float(got[6][b]) - r["score"]) / abs(r["score"]), abs(s32[b] - r["score"]) / abs(r["score"])
        print("%s row %d score %.9g: err %.2e, float32 err %.2e, gap %.2e" % (name, b, r["score"], e, e32, r["gap"]))
        assert e <= max(K.FACTOR * e32, K.FLOOR), (name, b, e, e32)
        assert r["gap"] > A.gap_threshold(c["lens"][b], len(c["labels"][b]))          # every row of these cases: none is left out
        assert all(o[b, :len(r[k])].tolist() == r[k].tolist() for k, o in zip(INTS, got)), (name, b)
    return c, got


@pytest.mark.parametrize("name", CASES)
def test_matches_float64(gpu, name):
    c, got = _check(gpu, name)
    if name == "blocks":                             # more diagonals than two staged blocks hold
        assert c["lens"][0] + c["x"].shape[2] - 1 > 2 * (65536 // min(c["lens"][0], c["x"].shape[2]))
    if name == "underflow":                          # the best path (see above), move for move; its probability is below the f32 range
        assert [o[0].tolist() for o in got[:4]] == [[0, 1, 4, 5], [1, 1, 1, 0], [-1, -1, 2, -1, -1, 4], [-1, -1, 2, -1, -1, 1]]
        assert np.exp(np.float32(got[6][0])) == 0.0 and np.isfinite(got[6][0])


def _equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_structure(gpu):
    """the same bits over two calls, with only d_scores given, alone and in the batch, from the host form; scores against the loss"""
    c = A.case("ragged_5_0_0")
    got = _run(gpu, c)
    assert _equal(got, _run(gpu, c)) and np.array_equal(got[6], _run(gpu, c, only_scores=True)[6])
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):
        u, one = len(lab), dict(c, labels=[lab], lens=[n])
        alone = _run(gpu, one, x=c["x"][b:b + 1, :n, :len(lab) + 1])
        assert _equal([o[b:b + 1, :k] for o, k in zip(got, (u, u, n, n, u, n))] + [got[6][b:b + 1]], alone), b
    host = NL.rnnt_tdt_align(c["x"], c["labels"], c["durs"], input_lengths=c["lens"], blank=c["blank"], sigma=c["sigma"])
    assert _equal(_run(gpu, c, x=c["x"]), host)

    for name in ("ragged_5_2_0.05", "d02", "d018"):  # never above -loss, bit for bit: max <= sum holds through every rounding
        c = A.case(name)
        loss, _ = NL.rnnt_tdt_loss_device(torch.from_numpy(K.with_nan_padding(c)).to(gpu), c["labels"], c["durs"], input_lengths=c["lens"],
                                          blank=c["blank"], sigma=c["sigma"], want_grad=False)
        assert (_run(gpu, c)[6] <= -loss.cpu().numpy()).all(), name
