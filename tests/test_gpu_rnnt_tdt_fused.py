"""The fused token-and-duration training loss (csrc/hip/rnnt_tdt_fused.hip) against tests/rnnt_tdt_fused_reference.py: float64 numpy,
and the tolerance of tests/test_gpu_rnnt_fused.py -- per output the device's error against float64, relative to the output's largest
|value| (per row for the loss, d_enc and d_pred, over the block for d_out), is at most rnnt_cases.FACTOR x the error of the float32 torch
restatement, or FLOOR where that is smaller.  Every ratio is printed.  Inputs carry NaN in the padding, outputs are prefilled with NaN.

Which case reaches which branch (V + D columns in blocks of 32, 8 blocks a pass of the forward's waves; cells in tiles of 32):
  the duration head: (V, D) = (5, 4) one partial block; (30, 5) straddles a block edge inside a pass; (32, 4) opens a block of its own;
    (254, 5) the last block of the first pass and the first of the second, two waves; (600, 5) the third pass
  ft_logits' tails J = 1, 5, 67; J = 260: a second J block, dw<2>; 515: dw<4>; 900: gw = 4 with V + D = 145 in two groups
  tiles: the ragged batch's 126 cells end in a tile of dead cells only; 20 / 32 / 33 cells; U1 = 301: the lattice's general form"""
import math

import numpy as np
import pytest
import torch

import rnnt_cases as K
import rnnt_tdt_fused_reference as TF
from nntoolkitcore_amd import layers as NL

pytestmark = pytest.mark.gpu
NAMES = ("loss", "d_enc", "d_pred", "d_out")
D5 = [0, 1, 2, 3, 4]


def _run(gpu, c, kind="tanh", want_grad=True, arrays=None):
    enc, pred = arrays or K.with_nan_padding(c)
    e, p, o = (torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (enc, pred, c["out"]))
    nan = lambda t: torch.full_like(t, float("nan"))
    loss = torch.full((enc.shape[0],), float("nan"), device=gpu)
    g = (nan(e), nan(p), nan(o)) if want_grad else (None, None, None)
    NL.rnnt_tdt_fused_loss_device(e, p, o, c["labels"], c["durs"], input_lengths=c["lens"], blank=c["blank"], sigma=c["sigma"],
                                  activation=kind, want_grad=want_grad, loss=loss, denc=g[0], dpred=g[1], dout=g[2])
    torch.cuda.synchronize()
    return (loss.cpu(),) + tuple(t.cpu() if want_grad else None for t in g)


def _rel(x, ref):
    sc = np.abs(ref).max()
    return np.abs(x - ref).max() / sc if sc > 0 else np.abs(x).max()


def _check(gpu, tag, c, kind="tanh", inf=()):
    """inf: the rows the float64 reference must find without a path; they give +inf and exact zeros, the others the tolerance"""
    r64, r32 = TF.loss_and_grads(c, kind), TF.torch_fused(c, kind, torch.float32)
    assert [b for b, l in enumerate(r64[0]) if l == math.inf] == list(inf) and not np.isnan(r64[0]).any()
    got = [t.double().numpy() for t in _run(gpu, c, kind)]
    assert all(np.isfinite(g).all() for g in got[1:]), tag
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):                # exact zeros in the padding and from a row without a path
        assert not got[1][b, n:].any() and not got[2][b, len(lab) + 1:].any(), (tag, b)
        assert b not in inf or (got[0][b] == math.inf and not got[1][b].any() and not got[2][b].any()), (tag, b)
    rows = [b for b in range(len(c["lens"])) if b not in inf]
    for nm, g, a, f in zip(NAMES, got, r64, r32):
        parts = [(g, a, f)] if nm == "d_out" else [(g[b], a[b], f[b]) for b in rows]
        for i, (x, ref, x32) in enumerate(parts):
            e, e32 = _rel(x, ref), _rel(x32, ref)
            print("%s %s[%d]: err %.2e, torch f32 err %.2e, ratio %.3f" % (tag, nm, i, e, e32, e / max(e32, 1e-300)))
            assert e <= max(K.FACTOR * e32, K.FLOOR), (tag, nm, i, e, e32)
    return got


# J, V, durations, blank (first / last / mid-block), sigma; V + D = 9, 35 and 259 are no multiple of 4
RAGGED = [(1, 5, [0, 1, 2, 3], 0, 0.0), (5, 30, D5, 29, 0.05), (67, 32, [0, 1, 2, 3], 16, 0.0), (67, 254, D5, 100, 0.0), (64, 600, D5, 300, 0.0),
          (260, 70, D5, 3, 0.0), (515, 40, D5, 39, 0.05), (900, 140, D5, 17, 0.0)]


@pytest.mark.parametrize("J,V,durs,blank,sigma", RAGGED)
def test_ragged_batch_matches_float64(gpu, J, V, durs, blank, sigma):
    c = TF.ragged(J, V, durs, blank, sigma)
    assert [len(r) for r in c["labels"]] == [3, 0, 5] and c["lens"][2] == 1 and (blank == V - 1 or c["labels"][2][4] == V - 1)
    assert 3 * 7 * 6 - 96 < 32 and c["lens"][2] * 6 + 2 * 42 <= 96           # the last tile: cells of row 2 with t >= 1 only
    _check(gpu, "ragged J %d V %d D %d" % (J, V, len(durs)), c)


@pytest.mark.parametrize("durs,inf", [([1, 2], [2]), ([0, 2], [0, 2])])
def test_rows_without_a_path_beside_rows_with_one(gpu, durs, inf):
    """{1, 2}: no zero duration, so five labels do not fit one frame; {0, 2}: the odd T_b = 7 and 1 cannot be reached, T_b = 4 can"""
    got = _check(gpu, "durations %s" % durs, TF.ragged(5, 5, durs, 2), inf=inf)
    assert np.isfinite(got[3]).all() and np.abs(got[3]).sum() > 0


@pytest.mark.parametrize("kind", ["identity", "tanh", "relu"])
@pytest.mark.parametrize("J,V", [(5, 30), (67, 254)])
def test_activations(gpu, J, V, kind):
    _check(gpu, "J %d V %d %s" % (J, V, kind), TF.ragged(J, V, D5, 1, seed=2), kind)


@pytest.mark.parametrize("T,U", [(4, 4), (4, 7), (3, 10), (3, 300)])
def test_cell_counts_around_one_tile_and_a_wide_lattice(gpu, T, U):
    assert T * (U + 1) in (20, 32, 33) or U + 1 > K.CTC_THREADS
    _check(gpu, "T %d U %d" % (T, U), TF.single(T, U, 5, 4, [0, 1, 2], 1, 40 + U))


@pytest.mark.parametrize("col", [297, 2, 302])
def test_running_log_sum_exp(gpu, col):
    """a +80 bias on a token of the last block (the running sum is rescaled by e^-80 there), of the first block (every later block adds
    terms of e^-80), and on one duration, which the paths then take: the blank's -F_blank W is the large early term of every d z sum"""
    J, V = 8, 300
    c = TF.ragged(J, V, D5, 5, seed=3)
    c["out"][J * (V + 5) + col] += 80.0
    _check(gpu, "+80 on column %d" % col, c)


def test_emission_underflow_on_both_heads(gpu):
    """the construction of test_gpu_rnnt_fused.py on both heads: token 7 and the duration 8, which no move of 6 frames can take, hold the
    mass; every needed token lies 200 below, every needed duration 150"""
    T, U, J, V = 6, 4, 4, 8
    c = TF.single(T, U, J, V, [0, 1, 8], 0, 9)
    c.update(labels=[[1, 2, 2, 4]], out=np.concatenate([c["out"][:J * 11] * 0.2, np.full(8, -200.0), np.full(3, -150.0)]).astype(np.float32))
    c["out"][J * 11 + 7] = c["out"][J * 11 + 10] = 0.0
    got = _check(gpu, "underflow", c)
    assert 340.0 * T < got[0][0] < 360.0 * (T + U + 1) and np.exp(-np.float32(got[0][0])) == 0.0


def _bits_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("J,V,durs", [(67, 254, D5), (5, 5, [0, 2])])
def test_bits(gpu, J, V, durs):
    """the same bits on every call, loss-only, with the rows in another order (a row without a path among them), and in the host form"""
    c = TF.ragged(J, V, durs, 2)
    got = _run(gpu, c)
    assert _bits_equal(got, _run(gpu, c))
    only = _run(gpu, c, want_grad=False)
    assert only[1] is None and _bits_equal(only[:1], got[:1])
    perm, (enc, pred) = [2, 0, 1], K.with_nan_padding(c)
    cp = dict(c, labels=[c["labels"][i] for i in perm], lens=[c["lens"][i] for i in perm])
    assert _bits_equal([t[perm] for t in got[:3]], _run(gpu, cp, arrays=(enc[perm], pred[perm]))[:3])
    host = NL.rnnt_tdt_fused_loss(c["enc"], c["pred"], c["out"], c["labels"], c["durs"], input_lengths=c["lens"], blank=2)
    dev = _run(gpu, c, arrays=(c["enc"], c["pred"]))
    assert all(np.array_equal(h.view(np.int32), g.numpy().view(np.int32)) for h, g in zip(host, dev))
