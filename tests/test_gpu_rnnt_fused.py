"""The fused transducer training loss (csrc/hip/rnnt_fused.hip: joiner + vocabulary projection + loss, the scores never stored) against
tests/rnnt_fused_reference.py.

Reference: float64 numpy (joiner, matmul, rnnt_reference.rnnt_loss_and_grad, the chain rule by hand; pinned to autograd by
tests/test_rnnt_fused_host.py).  Tolerance, measured and not fixed in advance, as in tests/test_gpu_rnnt.py: the same quantities come out
of a float32 torch restatement on the CPU (torch_fused); per output the device's error against float64, relative to the output's largest
|value| -- per row for the loss, d_enc and d_pred, over the whole block for d_out -- is at most FACTOR = 4 x that float32 error, or
FLOOR = 16 * 2^-24 where the float32 error is smaller.  Every measured ratio is printed.

Which test reaches which branch of rnnt_fused.hip (cells come in tiles of 32; V in blocks of 32 columns, 8 blocks a pass of the forward's
waves; J in pairs, groups of 8 and blocks of 32):
  ft_logits: J = 1 (the odd tail alone), 5 (pairs + tail), 64 / 67 (groups of 8, with and without pairs and tail)
  forward, running log-sum-exp: V = 2, 5 (one partial block), 33 (a second block of one column), 257 (a second pass of the waves, one
    column), 600 (a third pass); blank first / last / mid-block; a label in the last, partial block (every ragged case with blank !=
    V - 1 puts label V - 1 into row 2); the maximum in the last / first block: test_running_log_sum_exp; a label 200 below: underflow
  tiles: 126 cells (three full tiles and a partial one, live and dead cells mixed, NaN in the dead ones), 20 / 32 / 33 cells:
    test_cell_counts_around_one_tile; an all-dead tile (skipped, d z zero-filled): ragged row 1 (u > 0) and row 2 (t > 0)
  rnnt_fused_dz_kernel: gw = 8 (J <= 896) with one group (V <= 256) and more (V = 257, 600); gw = 4: J = 900, V = 140 (two groups);
    the blocks of J a wave owns: one (J <= 256), a second (J = 260), up to four (J = 900)
  rnnt_fused_dw_kernel<1> (J <= 256, 128 columns a workgroup): V <= 128 and V = 257, 600 (more workgroups, a partial last one);
    <2> (J = 260, 64 columns): V = 70; <4> (J = 515 / 900, 32 columns): V = 40 / 140
  rnnt_lattice_kernel<2> / <0> through the new emission writer: U1 = 301 / 601
  the three activations: ragged (identity and relu on three shapes, tanh on all)"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import rnnt_cases as K
import rnnt_fused_reference as FR
import rnnt_reference as R
from nntoolkitcore_amd import capi, layers as NL

pytestmark = pytest.mark.gpu

NAMES = ("loss", "d_enc", "d_pred", "d_out")


def _run(gpu, enc, pred, out, labels, lens, blank, kind, want_grad=True):
    """outputs prefilled with NaN: every element has to be written"""
    e, p, o = (torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (enc, pred, out))
    nan = lambda t: torch.full_like(t, float("nan"))
    loss = torch.full((enc.shape[0],), float("nan"), device=gpu)
    g = (nan(e), nan(p), nan(o)) if want_grad else (None, None, None)
    NL.rnnt_fused_loss_device(e, p, o, labels, input_lengths=lens, blank=blank, activation=kind, want_grad=want_grad, loss=loss,
                              denc=g[0], dpred=g[1], dout=g[2])
    torch.cuda.synchronize()
    return (loss.cpu(),) + tuple(t.cpu() if want_grad else None for t in g)


def _references(c, kind):
    r64 = FR.fused_loss_and_grads(c["enc"], c["pred"], c["out"], c["labels"], c["lens"], c["blank"], kind)
    r32 = FR.torch_fused(c["enc"], c["pred"], c["out"], c["labels"], c["lens"], c["blank"], kind, torch.float32)
    return r64, r32


def _errors(got, r64, per_row):
    """the largest error relative to the largest |value|: per row, or over the whole block"""
    got, r64 = np.asarray(got, np.float64), np.asarray(r64, np.float64)
    if not per_row:
        return [np.abs(got - r64).max() / np.abs(r64).max()]
    out = []
    for b in range(r64.shape[0]):
        sc = np.abs(r64[b]).max()
        out.append(np.abs(got[b] - r64[b]).max() / sc if sc > 0 else np.abs(got[b]).max())
    return out


def _assert_close(tag, got, refs):
    r64, r32 = refs
    assert np.isfinite(r64[0]).all() and (r64[0] > 0).all()
    for nm, g, a, b in zip(NAMES, got, r64, r32):
        g = g.double().numpy()
        assert np.isfinite(g).all(), (tag, nm)
        for i, (e, e32) in enumerate(zip(_errors(g, a, nm != "d_out"), _errors(b, a, nm != "d_out"))):
            print("%s %s[%d]: err %.2e, torch f32 err %.2e, ratio %.3f" % (tag, nm, i, e, e32, e / max(e32, 1e-300)))
            assert e <= max(K.FACTOR * e32, K.FLOOR), (tag, nm, i, e, e32)


def _check(gpu, tag, c, kind):
    enc, pred = K.with_nan_padding(c)
    got = _run(gpu, enc, pred, c["out"], c["labels"], c["lens"], c["blank"], kind)
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):                # exact zeros in the padding
        assert not got[1][b, n:].any() and not got[2][b, len(lab) + 1:].any(), (tag, b)
    _assert_close(tag, got, _references(c, kind))
    return got


RAGGED = [(1, 2, 0), (5, 5, 4), (5, 5, 2), (64, 33, 32), (64, 33, 0), (67, 257, 100), (67, 257, 256), (64, 600, 300), (5, 257, 0),
          (260, 70, 3), (515, 40, 39), (900, 140, 17)]
OTHER_KINDS = [(1, 2, 0), (67, 257, 100), (260, 70, 3)]


@pytest.mark.parametrize("J,V,blank", RAGGED)
def test_ragged_batch_matches_float64(gpu, J, V, blank):
    c = K.fused_ragged(J, V, blank)
    assert [len(r) for r in c["labels"]] == [3, 0, 5] and (blank == V - 1 or c["labels"][2][4] == V - 1)
    _check(gpu, "ragged J %d V %d blank %d tanh" % (J, V, blank), c, "tanh")


@pytest.mark.parametrize("kind", ["identity", "relu"])
@pytest.mark.parametrize("J,V,blank", OTHER_KINDS)
def test_ragged_batch_other_activations(gpu, J, V, blank, kind):
    _check(gpu, "ragged J %d V %d blank %d %s" % (J, V, blank, kind), K.fused_ragged(J, V, blank), kind)


@pytest.mark.parametrize("T,U", [(4, 4), (4, 7), (3, 10)])
def test_cell_counts_around_one_tile(gpu, T, U):
    assert T * (U + 1) in (20, 32, 33)
    _check(gpu, "cells %d" % (T * (U + 1)), K.fused_single(T, U, 5, 5, 1, 40 + U), "tanh")


@pytest.mark.parametrize("where", ["last", "first"])
def test_running_log_sum_exp(gpu, where):
    """the bias puts every cell's maximum into the last (first) block of V, 80 above everything before (after) it: the running sum
    is rescaled by e^-80 there (or every later block adds terms of e^-80)"""
    J, V = 8, 300
    c = K.fused_ragged(J, V, 5, seed=3)
    bias = c["out"][J * V:]
    if where == "last":
        bias[V - 3] += 80.0
    else:
        bias[2] += 80.0
    assert V > 256 + 32
    _check(gpu, "lse max in the %s block" % where, c, "tanh")


def test_emission_underflow(gpu):
    """the `underflow` construction of test_gpu_rnnt.py expressed through b: class 7 takes the mass everywhere, every needed class lies
    200 below it"""
    T, U, J, V = 6, 4, 4, 8
    rng = np.random.default_rng(9)
    c = dict(enc=rng.uniform(-0.5, 0.5, (1, T, J)).astype(np.float32), pred=rng.uniform(-0.5, 0.5, (1, U + 1, J)).astype(np.float32),
             out=np.concatenate([rng.uniform(-0.2, 0.2, J * V), np.full(V, -200.0)]).astype(np.float32), labels=[[1, 2, 2, 4]], lens=[T],
             blank=0)
    c["out"][J * V + 7] = 0.0
    r64 = FR.fused_loss_and_grads(c["enc"], c["pred"], c["out"], c["labels"], c["lens"], 0, "tanh")
    assert 190.0 * (T + U) < r64[0][0] < 210.0 * (T + U) and np.exp(-np.float32(r64[0][0])) == 0.0
    got = _check(gpu, "underflow", c, "tanh")
    assert np.isfinite(float(got[0][0]))


@pytest.mark.parametrize("U,nj", [(300, 2), (600, 0)])
def test_wide_lattices_through_the_new_emission_writer(gpu, U, nj):
    assert (1 if U + 1 <= 256 else 2 if U + 1 <= 512 else 0) == nj
    _check(gpu, "U %d" % U, K.fused_single(3, U, 4, 3, 0, U), "tanh")


def _bits_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("J,V,blank", [(67, 257, 100), (5, 5, 2)])
def test_structure(gpu, J, V, blank):
    """every element written (the outputs are prefilled with NaN), d_out finite with NaN padding, determinism, loss-only bits, row
    independence under permutation and further padding"""
    c = K.fused_ragged(J, V, blank)
    enc, pred = K.with_nan_padding(c)
    args = (c["out"], c["labels"], c["lens"], c["blank"], "tanh")
    got = _run(gpu, enc, pred, *args)
    assert all(torch.isfinite(t).all() for t in got)
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):
        assert not got[1][b, n:].any() and not got[2][b, len(lab) + 1:].any()
        assert got[1][b, :n].abs().sum() > 0 and got[2][b, :len(lab) + 1].abs().sum() > 0
    assert _bits_equal(got, _run(gpu, enc, pred, *args))
    only = _run(gpu, enc, pred, *args, want_grad=False)
    assert only[1] is None and _bits_equal(only[:1], got[:1])
    # the rows in another order
    perm = [2, 0, 1]
    gp = _run(gpu, enc[perm], pred[perm], c["out"], [c["labels"][i] for i in perm], [c["lens"][i] for i in perm], c["blank"], "tanh")
    assert _bits_equal([t[perm] for t in got[:3]], gp[:3])
    # T and max_label_len padded further (NaN), and a row alone without any padding
    B, T, U1 = 3, 7, 6
    e2, p2 = np.full((B, T + 3, J), np.nan, np.float32), np.full((B, U1 + 2, J), np.nan, np.float32)
    e2[:, :T], p2[:, :U1] = enc, pred
    g2 = _run(gpu, e2, p2, *args)
    assert _bits_equal([got[0], got[1], got[2]], [g2[0], g2[1][:, :T], g2[2][:, :U1]])
    assert not g2[1][:, T:].any() and not g2[2][:, U1:].any()
    for b in range(B):
        n, u = c["lens"][b], len(c["labels"][b])
        g1 = _run(gpu, enc[b:b + 1, :n], pred[b:b + 1, :u + 1], c["out"], [c["labels"][b]], [n], c["blank"], "tanh")
        assert _bits_equal([got[0][b:b + 1], got[1][b:b + 1, :n], got[2][b:b + 1, :u + 1]], g1[:3]), b


def test_host_form_equals_the_device_form(gpu):
    c = K.fused_ragged(5, 5, 2)
    got = _run(gpu, c["enc"], c["pred"], c["out"], c["labels"], c["lens"], c["blank"], "tanh")
    host = NL.rnnt_fused_loss(c["enc"], c["pred"], c["out"], c["labels"], input_lengths=c["lens"], blank=c["blank"], activation="tanh")
    assert all(np.array_equal(h.view(np.int32), g.numpy().view(np.int32)) for h, g in zip(host, got))
    h2 = NL.rnnt_fused_loss(c["enc"], c["pred"], c["out"], c["labels"], input_lengths=c["lens"], blank=c["blank"], activation="tanh",
                            want_grad=False)
    assert h2[1] is None and np.array_equal(h2[0], host[0])


def test_argument_errors_write_nothing(gpu):
    L = capi.load()
    B, T, ML, J, V = 2, 6, 3, 8, 5
    z = lambda *s: torch.zeros(s, device=gpu)
    enc, pred, out = z(B, T, J), z(B, ML + 1, J), z(J * V + V)
    ws = torch.empty(L.nntk_rnnt_fused_workspace_floats(B, T, ML, J, V, 1), device=gpu)
    dp = lambda t: C.c_void_p(t.data_ptr())
    ip = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(capi.ip)
    good = dict(il=[6, 4], lab=[[1, 2, 0], [3, 0, 0]], ll=[2, 1], blank=4, act=1)
    for change in (dict(il=[7, 4]), dict(ll=[4, 1]), dict(lab=[[1, 4, 0], [3, 0, 0]]), dict(blank=5), dict(act=3)):
        a = dict(good, **change)
        outs = [torch.full((B,), 7.0, device=gpu), torch.full_like(enc, 7.0), torch.full_like(pred, 7.0), torch.full_like(out, 7.0)]
        rc = L.nntk_rnnt_fused_loss_device(dp(enc), dp(pred), dp(out), B, T, J, V, a["act"], ip(a["il"]), ip(a["lab"]), ip(a["ll"]), ML,
                                           a["blank"], *[dp(t) for t in outs], dp(ws))
        torch.cuda.synchronize()
        assert rc == -1 and capi.last_error() != "" and all((t == 7.0).all() for t in outs), change


def test_one_training_step(gpu):
    """the end-to-end step of test_gpu_rnnt.py in one call per step: one SGD step of the device optimizer on enc, pred and the Dense
    block; the summed loss on the same batch goes down"""
    rng = np.random.default_rng(12)
    B, T, U1, J, V, blank = 2, 5, 4, 16, 8, 0
    labels, lens = [[3, 3, 5], [1, 7]], [5, 4]
    u = lambda sc, *s: torch.from_numpy(rng.uniform(-sc, sc, s).astype(np.float32)).to(gpu)
    enc, pred, w = u(1.0, B, T, J), u(1.0, B, U1, J), u(0.5, J * V + V)
    gw, denc, dpred = torch.zeros_like(w), torch.zeros_like(enc), torch.zeros_like(pred)
    opt = NL.Optimizer("sgd", [(w, gw), (enc, denc), (pred, dpred)], learning_rate=0.05, zero_gradients=1)
    losses = []
    for step in range(2):
        if step == 0:
            loss, _, _, _ = NL.rnnt_fused_loss_device(enc, pred, w, labels, input_lengths=lens, blank=blank, activation="tanh", denc=denc,
                                                      dpred=dpred, dout=gw)
            assert float(gw.abs().sum()) > 0 and float(denc.abs().sum()) > 0 and float(dpred.abs().sum()) > 0
            losses.append(float(loss.sum()))
            opt.step()
        else:
            loss, _, _, _ = NL.rnnt_fused_loss_device(enc, pred, w, labels, input_lengths=lens, blank=blank, activation="tanh", want_grad=False)
            losses.append(float(loss.sum()))
    torch.cuda.synchronize()
    print("summed transducer loss: %.5f before the step, %.5f after" % (losses[0], losses[1]))
    assert np.isfinite(losses).all() and losses[1] < losses[0]
    opt.destroy()
