"""The RNN-Transducer loss, its gradient with respect to the scores, and the joiner (csrc/hip/rnnt.hip) against tests/rnnt_reference.py.

Reference: the float64 numpy log-space recursion (itself pinned to enumeration and to autograd by tests/test_rnnt_host.py).

Tolerance, measured and not fixed in advance: the same quantities come out of a float32 torch log-space restatement on the CPU
(rnnt_reference.torch_rnnt); per row the device's error against float64 is at most FACTOR = 4 x that float32 error -- the loss relative
to |loss|, the gradient relative to the row's largest |gradient| -- or FLOOR where the float32 error is smaller.  FLOOR = 16 * 2^-24, the
floor of tests/test_gpu_ctc.py: the float32 restatement can be exact (on a lattice with one dominant path autograd's weights are exactly 1),
while the device rounds once per lattice step and once per factor of alpha beta / P, the exponential's argument, the exponential (1 ulp),
the division by P and the result -- some 2 (T_b + U_b) roundings of half an ulp that add up like a random walk, a few ulps at the sizes here.

Which test reaches which branch of rnnt.hip (every instantiation and every V- / U-dependent branch):
  rnnt_emit_kernel / rnnt_grad_kernel <VEC = false> (V % 4 != 0: 4-byte loads, rows off the 16-byte grid, zero-fill with head and tail
    stores): ragged V = 2, 5, 257 (more than one pass of the wavefront and an odd tail), the wide lattices (V = 3)
  ... <VEC = true> (16-byte loads and stores): ragged V = 64 (a quarter of the lanes busy) and V = 260 (more than one pass of quads),
    emission underflow (V = 8), end to end (V = 8)
  rnnt_lattice_kernel<1> (U1 <= 256): ragged, T = 300 x U = 2, T = 400 x U = 200, underflow
  rnnt_lattice_kernel<2> (256 < U1 <= 512, a lane owns two cells of a diagonal): T = 5 x U = 300
  rnnt_lattice_kernel<0> (U1 > 512, emissions fetched inside the step): T = 3 x U = 600; with the dynamic-LDS opt-in (2 U1 16 bytes
    > 48 KiB): T = 2 x U = 1600
  loss only (one direction, nothing stored): test_structure
  rnnt_joint_kernel<4> (J % 4 == 0) / <1>: J = 64 / J = 5
  rnnt_joint_reduce_kernel: whole groups of RNNT_JOINT_UNROLL = 4 terms only (U1 = 4), a remainder only (T = 3), groups and a
    remainder (T = 9 and U1 = 6)"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import rnnt_cases as K
import rnnt_reference as R
from nntoolkitcore_amd import capi, layers as NL

pytestmark = pytest.mark.gpu

RNNT_JOINT_UNROLL = 4                                # of rnnt.hip, mirrored; the constants that pick a lattice kernel: rnnt_cases.py


RAGGED = [(2, 0), (2, 1), (5, 0), (5, 4), (5, 2), (64, 0), (64, 63), (64, 17), (257, 0), (257, 256), (257, 100), (260, 7)]


def _case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("ragged"):                    # batch 3, T = 7 with lengths (7, 4, 1), max_label_len 5 with label lengths (3, 0, 5)
        return K.ragged(*(int(v) for v in name.split("_")[1:]))
    if name == "U300":                               # a second, short row inside the wide lattice
        return dict(x=rng.uniform(-2, 2, (2, 5, 301, 3)).astype(np.float32), labels=[K.labels(rng, 300, 3, 1), [0, 2]], lens=[5, 3], blank=1)
    if name == "T300":
        return dict(x=rng.uniform(-2, 2, (1, 300, 3, 3)).astype(np.float32), labels=[[1, 1]], lens=[300], blank=0)
    if name == "flat_T400_U200":                     # binomial(599, 200) = 1e164 paths of equal mass
        return dict(x=np.zeros((1, 400, 201, 3), np.float32), labels=[K.labels(rng, 200, 3, 2)], lens=[400], blank=2)
    if name == "U600":
        return dict(x=rng.uniform(-2, 2, (1, 3, 601, 3)).astype(np.float32), labels=[K.labels(rng, 600, 3, 0)], lens=[3], blank=0)
    if name == "U1600":
        return dict(x=rng.uniform(-2, 2, (2, 2, 1601, 3)).astype(np.float32), labels=[K.labels(rng, 1600, 3, 0), [1]], lens=[2, 1], blank=0)
    if name == "underflow":
        # V = 8: blank 0, labels 1..4, class 7 takes the mass everywhere.  Off the path every needed score lies 200 below it; on the path
        # the needed score equals it, except in two cells where it lies 120 below: one likely path, e^-240 of the mass on it
        T, U, V = 6, 4, 8
        lab = [1, 2, 2, 4]
        x = np.full((1, T, U + 1, V), -200.0, np.float32) + rng.uniform(-0.5, 0.5, (1, T, U + 1, V)).astype(np.float32)
        x[..., 7] = 0.0
        moves = "blbbllbblb"                          # b: a blank (t + 1), l: the next label (u + 1); ends with the blank out of (T-1, U)
        t = u = 0
        for i, m in enumerate(moves):
            x[0, t, u, 0 if m == "b" else lab[u]] = -120.0 if i in (3, 6) else 0.0
            t, u = (t + 1, u) if m == "b" else (t, u + 1)
        assert (t, u) == (T, U)
        return dict(x=x, labels=[lab], lens=[T], blank=0)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = _case(name)
    l64, g64 = R.rnnt_loss_and_grad(c["x"], c["labels"], c["lens"], c["blank"])
    l32, g32 = R.torch_rnnt(c["x"], c["labels"], c["lens"], c["blank"], torch.float32)
    for a in (l64, g64, l32, g32):
        a.setflags(write=False)
    return l64, g64, l32, g32


def _run(gpu, x, labels, lens, blank, want_grad=True):
    """outputs prefilled with NaN: every element has to be written"""
    d = torch.from_numpy(x).to(gpu)
    loss = torch.full((x.shape[0],), float("nan"), device=gpu)
    g = torch.full_like(d, float("nan")) if want_grad else None
    NL.rnnt_loss_device(d, labels, input_lengths=lens, blank=blank, want_grad=want_grad, loss=loss, dlogits=g)
    torch.cuda.synchronize()
    return loss.cpu(), (g.cpu() if want_grad else None)


def _assert_close(tag, loss, grad, ref):
    l64, g64, l32, g32 = ref
    loss, grad = loss.double().numpy(), grad.double().numpy()
    for b in range(loss.shape[0]):
        assert np.isfinite(l64[b]) and l64[b] > 0
        e, e32 = abs(loss[b] - l64[b]) / l64[b], abs(l32[b] - l64[b]) / l64[b]
        print("%s row %d loss %.9g: err %.2e, torch f32 err %.2e, ratio %.3f" % (tag, b, l64[b], e, e32, e / max(e32, 1e-300)))
        gs = np.abs(g64[b]).max()
        ge, ge32 = np.abs(grad[b] - g64[b]).max() / gs, np.abs(g32[b] - g64[b]).max() / gs
        print("%s row %d grad (max |g| %.3g): err %.2e, torch f32 err %.2e, ratio %.3f" % (tag, b, gs, ge, ge32, ge / max(ge32, 1e-300)))
        assert e <= max(K.FACTOR * e32, K.FLOOR), (tag, b, e, e32)
        assert ge <= max(K.FACTOR * ge32, K.FLOOR), (tag, b, ge, ge32)


def _check(gpu, name):
    c = _case(name)
    loss, grad = _run(gpu, K.with_nan_padding(c), c["labels"], c["lens"], c["blank"])
    assert torch.isfinite(loss).all() and not torch.isnan(grad).any()
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):
        assert not grad[b, n:].any() and not grad[b, :, len(lab) + 1:].any(), (name, b)      # exact zeros in the padding
    _assert_close(name, loss, grad, _reference(name))
    return c, loss, grad


@pytest.mark.parametrize("V,blank", RAGGED)
def test_ragged_batch_matches_float64(gpu, V, blank):
    c, _, _ = _check(gpu, "ragged_%d_%d" % (V, blank))
    assert c["labels"][0][0] == c["labels"][0][1] and [len(r) for r in c["labels"]] == [3, 0, 5] and K.lattice_path(5)[0] == 1


@pytest.mark.parametrize("name,nj,opt_in", [("U300", 2, False), ("T300", 1, False), ("flat_T400_U200", 1, False), ("U600", 0, False),
                                            ("U1600", 0, True)])
def test_lattices_wider_than_one_pass_of_lanes(gpu, name, nj, opt_in):
    c = _case(name)
    got_nj, lds = K.lattice_path(c["x"].shape[2] - 1)
    assert (got_nj, lds > K.LDS_OPT_IN) == (nj, opt_in), (name, got_nj, lds)
    _, loss, _ = _check(gpu, name)
    if name == "flat_T400_U200":                     # ln 3^600 - ln binomial(599, 200): the path count alone is past the f32 range
        assert 280.0 < float(loss[0]) < 283.0


def test_emission_underflow(gpu):
    c = _case("underflow")
    lp = R.log_softmax(c["x"][0])
    assert 119.0 < -lp[2, 1, 0] < 122.0 and 119.0 < -lp[3, 3, 0] < 122.0     # the two cells of the path with lse - x about 120
    l64 = _reference("underflow")[0]
    assert 240.0 < l64[0] < 255.0 and np.exp(-np.float32(l64[0])) == 0.0      # P itself is below the f32 range
    _, loss, _ = _check(gpu, "underflow")
    assert np.isfinite(float(loss[0]))


@pytest.mark.parametrize("name", ["ragged_64_17", "ragged_5_2", "U300"])
def test_structure(gpu, name):
    """sums over V, padding, determinism, loss-only bits, row independence -- all with the outputs prefilled with NaN (_run) and NaN in
    every padding cell of the scores"""
    c = _case(name)
    x = K.with_nan_padding(c)
    B, T, U1, V = x.shape
    loss, grad = _run(gpu, x, c["labels"], c["lens"], c["blank"])
    g64 = _reference(name)[1]
    # the gradient of a log-softmax's input sums to zero over V.  Each of the V stored entries is rounded once (<= 2^-24 max |g| each);
    # the cell's three scalars -- occupancy and the two flows, each <= 1 -- are computed apart, a handful of roundings each, and the
    # probabilities sum to 1 only within the rounding of lse and of the exponentials: 32 * 2^-24 absolute for those
    for b in range(B):
        gmax = np.abs(g64[b]).max()
        res = np.abs(grad[b].double().numpy().sum(-1)).max()
        bound = V * 2.0 ** -24 * gmax + 32 * 2.0 ** -24
        print("%s row %d: largest |sum over V| %.2e (bound %.2e, max |g| %.3g)" % (name, b, res, bound, gmax))
        assert res <= bound, (name, b, res, bound)
        n, u = c["lens"][b], len(c["labels"][b])
        assert not grad[b, n:].any() and not grad[b, :, u + 1:].any()
        assert grad[b, :n, :u + 1].abs().sum() > 0
    loss2, grad2 = _run(gpu, x, c["labels"], c["lens"], c["blank"])
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    loss3, none = _run(gpu, x, c["labels"], c["lens"], c["blank"], want_grad=False)
    assert none is None and torch.equal(loss3, loss)
    for b in range(B):
        l1, g1 = _run(gpu, x[b:b + 1], [c["labels"][b]], [c["lens"][b]], c["blank"])
        assert torch.equal(l1, loss[b:b + 1]) and torch.equal(g1, grad[b:b + 1]), (name, b)
        n, u = c["lens"][b], len(c["labels"][b])    # ... and without the T / max_label_len padding
        l0, g0 = _run(gpu, np.ascontiguousarray(x[b:b + 1, :n, :u + 1]), [c["labels"][b]], [n], c["blank"])
        assert torch.equal(l0, loss[b:b + 1]) and torch.equal(g0, grad[b:b + 1, :n, :u + 1]), (name, b)


def test_host_form_equals_the_device_form(gpu):
    c = _case("ragged_5_2")
    loss, grad = _run(gpu, c["x"], c["labels"], c["lens"], c["blank"])
    hl, hg = NL.rnnt_loss(c["x"], c["labels"], input_lengths=c["lens"], blank=c["blank"])
    assert np.array_equal(hl, loss.numpy()) and np.array_equal(hg, grad.numpy())
    hl2, none = NL.rnnt_loss(c["x"], c["labels"], input_lengths=c["lens"], blank=c["blank"], want_grad=False)
    assert none is None and np.array_equal(hl2, hl)


def test_argument_errors_write_nothing(gpu):
    L = capi.load()
    B, T, ML, V = 2, 6, 3, 5
    x = torch.zeros((B, T, ML + 1, V), device=gpu)
    ws = torch.empty(L.nntk_rnnt_workspace_floats(B, T, ML, 1), device=gpu)
    dp = lambda t: C.c_void_p(t.data_ptr())
    ip = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(capi.ip)
    good = dict(il=[6, 4], lab=[[1, 2, 0], [3, 0, 0]], ll=[2, 1], blank=4)
    for change in (dict(il=[7, 4]), dict(il=[6, 0]), dict(ll=[4, 1]), dict(lab=[[1, 4, 0], [3, 0, 0]]), dict(lab=[[1, 5, 0], [3, 0, 0]]),
                   dict(blank=5)):
        a = dict(good, **change)
        loss, g = torch.full((B,), 7.0, device=gpu), torch.full_like(x, 7.0)
        rc = L.nntk_rnnt_loss_device(dp(x), B, T, V, ip(a["il"]), ip(a["lab"]), ip(a["ll"]), ML, a["blank"], dp(loss), dp(g), dp(ws))
        torch.cuda.synchronize()
        assert rc == -1 and capi.last_error() != "" and (loss == 7.0).all() and (g == 7.0).all(), change


# ---- the joiner ----

KINDS = ("identity", "tanh", "relu")


def _joint_inputs(B, T, U1, J):
    rng = np.random.default_rng(B * 1000 + T * 100 + U1 * 10 + J)
    u = lambda *s: rng.uniform(-2, 2, s).astype(np.float32)
    return u(B, T, J), u(B, U1, J), u(B, T, U1, J)


def _torch_act(kind, z):
    return torch.tanh(z) if kind == "tanh" else torch.relu(z) if kind == "relu" else z


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,T,U1,J", [(2, 3, 4, 5), (2, 3, 4, 64), (2, 9, 6, 5), (1, 9, 6, 8)])
def test_joiner_forward_and_backward(gpu, kind, B, T, U1, J):
    assert T % RNNT_JOINT_UNROLL and (U1, T) in ((4, 3), (6, 9))            # the docstring's reduction passes
    enc, pred, dout = _joint_inputs(B, T, U1, J)
    e, p, d = (torch.from_numpy(a).to(gpu) for a in (enc, pred, dout))
    out = torch.full((B, T, U1, J), float("nan"), device=gpu)
    NL.rnnt_joint_device(e, p, kind, out=out)
    t32 = _torch_act(kind, torch.from_numpy(enc)[:, :, None, :] + torch.from_numpy(pred)[:, None, :, :])
    o = out.cpu()
    if kind != "tanh":
        assert torch.equal(o, t32)
    else:
        o64 = R.joint(enc, pred, kind)
        err, e32 = np.abs(o.double().numpy() - o64).max(), np.abs(t32.double().numpy() - o64).max()
        print("joiner tanh J %d: err %.2e, torch f32 err %.2e" % (J, err, e32))
        assert err <= max(K.FACTOR * e32, K.FLOOR), (err, e32)
    denc = torch.full((B, T, J), float("nan"), device=gpu)
    dpred = torch.full((B, U1, J), float("nan"), device=gpu)
    NL.rnnt_joint_backward_device(out, d, kind, denc=denc, dpred=dpred)
    denc2, dpred2 = NL.rnnt_joint_backward_device(out, d, kind)
    torch.cuda.synchronize()
    assert torch.equal(denc, denc2) and torch.equal(dpred, dpred2)
    # both references start from the device's own forward output, as the call does
    r_enc, r_pred = R.joint_backward(o.double().numpy(), dout, kind)
    dd = torch.from_numpy(dout) * (1 - o * o if kind == "tanh" else (o > 0).float() if kind == "relu" else torch.ones_like(o))
    for nm, got, ref, f32 in (("d_enc", denc, r_enc, dd.sum(2)), ("d_pred", dpred, r_pred, dd.sum(1))):
        sc = np.abs(ref).max()
        err, e32 = np.abs(got.cpu().double().numpy() - ref).max() / sc, np.abs(f32.double().numpy() - ref).max() / sc
        print("joiner %s %s J %d: err %.2e, torch f32 err %.2e" % (kind, nm, J, err, e32))
        assert err <= max(K.FACTOR * e32, K.FLOOR), (nm, err, e32)


def test_end_to_end_one_training_step(gpu):
    """encoder (a random tensor) and predictor outputs -> joiner -> the library's Dense on batch T U1 rows -> loss -> Dense gradient
    -> joiner backward -> one SGD step of the device optimizer on the Dense block and on both joiner inputs: the loss on the same
    batch goes down"""
    L = capi.load()
    rng = np.random.default_rng(12)
    B, T, U1, J, V, blank = 2, 5, 4, 16, 8, 0
    labels, lens = [[3, 3, 5], [1, 7]], [5, 4]
    rows = B * T * U1
    dp = lambda t: C.c_void_p(t.data_ptr())
    u = lambda sc, *s: torch.from_numpy(rng.uniform(-sc, sc, s).astype(np.float32)).to(gpu)
    enc, pred, w = u(1.0, B, T, J), u(1.0, B, U1, J), u(0.5, J * V + V)
    dense = L.DenseCreateForTraining(L.DenseConfigCreate(J, V, None), capi.ConvTrainingConfig(rows))
    assert dense, capi.last_error()
    gw, denc, dpred = torch.zeros_like(w), torch.zeros_like(enc), torch.zeros_like(pred)
    opt = NL.Optimizer("sgd", [(w, gw), (enc, denc), (pred, dpred)], learning_rate=0.05, zero_gradients=1)
    losses = []
    for step in range(2):
        assert L.DenseLoadWeightsDevice(dense, dp(w)) == 0, capi.last_error()
        joint = NL.rnnt_joint_device(enc, pred, "tanh")
        logits = torch.empty((B, T, U1, V), device=gpu)
        assert L.DenseApplyTrainingBatchDevice(dense, dp(joint), dp(logits)) == 0, capi.last_error()
        loss, dlogits = NL.rnnt_loss_device(logits, labels, input_lengths=lens, blank=blank)
        losses.append(float(loss.sum()))
        if step == 0:
            l64, _ = R.rnnt_loss_and_grad(logits.cpu().numpy(), labels, lens, blank)
            np.testing.assert_allclose(loss.cpu().double().numpy(), l64, rtol=1e-5)
            djoint = torch.empty_like(joint)
            assert L.DenseCalculateGradientDevice(dense, dp(gw), dp(djoint), dp(dlogits)) == 0, capi.last_error()
            NL.rnnt_joint_backward_device(joint, djoint, "tanh", denc=denc, dpred=dpred)
            assert float(gw.abs().sum()) > 0 and float(denc.abs().sum()) > 0 and float(dpred.abs().sum()) > 0
            opt.step()
    torch.cuda.synchronize()
    print("summed transducer loss: %.5f before the step, %.5f after" % (losses[0], losses[1]))
    assert np.isfinite(losses).all() and losses[1] < losses[0]
    opt.destroy(); L.DenseDestroy(dense)
