"""The host side of the RNN-Transducer calls (csrc/host/rnnt.c) -- the workspace size and every argument check, all made before anything
is allocated, uploaded or enqueued -- and the float64 reference the device tests rely on (tests/rnnt_reference.py), checked against
brute-force enumeration and against autograd.  No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import rnnt_cases as K
import rnnt_reference as R
from nntoolkitcore_amd import capi


def test_reference_equals_enumeration_of_every_alignment():
    rng = np.random.default_rng(1)
    V = 3
    for T, U, blank in itertools.product((1, 2, 3), (0, 1, 2), (0, 1, 2)):
        classes = [k for k in range(V) if k != blank]
        for lab in itertools.product(classes, repeat=U):
            x = rng.uniform(-3, 3, (1, T, U + 1, V))
            loss, _ = R.rnnt_loss_and_grad(x, [list(lab)], [T], blank)
            assert abs(loss[0] - R.brute_force_loss(x[0], list(lab), blank)) <= 1e-12 * max(1.0, abs(loss[0])), (T, U, blank, lab)


@pytest.mark.parametrize("V,blank", [(2, 0), (5, 4), (7, 3)])
def test_reference_gradient_equals_autograd_in_float64(V, blank):
    rng = np.random.default_rng(V)
    B, T, ML = 3, 7, 5
    classes = [k for k in range(V) if k != blank]
    labels = [[classes[i % len(classes)] for i in (0, 0, 1)], [], [classes[int(k)] for k in rng.integers(0, len(classes), 5)]]
    lens = [7, 4, 1]
    x = rng.uniform(-4, 4, (B, T, ML + 1, V))
    loss, grad = R.rnnt_loss_and_grad(x, labels, lens, blank)
    tl, tg = R.torch_rnnt(x, labels, lens, blank, torch.float64)
    np.testing.assert_allclose(loss, tl, rtol=1e-12)
    np.testing.assert_allclose(grad, tg, rtol=0, atol=1e-12)
    assert not grad[1, 4:].any() and not grad[1, :, 1:].any() and not grad[0, :, 4:].any()     # the padding
    assert np.abs(grad.sum(-1)).max() < 1e-12                                                  # d / d logits of a softmax: sums to 0 over V


def test_joiner_reference_equals_autograd():
    rng = np.random.default_rng(3)
    enc, pred, dout = rng.uniform(-2, 2, (2, 3, 5)), rng.uniform(-2, 2, (2, 4, 5)), rng.uniform(-1, 1, (2, 3, 4, 5))
    for kind, fn in (("identity", lambda z: z), ("tanh", torch.tanh), ("relu", torch.relu)):
        e, p = torch.from_numpy(enc).requires_grad_(True), torch.from_numpy(pred).requires_grad_(True)
        out = fn(e[:, :, None, :] + p[:, None, :, :])
        ge, gp = torch.autograd.grad((out * torch.from_numpy(dout)).sum(), (e, p))
        np.testing.assert_allclose(R.joint(enc, pred, kind), out.detach().numpy(), rtol=1e-14, atol=0)
        de, dp = R.joint_backward(R.joint(enc, pred, kind), dout, kind)
        np.testing.assert_allclose(de, ge.numpy(), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(dp, gp.numpy(), rtol=1e-12, atol=1e-14)


def test_workspace_size_is_nonzero_and_monotone():
    f = capi.load().nntk_rnnt_workspace_floats
    assert f(1, 1, 0, 0) > 0 and f(0, 0, 0, 0) > 0 and f(0, 0, 0, 1) > 0
    for B, T, L in ((1, 1, 1), (3, 50, 7), (16, 200, 40)):
        cells = B * T * (L + 1)
        for g in (0, 1):
            assert f(B, T, L, g) >= 4 * cells                                   # two emissions per cell, a mantissa and an exponent each
            assert f(B + 1, T, L, g) > f(B, T, L, g) and f(B, T + 1, L, g) > f(B, T, L, g) and f(B, T, L + 1, g) > f(B, T, L, g)
        assert f(B, T, L, 1) >= f(B, T, L, 0) + 6 * cells                       # lse as a double, alpha, beta
        assert f(B, T, L, 0) < f(B, T, L, 1)
    assert f(64, 1000, 4000, 1) > 2 ** 31                                       # no 32-bit arithmetic inside


GOOD, _ints = K.GOOD, K.ints
BAD = K.BAD + K.WS_BAD + K.PLAIN_ONLY + K.LOSS_ONLY


@pytest.mark.parametrize("name,change,word", BAD, ids=K.ids(BAD))
def test_device_form_rejects_before_touching_a_device(name, change, word):
    """dummy device pointers: a call that got past the checks would fault, a refusal never looks at them"""
    L = capi.load()
    a = dict(GOOD, **change)
    p = K.ptr
    rc = L.nntk_rnnt_loss_device(p(a["x"]), a["B"], a["T"], a["V"], _ints(a["il"]), _ints(a["lab"]), _ints(a["ll"]), a["ML"], a["blank"],
                                 p(a["loss"]), p(a["g"]), p(a["ws"]))
    assert rc == -1 and word in capi.last_error(), (name, capi.last_error())


HOST_BAD = [b for b in BAD if b[0].split()[0] not in ("misaligned", "gradient", "NULL") or b[0] in ("NULL labels", "NULL label lengths")]


@pytest.mark.parametrize("name,change,word", HOST_BAD, ids=K.ids(HOST_BAD))
def test_host_form_rejects_and_writes_nothing(name, change, word):
    L = capi.load()
    a = dict(GOOD, **change)
    n = 1 << 12                                           # never read: the refusal comes first
    x, loss, g = np.zeros(n, np.float32), np.full(n, 7.0, np.float32), np.full(n, 7.0, np.float32)
    rc = L.nntk_rnnt_loss(x.ctypes.data_as(capi.fp), a["B"], a["T"], a["V"], _ints(a["il"]), _ints(a["lab"]), _ints(a["ll"]), a["ML"],
                          a["blank"], loss.ctypes.data_as(capi.fp), g.ctypes.data_as(capi.fp))
    assert rc == -1 and word in capi.last_error(), (name, capi.last_error())
    assert (loss == 7.0).all() and (g == 7.0).all()


def test_host_form_null_arrays_and_the_empty_batch():
    L = capi.load()
    il, lab, ll = _ints(GOOD["il"]), _ints(GOOD["lab"]), _ints(GOOD["ll"])
    loss = np.full(2, 7.0, np.float32)
    assert L.nntk_rnnt_loss(None, 2, 6, 5, il, lab, ll, 3, 4, loss.ctypes.data_as(capi.fp), None) == -1 and "NULL" in capi.last_error()
    x = np.zeros(2 * 6 * 4 * 5, np.float32)
    assert L.nntk_rnnt_loss(x.ctypes.data_as(capi.fp), 2, 6, 5, il, lab, ll, 3, 4, None, None) == -1 and "NULL" in capi.last_error()
    assert (loss == 7.0).all()
    # an empty batch is not an error and needs no device either
    assert L.nntk_rnnt_loss(None, 0, 6, 5, None, None, None, 3, 4, None, None) == 0 and capi.last_error() == ""
    assert L.nntk_rnnt_loss_device(None, 0, 6, 5, None, None, None, 3, 4, None, None, None) == 0 and capi.last_error() == ""


JOINT_BAD = [("activation 3", dict(act=3), "activation"), ("activation -1", dict(act=-1), "activation"), ("batch < 0", dict(B=-1), "negative"),
             ("J < 0", dict(J=-4), "J"), ("NULL enc", dict(a=None), "NULL"), ("NULL pred / dout", dict(b=None), "NULL"),
             ("NULL out", dict(c=None), "NULL"), ("misaligned", dict(a=0x1002), "aligned")]


@pytest.mark.parametrize("name,change,word", JOINT_BAD, ids=[b[0] for b in JOINT_BAD])
def test_joiner_rejects_before_touching_a_device(name, change, word):
    L = capi.load()
    a = dict(dict(B=2, T=3, U1=4, J=8, act=1, a=0x1000, b=0x2000, c=0x3000, d=0x4000), **change)
    p = lambda v: None if v is None else C.c_void_p(v)
    assert L.nntk_rnnt_joint_device(p(a["a"]), p(a["b"]), a["B"], a["T"], a["U1"], a["J"], a["act"], p(a["c"])) == -1
    assert word in capi.last_error(), (name, capi.last_error())
    assert L.nntk_rnnt_joint_backward_device(p(a["a"]), p(a["b"]), a["B"], a["T"], a["U1"], a["J"], a["act"], p(a["c"]), p(a["d"])) == -1
    assert word in capi.last_error(), (name, capi.last_error())
    # an empty tensor is not an error
    assert L.nntk_rnnt_joint_device(None, None, 0, 3, 4, 8, 1, None) == 0 and capi.last_error() == ""
