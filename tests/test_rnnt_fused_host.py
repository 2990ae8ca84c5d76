"""The host side of the fused transducer training loss (csrc/host/rnnt.c, nntk_rnnt_fused_*): every refusal, made before anything is
allocated, uploaded or enqueued; the workspace size, which is the point of the call -- nothing in it grows like batch T U1 V; and the
float64 reference of the device tests (tests/rnnt_fused_reference.py) against autograd.  No GPU."""

import numpy as np
import pytest
import torch

import rnnt_cases as K
import rnnt_fused_reference as FR
from nntoolkitcore_amd import capi


@pytest.mark.parametrize("kind", ["identity", "tanh", "relu"])
def test_reference_gradients_equal_autograd_in_float64(kind):
    rng = np.random.default_rng(5)
    B, T, ML, J, V, blank = 3, 7, 5, 6, 5, 2
    labels, lens = [[0, 0, 3], [], [1, 4, 4, 3, 0]], [7, 4, 1]
    enc, pred, out = rng.uniform(-1, 1, (B, T, J)), rng.uniform(-1, 1, (B, ML + 1, J)), rng.uniform(-1, 1, J * V + V)
    for b in range(B):                                   # the padding is never looked at
        enc[b, lens[b]:] = np.nan
        pred[b, len(labels[b]) + 1:] = np.nan
    got = FR.fused_loss_and_grads(enc, pred, out, labels, lens, blank, kind)
    ref = FR.torch_fused(enc, pred, out, labels, lens, blank, kind, torch.float64)
    for g, r in zip(got, ref):
        assert np.isfinite(g).all()
        np.testing.assert_allclose(g, r, rtol=1e-10, atol=1e-12)
    assert not got[1][1, 4:].any() and not got[2][1, 1:].any() and not got[2][0, 4:].any()


def test_workspace_has_no_part_of_the_size_of_the_logits():
    f = capi.load().nntk_rnnt_fused_workspace_floats
    assert f(1, 1, 0, 1, 2, 0) > 0 and f(0, 0, 0, 1, 2, 1) > 0
    for J, V in ((1, 2), (64, 512), (512, 4096), (1024, 8192)):
        for g in (0, 1):
            for B, T, L in ((1, 1, 1), (3, 50, 7), (16, 200, 40)):
                w = f(B, T, L, J, V, g)
                assert f(B + 1, T, L, J, V, g) > w and f(B, T + 1, L, J, V, g) > w and f(B, T, L + 1, J, V, g) > w
                assert f(B, T, L, J, V + 1, g) >= w and f(B, T, L, J + 1 if J < 1024 else J, V, g) >= w
                # doubling the cells: at most 4 (J + 16) bytes per added cell with a gradient, 32 without
                cells = B * T * (L + 1)
                added = 4 * (f(2 * B, T, L, J, V, g) - w)
                assert added <= cells * (4 * (J + 16) if g else 32), (J, V, g, B, T, L, added / cells)
    # what V costs does not depend on the batch, T or the labels
    for J in (64, 512, 1024):
        for g in (0, 1):
            d = {f(B, T, L, J, 8192, g) - f(B, T, L, J, 2, g) for B, T, L in ((1, 1, 1), (16, 200, 40), (64, 500, 100))}
            assert len(d) == 1, (J, g, d)
    assert f(1, 1, 1, 64, 8192, 0) == f(1, 1, 1, 64, 2, 0)                      # loss only: V costs nothing at all
    # a training shape: the whole fused workspace is under half of ONE of the composed route's two [B][T][U1][V] tensors
    assert f(16, 200, 40, 512, 4096, 1) < 16 * 200 * 41 * 4096 / 2
    assert f(64, 1000, 4000, 1024, 8192, 1) > 2 ** 31                            # no 32-bit arithmetic inside


GOOD, _ints = K.GOOD, K.ints
BAD = K.BAD + K.WS_BAD + K.FUSED_ONLY + K.FUSED_LOSS_ONLY


@pytest.mark.parametrize("name,change,word", BAD, ids=K.ids(BAD))
def test_device_form_rejects_before_touching_a_device(name, change, word):
    """dummy device pointers: a call that got past the checks would fault, a refusal never looks at them"""
    L = capi.load()
    a = dict(GOOD, **change)
    p = K.ptr
    rc = L.nntk_rnnt_fused_loss_device(p(a["enc"]), p(a["pred"]), p(a["out"]), a["B"], a["T"], a["J"], a["V"], a["act"], _ints(a["il"]),
                                       _ints(a["lab"]), _ints(a["ll"]), a["ML"], a["blank"], p(a["loss"]), p(a["denc"]), p(a["dpred"]),
                                       p(a["dout"]), p(a["ws"]))
    assert rc == -1 and word in capi.last_error(), (name, capi.last_error())


HOST_BAD = [b for b in BAD if b[0].split()[0] not in ("misaligned", "NULL", "d_denc", "d_dpred", "d_dout", "loss")
            or b[0] in ("NULL labels", "NULL label lengths", "d_dout missing", "d_denc missing")]


@pytest.mark.parametrize("name,change,word", HOST_BAD, ids=K.ids(HOST_BAD))
def test_host_form_rejects_and_writes_nothing(name, change, word):
    L = capi.load()
    a = dict(GOOD, **change)
    n = 1 << 12                                           # never read: the refusal comes first
    x = np.zeros(n, np.float32)
    outs = {k: np.full(n, 7.0, np.float32) for k in ("loss", "denc", "dpred", "dout")}
    q = lambda k: None if a[k] is None else outs[k].ctypes.data_as(capi.fp)
    xp = x.ctypes.data_as(capi.fp)
    rc = L.nntk_rnnt_fused_loss(xp, xp, xp, a["B"], a["T"], a["J"], a["V"], a["act"], _ints(a["il"]), _ints(a["lab"]), _ints(a["ll"]), a["ML"],
                                a["blank"], q("loss"), q("denc"), q("dpred"), q("dout"))
    assert rc == -1 and word in capi.last_error(), (name, capi.last_error())
    assert all((o == 7.0).all() for o in outs.values())


def test_the_empty_batch_is_not_an_error():
    L = capi.load()
    assert L.nntk_rnnt_fused_loss_device(None, None, None, 0, 6, 8, 5, 1, None, None, None, 3, 4, None, None, None, None, None) == 0
    assert capi.last_error() == ""
    assert L.nntk_rnnt_fused_loss(None, None, None, 0, 6, 8, 5, 1, None, None, None, 3, 4, None, None, None, None) == 0
    assert capi.last_error() == ""
