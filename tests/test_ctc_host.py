"""The host side of the CTC calls (csrc/host/ctc.c): the workspace size and the argument checks of the host-pointer forms, which
run before anything is allocated, uploaded or enqueued.  No GPU."""
import numpy as np

from nntoolkitcore_amd import capi


def test_workspace_size_is_nonzero_and_monotone():
    f = capi.load().nntk_ctc_workspace_floats
    assert f(1, 1, 0) > 0 and f(0, 0, 0) > 0
    for B, T, L in ((1, 1, 1), (3, 50, 7), (64, 400, 130)):
        assert f(B, T, L) >= 2 * 2 * B * T * (2 * L + 1)               # both passes keep a pair of words per state and frame
        assert f(B + 1, T, L) > f(B, T, L) and f(B, T + 1, L) > f(B, T, L) and f(B, T, L + 1) > f(B, T, L)
    assert f(512, 1000, 100) > 2 ** 28                                  # no 32-bit arithmetic inside
    assert f(8, 0, 20) < f(8, 1, 20)                                    # T = 0: what a loss-only call touches


def _loss(L, p, il, lab, ll, blank, B=2, T=6, Cc=5, ML=3):
    ip = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(capi.ip)
    loss, g = np.full(B, 7.0, np.float32), np.full((B, T, Cc), 7.0, np.float32)
    rc = L.nntk_ctc_loss(p.ctypes.data_as(capi.fp), B, T, Cc, ip(il), ip(lab), ip(ll), ML, blank, loss.ctypes.data_as(capi.fp),
                         g.ctypes.data_as(capi.fp))
    return rc, loss, g


def test_host_forms_reject_bad_arguments_before_touching_a_device():
    L = capi.load()
    p = np.full((2, 6, 5), 0.2, np.float32)
    good = dict(il=[6, 4], lab=[[1, 2, 0], [3, 0, 0]], ll=[2, 1], blank=4)
    bad = [dict(il=[7, 4]), dict(il=[6, -1]), dict(ll=[4, 1]), dict(ll=[2, -1]), dict(lab=[[1, 4, 0], [3, 0, 0]]),
           dict(lab=[[1, 5, 0], [3, 0, 0]]), dict(lab=[[-1, 2, 0], [3, 0, 0]]), dict(blank=5), dict(blank=-1)]
    for change in bad:
        a = dict(good, **change)
        rc, loss, g = _loss(L, p, a["il"], a["lab"], a["ll"], a["blank"])
        assert rc == -1 and capi.last_error() != "", change
        assert (loss == 7.0).all() and (g == 7.0).all(), change
    # a label beyond a row's label length is padding: not looked at
    out, n = np.full((2, 6), 7, np.int32), np.full(2, 7, np.int32)
    for il, blank in (([7, 4], 0), ([6, -3], 0), ([6, 4], 5), ([6, 4], -1)):
        rc = L.nntk_ctc_greedy_decode(p.ctypes.data_as(capi.fp), 2, 6, 5, np.asarray(il, np.int32).ctypes.data_as(capi.ip), blank,
                                      out.ctypes.data_as(capi.ip), n.ctypes.data_as(capi.ip))
        assert rc == -1 and capi.last_error() != "", (il, blank)
        assert (out == 7).all() and (n == 7).all()
    # an empty batch is not an error and needs no device either
    assert L.nntk_ctc_loss(None, 0, 6, 5, None, None, None, 3, 4, None, None) == 0 and capi.last_error() == ""
