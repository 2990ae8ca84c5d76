"""CTC forced alignment: what the host layer decides before any device is touched (csrc/host/ctc.c) -- the workspace size and the
argument checks of the host-pointer form.  No GPU."""
import numpy as np
import pytest

from nntoolkitcore_amd import capi


def test_workspace_size_is_monotone_and_64_bit():
    ws = capi.load().nntk_ctc_align_workspace_floats
    assert ws(0, 0, 0) > 0 and ws(1, 1, 0) > 0
    for B, T, L in ((1, 1, 1), (3, 50, 7), (64, 400, 130)):
        base = ws(B, T, L)
        assert 4 * base >= B * T * (2 * L + 1) + 4 * B * (3 + L)            # a byte per row, frame and state, and the int header
        assert 4 * base <= B * T * (2 * L + 1) + 4 * B * (3 + L) + 64        # ... and no more than a byte
        assert ws(B + 1, T, L) >= base and ws(B, T + 1, L) >= base and ws(B, T, L + 1) >= base
        assert ws(B + 16, T, L) > base and ws(B, T + 16, L) > base and ws(B, T, L + 8) > base       # (sizes are whole 16 bytes)
    assert 4 * ws(512, 1000, 200) >= 512 * 1000 * 401
    assert 4 * ws(512, 4000, 4000) >= 512 * 4000 * 8001 > 2 ** 33            # no 32-bit arithmetic inside


GOOD = dict(il=[6, 4], lab=[[1, 2, 0], [3, 0, 0]], ll=[2, 1], blank=4)
BAD = [dict(il=[7, 4]), dict(il=[6, -1]), dict(ll=[4, 1]), dict(ll=[2, -1]), dict(lab=[[1, 4, 0], [3, 0, 0]]),
       dict(lab=[[1, 5, 0], [3, 0, 0]]), dict(lab=[[-1, 2, 0], [3, 0, 0]]), dict(blank=5), dict(blank=-1)]


def _align(L, p, il, lab, ll, blank, B, T, Cc, ML):
    ip = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(capi.ip)
    st, sp, sc = np.full((B, T), 7, np.int32), np.full((B, ML, 2), 7, np.int32), np.full(B, 7.0, np.float32)
    rc = L.nntk_ctc_align(p.ctypes.data_as(capi.fp), B, T, Cc, ip(il), ip(lab), ip(ll), ML, blank, st.ctypes.data_as(capi.ip),
                          sp.ctypes.data_as(capi.ip), sc.ctypes.data_as(capi.fp))
    return rc, st, sp, sc


@pytest.mark.parametrize("change", BAD, ids=lambda c: ",".join("%s=%s" % kv for kv in c.items()))
def test_host_form_refuses_what_the_loss_refuses_and_writes_nothing(change):
    L = capi.load()
    p = np.full((2, 6, 5), 0.2, np.float32)
    a = dict(GOOD, **change)
    ip = lambda v: np.ascontiguousarray(v, np.int32).ctypes.data_as(capi.ip)
    loss = np.full(2, 7.0, np.float32)
    assert L.nntk_ctc_loss(p.ctypes.data_as(capi.fp), 2, 6, 5, ip(a["il"]), ip(a["lab"]), ip(a["ll"]), 3, a["blank"],
                           loss.ctypes.data_as(capi.fp), None) == -1                 # the loss refuses it ...
    rc, st, sp, sc = _align(L, p, a["il"], a["lab"], a["ll"], a["blank"], 2, 6, 5, 3)
    assert rc == -1 and capi.last_error().startswith("nntk_ctc_align")              # ... and so does the alignment
    assert (st == 7).all() and (sp == 7).all() and (sc == 7.0).all()


def test_the_label_limit_is_named():
    L = capi.load()
    p = np.full((1, 2, 3), 1.0 / 3, np.float32)
    lab = np.ones((1, 4001), np.int32)
    rc, st, sp, sc = _align(L, p, None, lab, [1], 0, 1, 2, 3, 4001)
    assert rc == -1 and "4000" in capi.last_error() and "4001" in capi.last_error()
    assert (st == 7).all() and (sp == 7).all() and (sc == 7.0).all()
    assert L.nntk_ctc_align_device(None, 1, 2, 3, None, lab.ctypes.data_as(capi.ip), np.ones(1, np.int32).ctypes.data_as(capi.ip), 4001, 0,
                                   None, None, None, None) == -1 and "4000" in capi.last_error()


def test_empty_batch_needs_no_device():
    L = capi.load()
    assert L.nntk_ctc_align(None, 0, 6, 5, None, None, None, 3, 4, None, None, None) == 0 and capi.last_error() == ""
    assert L.nntk_ctc_align_device(None, 0, 6, 5, None, None, None, 3, 4, None, None, None, None) == 0 and capi.last_error() == ""
