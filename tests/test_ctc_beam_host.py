"""CTC prefix beam search: what the host layer decides before any device is touched (csrc/host/ctc.c) -- the workspace size and
the argument checks of the host-pointer form.  No GPU."""
import numpy as np
import pytest

from nntoolkitcore_amd import capi


def test_workspace_size_is_monotone_and_64_bit():
    ws = capi.load().nntk_ctc_beam_workspace_floats
    base = ws(4, 100, 29, 16, 0)
    assert base > 0
    assert ws(5, 100, 29, 16, 0) > base and ws(4, 101, 29, 16, 0) > base and ws(4, 100, 29, 17, 0) > base
    assert ws(4, 100, 29, 16, 5) > base                      # the class cut's pairs
    assert ws(4, 100, 29, 16, 28) == base and ws(4, 100, 29, 16, 40) == base
    assert ws(512, 1000, 64, 128, 0) > 2 ** 28


BAD = [dict(il=[7, 4]), dict(il=[6, -1]), dict(blank=5), dict(blank=-1), dict(W=0), dict(W=129, nbest=1), dict(nbest=0), dict(nbest=5),
       dict(cut=-1), dict(W=128, C=130, nbest=1)]


@pytest.mark.parametrize("change", BAD, ids=lambda c: ",".join("%s=%s" % kv for kv in c.items()))
def test_host_form_refuses_bad_arguments_and_writes_nothing(change):
    L = capi.load()
    B, T = 2, 6
    a = dict(dict(il=[6, 4], blank=4, W=4, nbest=2, cut=0, C=5), **change)
    nb = max(a["nbest"], 1)
    p = np.full((B, T, a["C"]), 1.0 / a["C"], np.float32)
    lab, n, sc = np.full((B, nb, T), 7, np.int32), np.full((B, nb), 7, np.int32), np.full((B, nb), 7.0, np.float32)
    il = np.asarray(a["il"], np.int32)
    rc = L.nntk_ctc_beam_decode(p.ctypes.data_as(capi.fp), B, T, a["C"], il.ctypes.data_as(capi.ip), a["blank"], a["W"], a["cut"],
                                a["nbest"], lab.ctypes.data_as(capi.ip), n.ctypes.data_as(capi.ip), sc.ctypes.data_as(capi.fp))
    assert rc == -1 and capi.last_error() != ""
    assert (lab == 7).all() and (n == 7).all() and (sc == 7.0).all()


def test_the_cell_limit_is_named():
    L = capi.load()
    p = np.full((1, 2, 130), 1.0 / 130, np.float32)
    lab, n, sc = np.zeros((1, 1, 2), np.int32), np.zeros((1, 1), np.int32), np.zeros((1, 1), np.float32)
    rc = L.nntk_ctc_beam_decode(p.ctypes.data_as(capi.fp), 1, 2, 130, None, 0, 128, 0, 1, lab.ctypes.data_as(capi.ip),
                                n.ctypes.data_as(capi.ip), sc.ctypes.data_as(capi.fp))
    assert rc == -1 and "16384" in capi.last_error()


def test_empty_batch_needs_no_device():
    L = capi.load()
    rc = L.nntk_ctc_beam_decode(None, 0, 6, 5, None, 4, 4, 0, 2, None, None, None)
    assert rc == 0 and capi.last_error() == ""
