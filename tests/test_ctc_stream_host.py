"""Streaming CTC decoding: what the host layer decides before any device is touched (csrc/host/ctc.c) -- the checks of
nntk_ctc_beam_stream_create, the size of a handle's device memory, the empty batch, the exported symbols.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from nntoolkitcore_amd import capi

GOOD = dict(batch=2, max_frames=8, C=5, blank=4, W=4, cut=0, nbest=2, max_labels=16)
BAD = [dict(W=0), dict(W=129, nbest=1), dict(nbest=0), dict(nbest=5), dict(cut=-1), dict(blank=5), dict(blank=-1), dict(max_frames=0),
       dict(max_labels=0), dict(batch=-1), dict(W=128, C=130, nbest=1)]


def _create(a):
    return capi.load().nntk_ctc_beam_stream_create(a["batch"], a["max_frames"], a["C"], a["blank"], a["W"], a["cut"], a["nbest"],
                                                   a["max_labels"])


@pytest.mark.parametrize("change", BAD, ids=lambda c: ",".join("%s=%s" % kv for kv in c.items()))
def test_create_refuses_bad_arguments(change):
    h = _create(dict(GOOD, **change))
    assert not h and capi.last_error() != ""


def test_the_cell_limit_is_named():
    assert not _create(dict(GOOD, W=128, C=130, nbest=1))
    assert "16384" in capi.last_error()


def test_create_and_destroy_need_no_device():
    L = capi.load()
    h = _create(GOOD)
    assert h and capi.last_error() == ""
    assert L.nntk_ctc_beam_stream_reset(h, (C.c_int * 2)(1, 0), 2) == 0
    assert L.nntk_ctc_beam_stream_reset(h, (C.c_int * 1)(2), 1) == -1 and capi.last_error() != ""
    L.nntk_ctc_beam_stream_destroy(h)
    L.nntk_ctc_beam_stream_destroy(None)


def test_state_bytes_are_monotone_and_64_bit():
    sb = capi.load().nntk_ctc_beam_stream_state_bytes
    base = sb(4, 50, 29, 16, 0, 100)
    assert base > 0
    assert sb(5, 50, 29, 16, 0, 100) > base and sb(4, 51, 29, 16, 0, 100) > base and sb(4, 50, 29, 17, 0, 100) > base
    assert sb(4, 50, 29, 16, 0, 101) > base
    assert sb(4, 50, 29, 16, 5, 100) > base                   # the class cut's pairs
    assert sb(4, 50, 29, 16, 28, 100) == base and sb(4, 50, 29, 16, 40, 100) == base and sb(4, 50, 30, 16, 0, 100) >= base
    # the carried state alone: 40 bytes per entry and two label strings, whatever a push holds
    per_entry = (sb(4, 50, 29, 17, 0, 100) - base - 4 * 50 * 8) / 4
    assert per_entry == 40 + 2 * 4 * 100
    assert sb(4096, 1000, 64, 128, 0, 4096) > 2 ** 34


def test_empty_batch_needs_no_device():
    L = capi.load()
    h = _create(dict(GOOD, batch=0))
    assert h and capi.last_error() == ""
    assert L.nntk_ctc_beam_stream_push_device(h, None, None, None, None, None, None) == 0
    assert L.nntk_ctc_beam_stream_push(h, None, None, None, None, None, None) == 0
    assert L.nntk_ctc_beam_stream_reset(h, None, 0) == 0
    assert capi.last_error() == ""
    L.nntk_ctc_beam_stream_destroy(h)
    assert L.nntk_ctc_greedy_decode_stream_device(None, 0, 6, 5, None, 4, None, None, None) == 0 and capi.last_error() == ""


def test_push_checks_come_before_any_device_use():
    """a refused push returns before the handle's device memory is reserved"""
    L = capi.load()
    h = _create(GOOD)
    lab, n, sc = np.full((2, 2, 16), 7, np.int32), np.full((2, 2), 7, np.int32), np.full((2, 2), 7.0, np.float32)
    p = np.full((2, 8, 5), 0.2, np.float32)
    args = (lab.ctypes.data_as(capi.ip), n.ctypes.data_as(capi.ip), sc.ctypes.data_as(capi.fp))
    for nf in ([-1, 3], [3, 9]):
        nf = np.asarray(nf, np.int32)
        assert L.nntk_ctc_beam_stream_push(h, p.ctypes.data_as(capi.fp), nf.ctypes.data_as(capi.ip), None, *args) == -1
        assert capi.last_error() != ""
    nf = np.asarray([1, 1], np.int32)
    assert L.nntk_ctc_beam_stream_push(h, None, nf.ctypes.data_as(capi.ip), None, *args) == -1 and capi.last_error() != ""
    assert L.nntk_ctc_beam_stream_push(h, p.ctypes.data_as(capi.fp), None, None, *args) == -1 and capi.last_error() != ""
    assert (lab == 7).all() and (n == 7).all() and (sc == 7.0).all()
    L.nntk_ctc_beam_stream_destroy(h)
    bad = np.asarray([7, 0], np.int32)
    assert L.nntk_ctc_greedy_decode_stream_device(None, 2, 6, 5, bad.ctypes.data_as(capi.ip), 4, None, None, None) == -1
    assert L.nntk_ctc_greedy_decode_stream_device(None, 2, 6, 5, None, 4, None, None, None) == -1 and capi.last_error() != ""


def test_the_symbols_are_exported_and_bound():
    L = capi.load()
    for name in ("nntk_ctc_beam_stream_create", "nntk_ctc_beam_stream_state_bytes", "nntk_ctc_beam_stream_push_device",
                 "nntk_ctc_beam_stream_reset", "nntk_ctc_beam_stream_destroy", "nntk_ctc_beam_stream_push",
                 "nntk_ctc_greedy_decode_stream_device"):
        assert name in capi.SIGNATURES and getattr(L, name).argtypes == capi.SIGNATURES[name][1], name
