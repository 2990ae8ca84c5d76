"""CPU-only: the attention entries are bound with their declared arguments, and their refusals are made on the host before anything
is enqueued (-1, a message, nothing written), so they need no device."""
import ctypes as C

import numpy as np
import pytest

from nntoolkitcore_amd import capi

HD = 2 * 8              # heads * d_head of the made-up call


def _call(L, entry="nntk_attention_device", **kw):
    """the entry on made-up (never dereferenced) addresses, far apart; kw overrides an argument"""
    a = dict(q=C.c_void_p(0x1000000), k=C.c_void_p(0x2000000), v=C.c_void_p(0x3000000), batch=2, heads=2, d_head=8, Tq=10, Tk=12,
             qfs=HD, qbs=10 * HD, kfs=HD, kbs=12 * HD, vfs=HD, vbs=12 * HD, kv_lengths=None, q_offset=2, pos0=0, chunk=1, left=-1,
             right=-1, scale=0.5, out=C.c_void_p(0x4000000), lse=C.c_void_p(0x5000000))
    a.update(kw)
    return getattr(L, entry)(*a.values())


def test_both_entries_are_bound_with_23_arguments():
    for name in ("nntk_attention_device", "nntk_attention"):
        assert len(capi.SIGNATURES[name][1]) == 23


@pytest.mark.parametrize("kw,word", [
    (dict(q=None), "NULL"), (dict(k=None), "NULL"), (dict(v=None), "NULL"), (dict(out=None), "NULL"),
    (dict(d_head=0), "d_head"), (dict(d_head=129), "128"), (dict(heads=0), "heads"), (dict(heads=65), "64"),
    (dict(Tq=0), "Tq"), (dict(Tk=32769, kbs=0, vbs=0), "32768"), (dict(q_offset=3), "q_offset"), (dict(q_offset=-1), "q_offset"),
    (dict(batch=-1), "batch"), (dict(chunk=0), "chunk"), (dict(left=-2), "left"), (dict(right=-2), "right"),
    (dict(pos0=-1), "pos0"), (dict(pos0=2 ** 30 - 11), "pos0"),
    (dict(qfs=HD - 1), "stride"), (dict(kfs=HD - 1), "stride"), (dict(vfs=0), "stride"), (dict(kbs=-1), "stride"),
    (dict(q=C.c_void_p(0x1000002)), "aligned"), (dict(lse=C.c_void_p(0x5000001)), "aligned"),
    (dict(scale=float("nan")), "scale"), (dict(scale=float("inf")), "scale"),
    (dict(out=C.c_void_p(0x2000000 + 4 * (2 * 12 * HD - 1))), "overlap"),          # the last float of k
    (dict(lse=C.c_void_p(0x3000000)), "overlap"), (dict(lse=C.c_void_p(0x4000000 + 4 * (2 * 10 * HD - 1))), "overlap"),
])
def test_device_entry_refusals_need_no_device(built_lib, kw, word):
    assert _call(built_lib, **kw) == -1
    err = capi.last_error()
    assert err.startswith("nntk_attention_device") and word in err, err


@pytest.mark.parametrize("lengths", [[12, 13], [-1, 5]])
def test_key_count_outside_its_range_is_refused(built_lib, lengths):
    kl = np.asarray(lengths, np.int32)
    assert _call(built_lib, kv_lengths=kl.ctypes.data_as(capi.ip)) == -1
    assert "kv_lengths" in capi.last_error() and "[0, Tk = 12]" in capi.last_error()


def test_host_entry_refuses_the_same_and_writes_nothing(built_lib):
    q, k, v = (np.zeros((2, t, HD), np.float32) for t in (10, 12, 12))
    out, lse = np.full((2, 10, HD), 77, np.float32), np.full((2, 2, 10), 77, np.float32)
    p = lambda a: a.ctypes.data_as(capi.fp)
    host = dict(entry="nntk_attention", q=p(q), k=p(k), v=p(v), out=p(out), lse=p(lse))
    for kw, word in ((dict(d_head=129), "128"), (dict(chunk=0), "chunk"), (dict(k=None), "NULL"), (dict(out=p(v)), "overlap"),
                     (dict(kv_lengths=np.asarray([3, 13], np.int32).ctypes.data_as(capi.ip)), "kv_lengths")):
        assert _call(built_lib, **{**host, **kw}) == -1
        assert capi.last_error().startswith("nntk_attention:") and word in capi.last_error(), capi.last_error()
    assert (out == 77).all() and (lse == 77).all() and not v.any()


def test_empty_batch_needs_no_device(built_lib):
    for entry in ("nntk_attention_device", "nntk_attention"):
        assert _call(built_lib, entry=entry, q=None, k=None, v=None, out=None, lse=None, batch=0) == 0 and capi.last_error() == ""
