"""CPU-only: the attention backward entries are bound with their declared arguments, and what they refuse beyond the forward call
is refused on the host before anything is enqueued (-1, a message, nothing written), so it needs no device."""
import ctypes as C

import numpy as np
import pytest

from nntoolkitcore_amd import capi

HD = 2 * 8              # heads * d_head of the made-up call
GFS = 3 * HD            # dq, dk, dv as the thirds of one fused gradient buffer (Tq == Tk == 12)
G = 0x8000000


def _call(L, entry="nntk_attention_backward_device", **kw):
    """the entry on made-up (never dereferenced) addresses, far apart; kw overrides an argument"""
    a = dict(q=C.c_void_p(0x1000000), k=C.c_void_p(0x2000000), v=C.c_void_p(0x3000000), out=C.c_void_p(0x4000000), lse=C.c_void_p(0x5000000),
             dout=C.c_void_p(0x6000000), batch=2, heads=2, d_head=8, Tq=12, Tk=12, qfs=HD, qbs=12 * HD, kfs=HD, kbs=12 * HD, vfs=HD,
             vbs=12 * HD, kv_lengths=None, q_offset=0, pos0=0, chunk=1, left=-1, right=-1, scale=0.5, gfs=GFS, dq=C.c_void_p(G),
             dk=C.c_void_p(G + 4 * HD), dv=C.c_void_p(G + 8 * HD), ws=C.c_void_p(0x9000000))
    a.update(kw)
    if entry == "nntk_attention_backward":
        del a["ws"]
    return getattr(L, entry)(*a.values())


def test_entries_are_bound_as_declared(built_lib):
    assert len(capi.SIGNATURES["nntk_attention_backward_device"][1]) == 29 and len(capi.SIGNATURES["nntk_attention_backward"][1]) == 28
    assert built_lib.nntk_attention_backward_workspace_floats(3, 5, 7) == 3 * 5 * 7
    assert built_lib.nntk_attention_backward_workspace_floats(3, 0, 7) == 0


@pytest.mark.parametrize("kw,word", [
    (dict(out=None), "NULL"), (dict(lse=None), "NULL"), (dict(dout=None), "NULL"), (dict(dq=None), "NULL"), (dict(dk=None), "NULL"),
    (dict(dv=None), "NULL"), (dict(ws=None), "NULL"), (dict(d_head=129), "128"), (dict(chunk=0), "chunk"),
    (dict(gfs=HD - 1), "grad_frame_stride"), (dict(dout=C.c_void_p(0x6000002)), "aligned"), (dict(dk=C.c_void_p(G + 4 * HD + 1)), "aligned"),
    (dict(dv=C.c_void_p(0x2000000 + 4 * (2 * 12 * HD - 1))), "overlap"),          # the last float of k
    (dict(ws=C.c_void_p(0x6000000)), "overlap"),                                  # the workspace on dout
    (dict(dk=C.c_void_p(G + 4 * (HD - 1))), "overlap"),                           # dk's slice starts on the last float of dq's
    (dict(ws=C.c_void_p(G + 4 * 100)), "overlap"),                                # the workspace inside the gradient buffer
])
def test_refusals_need_no_device(built_lib, kw, word):
    assert _call(built_lib, **kw) == -1
    err = capi.last_error()
    assert err.startswith("nntk_attention_backward_device") and word in err, err


def test_host_entry_refuses_and_writes_nothing(built_lib):
    q, k, v, out, dout = (np.zeros((2, 12, HD), np.float32) for _ in range(5))
    lse, grad = np.zeros((2, 2, 12), np.float32), np.full((2, 12, GFS), 77, np.float32)
    p = lambda a, off=0: C.cast(a.ctypes.data + 4 * off, capi.fp)
    host = dict(entry="nntk_attention_backward", q=p(q), k=p(k), v=p(v), out=p(out), lse=p(lse), dout=p(dout), dq=p(grad), dk=p(grad, HD),
                dv=p(grad, 2 * HD))
    for kw, word in ((dict(heads=65), "64"), (dict(lse=None), "NULL"), (dict(gfs=HD - 1), "grad_frame_stride"), (dict(dq=p(k)), "overlap"),
                     (dict(dv=p(grad, 2 * HD - 1)), "overlap")):
        assert _call(built_lib, **{**host, **kw}) == -1
        assert capi.last_error().startswith("nntk_attention_backward:") and word in capi.last_error(), capi.last_error()
    assert (grad == 77).all() and not k.any()


def test_empty_batch_needs_no_device(built_lib):
    none = dict(q=None, k=None, v=None, out=None, lse=None, dout=None, dq=None, dk=None, dv=None, ws=None, batch=0)
    for entry in ("nntk_attention_backward_device", "nntk_attention_backward"):
        assert _call(built_lib, entry=entry, **none) == 0 and capi.last_error() == ""
