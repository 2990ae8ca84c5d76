"""The streamed token-and-duration beam search (csrc/hip/rnnt_tdt_beam.hip, the STREAM instantiations) against the one-shot device call,
which tests/test_gpu_rnnt_tdt_beam*.py tie to the float64 reference: after every push every output EQUALS, bit for bit, the one-shot
call's on the frames pushed so far.  No reference of its own, no tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_rnnt_tdt_beam_host as H
from nntoolkitcore_amd import capi, layers as NL
from rnnt_beam_device import host as _host, same as _same, to_device as _t
from test_gpu_rnnt_tdt_beam import _decoder
from test_rnnt_tdt_beam_opt_host import ALPHA, BETA, case as _opt_case, table as _table

pytestmark = pytest.mark.gpu
SPLITS = {"1": [1] * 11, "3": [3] * 4, "uneven": [2, 0, 5, 1, 3, 0, 4], "whole": [11]}
_p = lambda t: C.c_void_p(t if isinstance(t, int) else t.data_ptr())
_ip = lambda a: np.asarray(a, np.int32).ctypes.data_as(capi.ip)


def _setup(gpu, name, on):
    c = _opt_case(name) if name.startswith("awkward") else H.case(name)
    kw = dict(lm=NL.NgramLm.from_arrays(alpha=ALPHA, beta=BETA, **_table(name)), detail=True, length_norm=True) if on else {}
    return c, _decoder(gpu, c), kw


def _chunk(c, enc, N, size):
    """the push after N frames: a row gets min(size, what it has left), the rest of its chunk is NaN"""
    take = [max(0, min(size, n - N)) for n in c["n"]]
    chunk = np.full((enc.shape[0], size, enc.shape[2]), np.nan, np.float32)
    for b, k in enumerate(take):
        chunk[b, :k] = enc[b, N:N + k]
    return chunk, take


def _one_shot(gpu, dec, c, N, kw):
    enc = _t(gpu, np.ascontiguousarray(c["enc"][:, :N]))
    return _host(dec.tdt_beam_decode(enc, [min(n, N) for n in c["n"]], c["W"], c["nbest"], c["max_labels"], **kw))


def _pushes(gpu, dec, c, sizes, kw, enc=None):
    s, N, got = NL.RnntTdtBeamStream(dec, len(c["n"]), c["W"], c["max_labels"], **kw), 0, []
    for size in sizes:
        chunk, take = _chunk(c, c["enc"] if enc is None else enc, N, size)
        N += size
        got.append((N, _host(s.push(_t(gpu, chunk), take, c["nbest"]))))
    return s.close() or got


@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("name,on", [("awkward", False), ("awkward", True), ("skip", False), ("clamp", False), ("pruned", False), ("ring", False)])
def test_every_push_equals_the_one_shot_call_on_the_frames_so_far(gpu, name, on, split):
    c, dec, kw = _setup(gpu, name, on)
    enc = c["enc"].copy()
    if name == "skip":                                                               # durations (0, 2, 4): odd frames are never landed on
        enc[:, 1::2] = np.nan
    for N, got in _pushes(gpu, dec, c, SPLITS[split], kw, enc):
        want = _one_shot(gpu, dec, c, N, kw)
        assert len(got) == (6 if on else 3) and _same(got, want), (name, split, N, got, want)
    dec.destroy()


def test_a_reset_row_starts_again_and_the_others_continue(gpu):
    c, dec, kw = _setup(gpu, "awkward", True)
    s, at = NL.RnntTdtBeamStream(dec, 3, c["W"], c["max_labels"], **kw), [0, 0, 0]
    for i in range(5):                                                               # 3 frames a push; row 1 (4 frames) starts again after the first
        take = [max(0, min(3, n - a)) for n, a in zip(c["n"], at)]
        chunk = np.zeros((3, 3, c["enc"].shape[2]), np.float32)
        for b, k in enumerate(take):
            chunk[b, :k] = c["enc"][b, at[b]:at[b] + k]
        got = _host(s.push(_t(gpu, chunk), take, c["nbest"]))
        at = [a + k for a, k in zip(at, take)]
        if i == 0:
            s.reset([1])
            at[1] = 0
    assert at == c["n"] and _same(got, _one_shot(gpu, dec, c, 10, kw))
    s.close(); dec.destroy()


def test_host_pointer_form_and_group_size_change_no_bit(gpu):
    """the device form with the hypotheses one by one, the host-pointer form with the default group: the same bits after every push"""
    L = capi.load()
    c, dec, kw = _setup(gpu, "awkward", True)
    try:
        L.nntk_shim_rnnt_tdt_beam_set_group(1)
        device = _pushes(gpu, dec, c, SPLITS["uneven"], kw)
    finally:
        L.nntk_shim_rnnt_tdt_beam_set_group(0)
    s, shape = NL.RnntTdtBeamStream(dec, 3, c["W"], c["max_labels"], **kw), (3, c["nbest"], c["max_labels"])
    outs = [np.empty(shape[:n], t) for n, t in ((3, np.int32), (2, np.int32), (2, np.float32), (3, np.int32), (3, np.int32), (3, np.float32))]
    o = capi.NntkRnntTdtBeamOptions(kw["lm"].h, 1, *(x.ctypes.data for x in outs[3:]))
    for (N, want), size in zip(device, SPLITS["uneven"]):
        chunk, take = _chunk(c, c["enc"], N - size, size)
        assert L.nntk_rnnt_tdt_beam_stream_push(dec.h, s.h, chunk.ctypes.data_as(capi.fp), 3, size, _ip(take), c["nbest"], C.byref(o),
                                                *(x.ctypes.data_as(capi.ip) for x in outs[:2]), outs[2].ctypes.data_as(capi.fp)) == 0, capi.last_error()
        assert _same(outs, want), N
    s.close(); dec.destroy()


def test_refusals_write_nothing_leave_the_state_as_it_was_and_the_sizes_are_as_stated(gpu):
    L = capi.load()
    c, tdt, kw = _setup(gpu, "awkward", True)
    (B, T, _), W, NB, ML, m = c["enc"].shape, c["W"], c["nbest"], c["max_labels"], c["m"]
    tdt2 = _decoder(gpu, c)
    classic = NL.RnntDecoder(_t(gpu, m["embed"]), _t(gpu, m["lstm"]), _t(gpu, m["proj"]), _t(gpu, m["out"][:23 * 5]), blank=0)
    lm, lm2 = kw["lm"], NL.NgramLm.from_arrays(alpha=ALPHA, beta=BETA, **_table("awkward"))
    plain, full = NL.RnntTdtBeamStream(tdt, B, W, ML), NL.RnntTdtBeamStream(tdt, B, W, ML, **kw)
    enc, first = _t(gpu, c["enc"]), _chunk(c, c["enc"], 0, 4)
    for s in (plain, full):
        s.push(_t(gpu, first[0]), first[1], NB)
    nl = B * NB * ML
    buf, sc = torch.full((4 * nl + B * NB,), 7, dtype=torch.int32, device=gpu), torch.full((B * NB,), 7.0, device=gpu)
    lab, fr, du, lp, ln = [buf[i * nl:(i + 1) * nl] for i in range(4)] + [buf[4 * nl:]]
    o = lambda lm=None, norm=0, fr=None: capi.NntkRnntTdtBeamOptions(lm, norm, fr, None, None)
    ws = torch.full((L.nntk_rnnt_tdt_beam_opt_workspace_floats(tdt.h, B, W, ML, C.byref(o(lm.h, 1))) + 8,), 7.0, device=gpu)
    on, big = o(lm.h, 1, fr.data_ptr()), 2 ** 31 - 1 - 16
    bad = [(tdt2, plain, B, T, None, NB, o(), "another decoder"), (tdt, plain, B - 1, T, None, NB, o(), "batch"),
           (tdt, plain, B, T, None, NB, o(lm.h), "without a language model"), (tdt, full, B, T, None, NB, o(None, 1), "with a language model"),
           (tdt, full, B, T, None, NB, o(lm2.h, 1), "another language model"), (tdt, plain, B, T, None, NB, o(norm=1), "without detail"),
           (tdt, plain, B, T, None, NB, o(fr=fr.data_ptr()), "without detail"), (tdt, full, B, T, None, NB, o(lm.h), "with detail"),
           (tdt, full, B, T, None, W + 1, on, "nbest"), (tdt, full, B, T, None, NB, o(lm.h, 2), "length_norm"),
           (tdt, full, B, T, [T + 1, 0, 0], NB, on, "n_frames"), (classic, plain, B, T, None, NB, o(), "nntk_rnnt_beam_decode_device"),
           (tdt, None, B, T, None, NB, o(), "NULL state"), (tdt, full, B, big, [big, 0, 0], NB, on, "INT_MAX - 16")]
    for dec, s, b, t, n, nbest, opt, word in bad:
        rc = L.nntk_rnnt_tdt_beam_stream_push_device(dec.h, s.h if s else None, _p(enc), b, t, _ip(n) if n else None, nbest, C.byref(opt),
                                                     _p(lab), _p(ln), _p(sc), _p(ws))
        torch.cuda.synchronize()
        assert rc == -1 and word in capi.last_error() and (buf == 7).all() and (sc == 7.0).all() and (ws == 7.0).all(), (word, capi.last_error())
    rest = _chunk(c, c["enc"], 4, 6)
    ask = lambda with_lm, dt: L.nntk_rnnt_tdt_beam_opt_workspace_floats(tdt.h, B, W, ML, C.byref(o(lm.h if with_lm else None, dt)))
    for with_lm, dt in ((0, 0), (1, 0), (0, 1), (1, 1)):                             # J 22, Dmax 3: the row block, 4 counts, 44 held floats, 2 host ints
        assert L.nntk_rnnt_tdt_beam_state_bytes(tdt.h, B, W, ML, with_lm, dt) == 4 * (ask(with_lm, dt) - 4 - 8 + B * (4 + 44)) + 8 * B
    assert [L.nntk_rnnt_tdt_beam_state_bytes(*a, 0, 0) for a in ((classic.h, B, W, ML), (tdt.h, 0, W, ML), (tdt.h, B, 33, ML), (tdt.h, B, W, 0))] == [0] * 4
    assert not L.nntk_rnnt_tdt_beam_state_create(classic.h, B, W, ML, None, 0) and "nntk_rnnt_beam_state_create" in capi.last_error()
    for s, k in ((plain, {}), (full, kw)):                                           # the streams go on as if nothing had been asked
        assert _same(_host(s.push(_t(gpu, rest[0]), rest[1], NB)), _one_shot(gpu, tdt, c, 10, k))
        s.close()
    tdt.destroy(); tdt2.destroy(); classic.destroy()
