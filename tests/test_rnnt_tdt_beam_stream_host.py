"""The host side of the streamed token-and-duration beam search (csrc/host/rnnt_decode.c): the names are declared with the bound argument
lists, and what can be refused without a decoder is refused and writes nothing.  The sizes need a decoder: the GPU file.  No GPU."""
import ctypes as C, os, re

import numpy as np

from nntoolkitcore_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = {"nntk_rnnt_tdt_beam_state_create": 6, "nntk_rnnt_tdt_beam_state_bytes": 6, "nntk_rnnt_tdt_beam_state_reset": 3,
        "nntk_rnnt_tdt_beam_state_destroy": 1, "nntk_rnnt_tdt_beam_stream_push_device": 12, "nntk_rnnt_tdt_beam_stream_push": 11}


def test_names_are_declared_with_the_bound_argument_lists():
    L = capi.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nntoolkitcore_hip.h")).read(), flags=re.S)
    for name, count in ARGS.items():
        declared = re.search(r"\b" + name + r"\s*\(([^;{]*)\)\s*;", header)
        assert declared and len(declared.group(1).split(",")) == count == len(capi.SIGNATURES[name][1]), name
        assert getattr(L, name).argtypes == capi.SIGNATURES[name][1], name
    assert "typedef struct NntkRnntTdtBeamStateStruct *NntkRnntTdtBeamState;" in header


def test_without_a_decoder_everything_is_refused_and_nothing_written():
    L = capi.load()
    out, sc, enc = np.full(64, 7, np.int32), np.full(4, 7.0, np.float32), np.zeros(2 * 3 * 4, np.float32)
    ip, fp, p = out.ctypes.data_as(capi.ip), sc.ctypes.data_as(capi.fp), C.c_void_p
    n = np.array([3, 3], np.int32).ctypes.data_as(capi.ip)
    assert L.nntk_rnnt_tdt_beam_stream_push(None, None, enc.ctypes.data_as(capi.fp), 2, 3, n, 1, None, ip, ip, fp) == -1
    assert capi.last_error().startswith("nntk_rnnt_tdt_beam_stream_push:") and "NULL decoder" in capi.last_error()
    assert L.nntk_rnnt_tdt_beam_stream_push_device(None, None, p(0x1000), 2, 3, n, 1, None, p(0x2000), p(0x3000), p(0x4000), p(0x5000)) == -1
    assert capi.last_error().startswith("nntk_rnnt_tdt_beam_stream_push_device:") and "NULL decoder" in capi.last_error()
    assert not L.nntk_rnnt_tdt_beam_state_create(None, 2, 4, 4, None, 0) and "NULL decoder" in capi.last_error()
    assert L.nntk_rnnt_tdt_beam_state_reset(None, None, 0) == -1 and "NULL state" in capi.last_error()
    assert all(L.nntk_rnnt_tdt_beam_state_bytes(None, 2, 4, 4, lm, detail) == 0 for lm in (0, 1) for detail in (0, 1))
    L.nntk_rnnt_tdt_beam_state_destroy(None)
    assert (out == 7).all() and (sc == 7.0).all()
