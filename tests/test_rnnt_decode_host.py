"""The host side of greedy transducer decoding (csrc/host/rnnt_decode.c): every refusal that can be provoked without a device -- the
configuration, the weight pointers and the NULL handles, each -1 / NULL with a message and nothing touched -- and the float64 reference
of the device tests (tests/rnnt_decode_reference.py) against a case worked by hand.  The refusals of a decode call that need a live
decoder or state (a decoder copies its weights on the device when it is created) are in tests/test_gpu_rnnt_decode.py.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import rnnt_decode_reference as R
from nntoolkitcore_amd import capi


def test_reference_agrees_with_a_hand_worked_two_frame_case():
    """V = 2 (blank 0), E = H = J = 1, identity joiner, no projection; W_out = [-1, 1], so the logits are (-z, z), z = enc + h.
    Only the candidate gate sees the input: W = (0, 0, -3, 0), U = 0, b_i = (0, 0, 0.5, 0), b_h = 0; embed = (0, 1)."""
    sig = lambda x: 1.0 / (1.0 + math.exp(-x))
    lp = lambda z: abs(z) - math.log(math.exp(z) + math.exp(-z))             # the winner's log-probability
    # the start step on embed[blank] = 0 from the zero state: i = f = o = 1/2, g = tanh(0.5)
    c = 0.5 * math.tanh(0.5)
    h = 0.5 * math.tanh(c)
    assert abs(h - 0.11351) < 1e-5
    z0 = 0.15 + h                                                           # frame 0: z > 0, label 1
    assert z0 > 0
    c = 0.5 * c + 0.5 * math.tanh(-3.0 + 0.5)                               # the step on embed[1] = 1
    h = 0.5 * math.tanh(c)
    z1 = 0.15 + h                                                           # frame 0 again: z < 0, blank
    assert -0.04 < z1 < -0.02
    z2 = -0.5 + h                                                           # frame 1: blank
    want = lp(z0) + lp(z1) + lp(z2)
    embed = np.array([[0.0], [1.0]])
    lstm = np.array([0, 0, -3.0, 0, 0, 0, 0, 0, 0, 0, 0.5, 0, 0, 0, 0, 0])
    out = np.array([-1.0, 1.0, 0, 0])
    enc = np.array([[[0.15], [-0.5]]])
    r = R.greedy_decode(embed, lstm, None, out, enc, blank=0, activation="identity", max_symbols_per_frame=5)
    assert r["labels"] == [[1]] and r["frames"] == [[0]] and r["cells"] == [[(0, 0), (0, 1), (1, 1)]]
    assert abs(r["scores"][0] - want) < 1e-14 and abs(r["gaps"][0] - 2 * abs(z1)) < 1e-14
    assert r["capped"][0] == 0 and not r["ends_on_label"][0]
    # the cap at one symbol a frame: the label moves on without a blank, the second decision is made at frame 1
    r1 = R.greedy_decode(embed, lstm, None, out, enc, blank=0, activation="identity", max_symbols_per_frame=1)
    assert r1["labels"] == [[1]] and r1["cells"] == [[(0, 0), (1, 1)]] and r1["capped"][0] == 1
    assert abs(r1["scores"][0] - (lp(z0) + lp(z2))) < 1e-14
    # max_labels: the row stops for good
    r2 = R.greedy_decode(embed, lstm, None, out, enc, blank=0, activation="identity", max_symbols_per_frame=5, max_labels=1)
    assert r2["labels"] == [[1]] and r2["cells"] == [[(0, 0)]] and r2["ends_on_label"][0] and abs(r2["scores"][0] - lp(z0)) < 1e-14
    # the float32 restatement decodes the same and scores within float32 rounding
    r32 = R.greedy_decode(embed, lstm, None, out, enc, blank=0, activation="identity", max_symbols_per_frame=5, dtype=np.float32)
    assert r32["labels"] == r["labels"] and r32["scores"].dtype == np.float32 and abs(float(r32["scores"][0]) - want) < 1e-6


GOOD = dict(V=5, blank=0, E=7, H=12, J=20, act=1, ms=3, embed=0x10000, lstm=0x20000, proj=0x30000, out=0x40000)
BAD = [("V = 1", dict(V=1), "V 1"), ("V above the limit", dict(V=8193), "limit"), ("blank = V", dict(blank=5), "blank"),
       ("blank < 0", dict(blank=-1), "blank"), ("E = 0", dict(E=0), "at least 1"), ("H = 0", dict(H=0), "at least 1"),
       ("J < 0", dict(J=-2), "at least 1"), ("E above the limit", dict(E=1025), "limit"), ("H above the limit", dict(H=1025), "limit"),
       ("J above the limit", dict(J=1025), "limit"), ("no projection with H != J", dict(proj=None), "H 12 != J 20"),
       ("activation 3", dict(act=3), "joint_activation"), ("activation -1", dict(act=-1), "joint_activation"),
       ("max_symbols_per_frame 0", dict(ms=0), "max_symbols_per_frame"), ("NULL embed", dict(embed=None), "NULL"),
       ("NULL lstm", dict(lstm=None), "NULL"), ("NULL out", dict(out=None), "NULL"), ("misaligned embed", dict(embed=0x10002), "aligned"),
       ("misaligned lstm", dict(lstm=0x20001), "aligned"), ("misaligned projection", dict(proj=0x30002), "aligned"),
       ("misaligned out", dict(out=0x40003), "aligned")]


@pytest.mark.parametrize("name,change,word", BAD, ids=[b[0] for b in BAD])
def test_create_rejects_before_touching_a_device(name, change, word):
    """dummy device pointers: a create that got past the checks would fault or need a device, a refusal never looks at them"""
    a = dict(GOOD, **change)
    p = lambda v: None if v is None else C.c_void_p(v)
    cfg = capi.NntkRnntDecoderConfig(a["V"], a["blank"], a["E"], a["H"], a["J"], a["act"], a["ms"])
    h = capi.load().nntk_rnnt_decoder_create(cfg, p(a["embed"]), p(a["lstm"]), p(a["proj"]), p(a["out"]))
    assert not h and word in capi.last_error(), (name, capi.last_error())


def test_the_limits_admit_the_documented_sizes():
    """E = H = J = 1024, V = 8192 and every size from 1 up pass the configuration checks: the refusal that follows is about a pointer"""
    L = capi.load()
    for V, E, H, J in ((8192, 1024, 1024, 1024), (2, 1, 1, 1), (3, 1, 2, 2), (1000, 63, 65, 129)):
        cfg = capi.NntkRnntDecoderConfig(V, V - 1, E, H, J, 2, 1)
        assert not L.nntk_rnnt_decoder_create(cfg, None, None, None, None) and "d_embed is NULL" in capi.last_error(), (V, E, H, J)


def test_null_handles_are_refused_and_write_nothing():
    L = capi.load()
    out = np.full(16, 7, np.int32)
    sc = np.full(2, 7.0, np.float32)
    enc = np.zeros(2 * 3 * 4, np.float32)
    ip, fp = out.ctypes.data_as(capi.ip), sc.ctypes.data_as(capi.fp)
    n = np.array([3, 3], np.int32).ctypes.data_as(capi.ip)
    assert L.nntk_rnnt_greedy_decode(None, None, enc.ctypes.data_as(capi.fp), 2, 3, n, 4, ip, None, ip, fp) == -1
    assert "NULL decoder" in capi.last_error()
    assert L.nntk_rnnt_greedy_decode_device(None, None, C.c_void_p(0x1000), 2, 3, n, 4, C.c_void_p(0x2000), None, C.c_void_p(0x3000), None) == -1
    assert "NULL decoder" in capi.last_error()
    assert L.nntk_rnnt_decoder_load_weights_device(None, C.c_void_p(0x1000), C.c_void_p(0x2000), None, C.c_void_p(0x3000)) == -1
    assert "NULL" in capi.last_error()
    assert not L.nntk_rnnt_decode_state_create(None, 2) and "NULL decoder" in capi.last_error()
    assert L.nntk_rnnt_decode_state_reset(None, None, 0) == -1 and "NULL state" in capi.last_error()
    L.nntk_rnnt_decoder_destroy(None)
    L.nntk_rnnt_decode_state_destroy(None)
    assert (out == 7).all() and (sc == 7.0).all()
