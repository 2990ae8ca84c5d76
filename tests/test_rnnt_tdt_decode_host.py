"""The host side of token-and-duration greedy decoding (csrc/host/rnnt_decode.c): the duration table's refusals, made before anything is
allocated or any pointer looked at, and the float64 reference of the device tests (tests/rnnt_tdt_decode_reference.py) against a case
worked by hand.  The refusals that need a live handle are in tests/test_gpu_rnnt_tdt_decode.py.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import rnnt_tdt_decode_reference as R
from nntoolkitcore_amd import capi


def test_reference_agrees_with_a_hand_worked_two_frame_case():
    """The hand-worked model of test_rnnt_decode_host.py (V = 2, blank 0, E = H = J = 1, identity joiner; token scores (-z, z), z = enc +
    h) with durations (0, 2) scored (z, -z): a label (z > 0) prefers duration 0, a blank (z < 0) would prefer 2 anyway."""
    sig2 = lambda z: abs(z) - math.log(math.exp(z) + math.exp(-z))          # the winner's log-probability in a head scored (z, -z)
    c = 0.5 * math.tanh(0.5)
    h = 0.5 * math.tanh(c)
    z0 = 0.15 + h                                                           # frame 0: label 1 with duration 0
    c = 0.5 * c + 0.5 * math.tanh(-3.0 + 0.5)
    h = 0.5 * math.tanh(c)
    z1 = 0.15 + h                                                           # frame 0 again: z < 0, blank, duration 2: lands on n = 2
    assert z0 > 0 and -0.04 < z1 < -0.02
    embed = np.array([[0.0], [1.0]])
    lstm = np.array([0, 0, -3.0, 0, 0, 0, 0, 0, 0, 0, 0.5, 0, 0, 0, 0, 0])
    out = np.array([-1.0, 1.0, 1.0, -1.0, 0, 0, 0, 0])
    enc = np.array([[[0.15], [np.nan]]])                                    # frame 1 is jumped over
    kw = dict(blank=0, activation="identity", max_symbols_per_frame=5)
    r = R.greedy_decode(embed, lstm, None, out, enc, (0, 2), **kw)
    assert r["labels"] == [[1]] and r["frames"] == [[0]] and r["durations"] == [[0]] and r["cells"] == [[(0, 0), (0, 1)]]
    assert abs(r["scores"][0] - 2 * (sig2(z0) + sig2(z1))) < 1e-14 and abs(r["gaps"][0] - 2 * abs(z1)) < 1e-14
    assert (r["label_zero"][0], r["blank_zero"][0], r["capped"][0], r["skipped"][0], r["ends_exact"][0]) == (1, 0, 0, 1, True)
    # durations (0, 1) scored (-z, z): the blank's unrestricted winner is 0, it takes 1 and pays for it; frame 1 (z < 0) is a blank too
    out01 = np.array([-1.0, 1.0, -1.0, 1.0, 0, 0, 0, 0])
    enc2 = np.array([[[0.15], [-0.5]]])
    r = R.greedy_decode(embed, lstm, None, out01, enc2, (0, 1), **kw)
    z2 = -0.5 + h
    lose = lambda z: -abs(z) - math.log(math.exp(z) + math.exp(-z))
    assert r["labels"] == [[1]] and r["durations"] == [[1]] and r["cells"] == [[(0, 0), (1, 1)]] and r["blank_zero"][0] == 1
    assert abs(r["scores"][0] - (2 * sig2(z0) + sig2(z2) + lose(z2))) < 1e-14
    assert abs(r["gaps"][0] - 2 * min(z0, -z2)) < 1e-14                      # a blank's only positive duration has no runner-up
    # the cap at one symbol a frame moves on unscored and the recorded duration stays 0
    r = R.greedy_decode(embed, lstm, None, out, enc2, (0, 2), blank=0, activation="identity", max_symbols_per_frame=1)
    assert r["durations"] == [[0]] and r["cells"] == [[(0, 0), (1, 1)]] and r["capped"][0] == 1 and not r["ends_exact"][0]
    # the lattice's scores at the decoder's cells are the decoder's scores
    x = R.lattice_scores(embed, lstm, None, out, enc2, 2, [[1]], blank=0, activation="identity")
    assert x.shape == (1, 2, 2, 4) and np.allclose(x[0, 0, 1], [-z1, z1, z1, -z1], atol=1e-14)


BAD = [("empty", [], 0, "n_durations"), ("nine", list(range(9)), 9, "n_durations"), ("descending", [2, 1], 2, "ascending"),
       ("repeated", [1, 1], 2, "ascending"), ("negative", [-1, 1], 2, "negative"), ("all zero", [0], 1, "positive"),
       ("above 16", [1, 17], 2, "more than"), ("NULL", None, 3, "NULL durations")]


@pytest.mark.parametrize("name,durs,n,word", BAD, ids=[b[0] for b in BAD])
def test_create_rejects_the_durations_before_touching_a_device(name, durs, n, word):
    """dummy device pointers: a create that got past the checks would fault or need a device, a refusal never looks at them"""
    cfg = capi.NntkRnntDecoderConfig(5, 0, 7, 12, 20, 1, 3)
    d = None if durs is None else np.asarray(durs + [0], np.int32).ctypes.data_as(capi.ip)
    h = capi.load().nntk_rnnt_tdt_decoder_create(cfg, d, n, C.c_void_p(0x10000), C.c_void_p(0x20000), C.c_void_p(0x30000), C.c_void_p(0x40000))
    assert not h and word in capi.last_error(), (name, capi.last_error())
