"""The host side of transducer beam search (csrc/host/rnnt_decode.c, the nntk_rnnt_beam_* functions): the refusals that can be provoked
without a device, the size functions, the exported symbols, and the float64 reference of the device tests
(tests/rnnt_beam_reference.py) against the transducer loss of tests/rnnt_reference.py.  The refusals that need a live decoder or state
(a decoder copies its weights on the device when it is created) are in tests/test_gpu_rnnt_beam.py.  No GPU."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np

import rnnt_beam_reference as RB
import rnnt_reference as RR
from nntoolkitcore_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["nntk_rnnt_beam_workspace_floats", "nntk_rnnt_beam_decode_device", "nntk_rnnt_beam_decode", "nntk_rnnt_beam_state_create",
         "nntk_rnnt_beam_state_bytes", "nntk_rnnt_beam_state_reset", "nntk_rnnt_beam_state_destroy"]


def test_symbols_are_declared_bound_and_exported():
    L = capi.load()
    header = open(os.path.join(ROOT, "include", "nntoolkitcore_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in capi.SIGNATURES and getattr(L, name).argtypes == capi.SIGNATURES[name][1], name
    assert "RNN-Transducer: beam search" in header


def test_null_handles_are_refused_and_write_nothing():
    L = capi.load()
    out = np.full(64, 7, np.int32)
    sc = np.full(4, 7.0, np.float32)
    enc = np.zeros(2 * 3 * 4, np.float32)
    ip, fp = out.ctypes.data_as(capi.ip), sc.ctypes.data_as(capi.fp)
    n = np.array([3, 3], np.int32).ctypes.data_as(capi.ip)
    assert L.nntk_rnnt_beam_decode(None, None, enc.ctypes.data_as(capi.fp), 2, 3, n, 4, 2, 4, ip, ip, fp) == -1
    assert "NULL decoder" in capi.last_error()
    p = C.c_void_p
    assert L.nntk_rnnt_beam_decode_device(None, None, p(0x1000), 2, 3, n, 4, 2, 4, p(0x2000), p(0x3000), p(0x4000), p(0x5000)) == -1
    assert "NULL decoder" in capi.last_error()
    assert not L.nntk_rnnt_beam_state_create(None, 2, 4, 4) and "NULL decoder" in capi.last_error()
    assert L.nntk_rnnt_beam_state_reset(None, None, 0) == -1 and "NULL state" in capi.last_error()
    L.nntk_rnnt_beam_state_destroy(None)
    assert (out == 7).all() and (sc == 7.0).all()


def test_size_functions_without_a_decoder_are_zero():
    """the sizes depend on the decoder's widths: without one, or for an empty batch, nothing is needed (the monotonicity in each
    argument needs a live decoder: tests/test_gpu_rnnt_beam.py)"""
    L = capi.load()
    assert L.nntk_rnnt_beam_workspace_floats(None, 2, 4, 4) == 0 and L.nntk_rnnt_beam_state_bytes(None, 2, 4, 4) == 0
    assert L.nntk_rnnt_beam_workspace_floats(None, 0, 4, 4) == 0 and L.nntk_rnnt_beam_state_bytes(None, -1, 4, 4) == 0


def test_shim_workspace_is_monotone_in_each_argument_and_zero_for_an_empty_batch():
    size = capi.load().nntk_shim_rnnt_beam_workspace_floats
    size.restype, size.argtypes = C.c_size_t, [C.c_int] * 9
    f = lambda *a: size(*a, 0, 0)                                          # no model, no detail: the acoustic part alone
    base = dict(batch=2, H=12, J=20, V=5, S=3, W=4, ML=6)
    order = ("batch", "H", "J", "V", "S", "W", "ML")
    v0 = f(*(base[k] for k in order))
    assert v0 > 0 and v0 % 4 == 0
    for k in order:
        prev = v0
        for step in (1, 2, 5):
            v = f(*(dict(base, **{k: base[k] + step})[x] for x in order))
            assert v >= prev and v % 4 == 0, (k, step)
            prev = v
        assert prev > v0 or k == "S", k                                    # (S above max_labels adds no level)
    assert f(*(dict(base, S=9)[x] for x in order)) == f(*(dict(base, S=6)[x] for x in order))      # S' = min(S, max_labels)
    assert f(0, 12, 20, 5, 3, 4, 6) == 0 and f(-3, 12, 20, 5, 3, 4, 6) == 0


def test_group_override_and_lds_limit():
    L = capi.load()
    grp, fits = L.nntk_shim_rnnt_beam_group, L.nntk_shim_rnnt_beam_fits
    assert grp(8, 12, 20, 5) == 4 and grp(1, 12, 20, 5) == 1
    assert fits(1024, 1024, 8192) and grp(8, 1024, 1024, 8192) == 1           # the limits fit one hypothesis a pass, not four
    L.nntk_shim_rnnt_beam_set_group(1)
    assert grp(8, 12, 20, 5) == 1
    L.nntk_shim_rnnt_beam_set_group(4)
    assert grp(1, 12, 20, 5) == 4 and grp(8, 1024, 1024, 8192) == 1
    L.nntk_shim_rnnt_beam_set_group(0)
    assert grp(8, 12, 20, 5) == 4


def _tiny(seed, blank):
    rng = np.random.default_rng(seed)
    V, E, H, J = 3, 2, 3, 4
    u = lambda sc, *s: rng.uniform(-sc, sc, s)
    G = 4 * H
    return dict(V=V, E=E, H=H, J=J, blank=blank, embed=u(1.0, V, E),
                lstm=np.concatenate([u(1.5, E * G), u(1.0, H * G), u(0.1, G), u(0.1, G)]),
                proj=np.concatenate([u(1.0, H * J), u(0.1, J)]), out=np.concatenate([u(1.5, J * V), u(0.1, V)]),
                enc=u(1.5, 2, 4, J))


def test_reference_with_nothing_pruned_reproduces_the_transducer_loss():
    """V = 3, at most 2 labels, S = 2, W = 8: the 7 sequences all survive, nothing is ever cut, and each final score is minus the
    transducer loss of that sequence on the lattice built from the same model (tests/rnnt_reference.py, and by enumeration)"""
    for blank in (0, 2):
        m = _tiny(5 + blank, blank)
        n = [4, 2]
        kw = dict(blank=blank, activation="tanh")
        r = RB.beam_decode(m["embed"], m["lstm"], m["proj"], m["out"], m["enc"], n_frames=n, max_symbols_per_frame=2, beam_width=8,
                           nbest=8, max_labels=2, **kw)
        labels = [v for v in range(3) if v != blank]
        want = sorted([()] + [(a,) for a in labels] + list(itertools.product(labels, labels)))
        for b in range(2):
            assert sorted(tuple(l) for l in r["labels"][b]) == want and r["cuts"][b] == 0 and r["cut_gap"][b] == math.inf
            assert r["merges"][b] > 0 and r["at_max"][b] > 0
            total = 0.0
            for y, s in zip(r["labels"][b], r["scores"][b]):
                lg = RB.lattice_logits(m["embed"], m["lstm"], m["proj"], m["out"], m["enc"][b, :n[b]], y, **kw)
                loss, _ = RR.rnnt_loss_and_grad(lg[None], [y], [n[b]], blank)
                assert abs(-loss[0] - s) < 1e-12, (blank, b, y, loss[0], s)
                assert abs(RR.brute_force_loss(lg, y, blank) + s) < 1e-12
                total += math.exp(s)
            assert total <= 1.0 + 1e-12
            assert r["scores"][b] == sorted(r["scores"][b], reverse=True)
        r32 = RB.beam_decode(m["embed"], m["lstm"], m["proj"], m["out"], m["enc"], n_frames=n, max_symbols_per_frame=2, beam_width=8,
                             nbest=8, max_labels=2, dtype=np.float32, **kw)
        assert r32["labels"] == r["labels"]
        assert max(abs(float(x) - y) for b in range(2) for x, y in zip(r32["scores"][b], r["scores"][b])) < 1e-5


def test_reference_prunes_and_breaks_ties_as_the_contract_says():
    """W_out = 0: the logits are the bias whatever the state, labels 1 and 3 share a bias.  W = 2: at depth 0 the cells (0, 1) and (0, 3)
    tie and are kept in that order; B's tie between (1,) and (3,) goes to the earlier insertion."""
    m = _tiny(1, 0)
    V, J = 5, m["J"]
    rng = np.random.default_rng(2)
    embed = rng.uniform(-1, 1, (V, m["E"]))
    out = np.concatenate([np.zeros(J * V), [0.5, 0.25, -1.0, 0.25, -2.0]])
    r = RB.beam_decode(embed, m["lstm"], m["proj"], out, m["enc"][:1, :2], max_symbols_per_frame=1, beam_width=2, nbest=2, max_labels=4)
    assert r["labels"][0][0] == [] and r["labels"][0][1] == [1] and r["cut_gap"][0] == 0.0 and r["cuts"][0] > 0
    r3 = RB.beam_decode(embed, m["lstm"], m["proj"], out, m["enc"][:1, :2], max_symbols_per_frame=1, beam_width=3, nbest=3, max_labels=4)
    assert r3["labels"][0] == [[], [1], [3]] and r3["scores"][0][1] == r3["scores"][0][2]
