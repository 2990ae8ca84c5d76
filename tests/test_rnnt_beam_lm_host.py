"""The host side of the fused transducer beam search (csrc/host/rnnt_decode.c, the nntk_rnnt_beam_*_lm functions; csrc/host/ngram_lm.c):
the exported symbols, the refusals and sizes that need no device, the float64 reference of the device tests
(tests/rnnt_beam_reference.py with a model) against the acoustic reference and the lattice, and the premises of every case of
tests/test_gpu_rnnt_beam_lm.py (tests/rnnt_beam_lm_cases.py).  The refusals that need a live decoder or state are in the GPU file.
No GPU."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import rnnt_beam_lm_cases as K
import rnnt_beam_reference as RB
import rnnt_reference as RR
from nntoolkitcore_amd import capi, layers as NL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["nntk_rnnt_beam_decode_lm_device", "nntk_rnnt_beam_decode_lm", "nntk_rnnt_beam_lm_workspace_floats",
         "nntk_rnnt_beam_state_create_lm", "nntk_rnnt_beam_state_bytes_lm", "nntk_ngram_lm_rnnt_device_bytes"]


def test_symbols_are_declared_bound_and_exported():
    L = capi.load()
    header = open(os.path.join(ROOT, "include", "nntoolkitcore_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in capi.SIGNATURES and getattr(L, name).argtypes == capi.SIGNATURES[name][1], name


def test_refusals_and_sizes_that_need_no_device():
    L = capi.load()
    t, alpha, beta = K.table("awkward")
    lm = NL.NgramLm.from_arrays(alpha=alpha, beta=beta, **t)
    na, ns = len(t["arc_label"]), len(t["backoff_state"])
    assert L.nntk_ngram_lm_rnnt_device_bytes(lm.h) == 8 * na + 16 * ns == lm.rnnt_device_bytes()
    assert L.nntk_ngram_lm_device_bytes(lm.h) == 16 * (na + 2 * ns) and L.nntk_ngram_lm_rnnt_device_bytes(None) == 0
    out = np.full(64, 7, np.int32)
    sc = np.full(4, 7.0, np.float32)
    enc = np.zeros(2 * 3 * 4, np.float32)
    ip, fp = out.ctypes.data_as(capi.ip), sc.ctypes.data_as(capi.fp)
    n = np.array([3, 3], np.int32).ctypes.data_as(capi.ip)
    p = C.c_void_p
    for h in (None, lm.h):
        assert L.nntk_rnnt_beam_decode_lm(None, None, enc.ctypes.data_as(capi.fp), 2, 3, n, 4, 2, 4, h, ip, ip, fp) == -1
        assert "NULL decoder" in capi.last_error() and capi.last_error().startswith("nntk_rnnt_beam_decode_lm:")
        assert L.nntk_rnnt_beam_decode_lm_device(None, None, p(0x1000), 2, 3, n, 4, 2, 4, h, p(0x2000), p(0x3000), p(0x4000), p(0x5000)) == -1
        assert "NULL decoder" in capi.last_error() and capi.last_error().startswith("nntk_rnnt_beam_decode_lm_device:")
        assert not L.nntk_rnnt_beam_state_create_lm(None, 2, 4, 4, h) and "NULL decoder" in capi.last_error()
    assert L.nntk_rnnt_beam_lm_workspace_floats(None, 2, 4, 4) == 0 and L.nntk_rnnt_beam_state_bytes_lm(None, 2, 4, 4) == 0
    assert (out == 7).all() and (sc == 7.0).all()
    lm.close()


def test_shim_workspace_appends_to_the_acoustic_layout():
    """per row one int per hypothesis slot and beam_width V doubles more, each part rounded up to 16 bytes; the acoustic size is untouched"""
    L = capi.load()
    size = L.nntk_shim_rnnt_beam_workspace_floats
    size.restype, size.argtypes = C.c_size_t, [C.c_int] * 9
    f, g = lambda *a: size(*a, 0, 0), lambda *a: size(*a, 1, 0)            # without and with a model, no detail
    pad = lambda x: (x + 3) & ~3
    for batch, H, J, V, S, W, ML in [(2, 12, 20, 5, 3, 4, 6), (3, 13, 22, 1030, 1, 3, 4), (1, 16, 16, 70, 3, 8, 2), (5, 7, 9, 6, 4, 32, 3)]:
        slots = (min(S, ML) + 2) * W
        assert g(batch, H, J, V, S, W, ML) == f(batch, H, J, V, S, W, ML) + batch * (pad(slots) + pad(2 * W * V)), (batch, H, J, V, S, W, ML)
    assert g(0, 12, 20, 5, 3, 4, 6) == 0


def test_the_model_in_python_equals_the_host_scorer():
    for name in ("awkward", "big_v", "stream", "exhaustive4"):
        t, alpha, beta = K.table(name)
        lm, ref = NL.NgramLm.from_arrays(alpha=alpha, beta=beta, **t), RB.Lm(t, alpha, beta)
        labels = [v for v in range(t["n_classes"]) if v != t["blank"]]
        rng = np.random.default_rng(3)
        for _ in range(20):
            y = rng.choice(labels, int(rng.integers(0, 6))).tolist()
            for wf in (False, True):
                assert lm.score(y, with_final=wf) == ref.score(y, with_final=wf), (name, y, wf)
        lm.close()


@pytest.mark.parametrize("name", ["awkward", "awkward_w3", "wide_identity", "stream", "tie"])
def test_a_unit_model_leaves_the_acoustic_reference_exactly(name):
    c = K.case(name)
    m = c["m"]
    t = dict(K.table("awkward" if m["V"] == 5 else name)[0], final_logp=None)
    for dtype in (np.float64, np.float32):
        got = RB.beam_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], lm=RB.Lm(t, 0.0, 0.0), dtype=dtype, **K.search_kw(c))
        want = RB.beam_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], dtype=dtype, **K.search_kw(c))
        for key in ("labels", "scores", "final"):
            assert got[key] == want[key], (name, key)
        for key in ("cut_gap", "order_gap", "merges", "cuts", "at_max", "max_b"):
            assert np.array_equal(got[key], want[key]), (name, key)


@pytest.mark.parametrize("name", ["exhaustive3", "exhaustive4"])
def test_exhaustive_search_minus_the_model_is_the_lattice(name):
    """nothing is cut, every sequence of at most 2 labels is reported, and score - (the model's walk with the end-of-sentence term) is
    the lattice log-likelihood of tests/rnnt_reference.py"""
    r64, _, lm = K.reference(name)
    c = K.case(name)
    m = c["m"]
    assert r64["cuts"].sum() == 0
    lab = [v for v in range(m["V"]) if v != m["blank"]]
    want = sorted([()] + [(a,) for a in lab] + list(itertools.product(lab, lab)))
    assert lm.unk > 0 and lm.backoffs > 0
    for b, n in enumerate(c["n"]):
        assert sorted(tuple(r[0]) for r in r64["final"][b]) == want
        for y, s, _, _ in r64["final"][b]:
            logits = RB.lattice_logits(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"][b, :n], y, blank=m["blank"], activation=c["act"])
            loss, _ = RR.rnnt_loss_and_grad(logits[None], [y], [n], m["blank"])
            # float64 throughout: a few dozen additions of terms below 32 in magnitude, 2^-53 * 32 * 50 < 2e-13
            assert abs((s - lm.score(y, with_final=True)) + loss[0]) < 1e-12, (b, y, s, loss[0])


@pytest.mark.parametrize("name", K.GAP_CASES)
def test_case_premises(name):
    K.assert_premise(name)


def test_premises_of_the_special_cases():
    # the model decides: the best hypothesis of some row differs with and without it
    a, r = K.acoustic_reference("decides"), K.reference("decides")[0]
    assert any(a["labels"][b][0] != r["labels"][b][0] for b in range(2))
    # zero-mass arcs: the acoustic-and-model best of row 0 takes them; with them at zero mass no hypothesis does, and terms of -inf were met
    t = K.table("awkward")[0]
    pairs = {(t["arc_label"][q], q) for q in K.zero_arcs()}
    assert pairs and K.reference("zero_arc")[2].dead > 0
    assert K.reference("zero_arc")[0]["labels"][0][0] != K.reference("awkward")[0]["labels"][0][0]
    # end of sentence at -inf: the best hypothesis of row 0 leaves the report, and stays in the carried beam
    best = K.reference("awkward")[0]["labels"][0][0]
    r = K.reference("final_drop")[0]
    assert best not in [r4[0] for r4 in r["final"][0]] and best in [y for y, _, _ in r["carried"][0]]
    # end of sentence reorders, ties to the lower rank in A: [1] and [3] tie before and after, the empty hypothesis overtakes both
    r = K.reference("final_tie")[0]
    assert [y for y, _, _ in r["carried"][0]][:3] == [[1], [3], []] and r["carried"][0][0][1] == r["carried"][0][1][1]
    assert r["labels"][0] == [[], [1], [3]] and r["scores"][0][1] == r["scores"][0][2]
    assert K.f32_error("final_tie") >= 0 and K.score_tol() > 0
