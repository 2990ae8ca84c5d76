"""The host side of token-and-duration forced alignment (csrc/host/rnnt.c) and the premises of tests/test_gpu_rnnt_tdt_align.py: the
float64 reference (tests/rnnt_tdt_align_reference.py) pinned to enumeration of every path, tie-break included; every row of the device
cases clear of the gap threshold, and without a path where the case says so; the entry's refusals.  No GPU."""
import math

import numpy as np
import pytest

import rnnt_cases as K
import rnnt_tdt_align_reference as A
from nntoolkitcore_amd import capi

GPU_CASES = ["ragged_5_0_0", "ragged_64_63_0", "ragged_257_100_0", "ragged_5_2_0.05", "d12", "d12_short", "d02", "d018", "underflow",
             "U300", "U512", "long", "blocks"]
ARRAYS = ["label_frames", "label_durations", "frame_labels", "frame_durations", "label_logp", "frame_logp"]


@pytest.mark.parametrize("name", ["d12", "d02", "d12_short", "flat"])
def test_reference_equals_enumeration(name):
    c = A.case(name)
    for b, (r, e) in enumerate(zip(A.reference(name)[0], A.rows(c, fn=A.enumerate_row))):
        assert r["score"] == e["score"] and all(np.array_equal(r[k], e[k]) for k in ARRAYS), (name, b)
        assert (r["score"] == -math.inf) == (b in c["inf"])
    if name == "flat":       # every move costs ln 9, so the paths of three moves tie: the terminal blank takes i = 1 before i = 2, and so on back
        assert r["gap"] == 0.0 and r["label_frames"].tolist() == [0, 2] and r["label_durations"].tolist() == [2, 0]
        assert r["frame_labels"].tolist() == [-1, -1, 2] and r["frame_durations"].tolist() == [-1, -1, 1]


@pytest.mark.parametrize("name", GPU_CASES)
def test_premises_of_the_device_cases(name):
    c = A.case(name)
    for b, r in enumerate(A.reference(name)[0]):
        assert (r["score"] == -math.inf) == (b in c["inf"]), (name, b)
        assert r["gap"] > A.gap_threshold(c["lens"][b], len(c["labels"][b])), (name, b, r["gap"])


GOOD = dict(K.GOOD, dur=[0, 1, 2], sigma=0.0, ld=0x450000, fd=0x460000)
BAD = [("durations not ascending", dict(dur=[0, 2, 2]), "ascending"), ("negative sigma", dict(sigma=-0.1), "sigma"),
       ("label_durations overlaps frame_logp", dict(ld=0x430000 + 8), "d_label_durations overlaps d_frame_logp"),
       ("scores inside the workspace", dict(sc=0x800000 + 64), "d_scores overlaps d_workspace"), ("NULL scores", dict(sc=None), "NULL")] + K.WS_BAD


@pytest.mark.parametrize("name,change,word", BAD, ids=K.ids(BAD))
def test_device_form_rejects_before_touching_a_device(name, change, word):
    """dummy device pointers: a call that got past the checks would fault, a refusal never looks at them and writes nothing"""
    a, p = dict(GOOD, **change), K.ptr
    rc = capi.load().nntk_rnnt_tdt_align_device(p(a["x"]), a["B"], a["T"], a["V"], K.ints(a["dur"]), len(a["dur"]), K.ints(a["il"]),
                                                K.ints(a["lab"]), K.ints(a["ll"]), a["ML"], a["blank"], a["sigma"], p(a["lf"]), p(a["ld"]),
                                                p(a["fl"]), p(a["fd"]), p(a["lp"]), p(a["fp"]), p(a["sc"]), p(a["ws"]))
    assert rc == -1 and word in capi.last_error(), (name, capi.last_error())

