"""CPU-only: every entry point of the bidirectional training calls (the *Bidirectional{ApplyTrainingBatch,CalculateGradient}[Device]
layer calls and the device forms of the gradient helpers) is declared in include/nntoolkitcore_hip.h, exported by the built library and
bound in capi.py; the argument checks that need no device refuse before they touch one."""
import os
import re

import pytest

from nntoolkitcore_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPERS = ["bd_merge_concat_gradient_device", "bd_merge_sum_gradient_device", "bd_accumulate_d_x_device",
           "bd_merge_gradient_varlen_device", "bd_accumulate_d_x_varlen_device"]
LAYER_CALLS = [cell + "Bidirectional" + call for cell in ("GRU", "LSTM", "RNN")
               for call in ("ApplyTrainingBatchDevice", "CalculateGradientDevice", "ApplyTrainingBatch", "CalculateGradient")]
NEW = HELPERS + LAYER_CALLS


def _declared():
    header = open(os.path.join(ROOT, "include", "nntoolkitcore_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    return set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", header))


@pytest.mark.parametrize("name", NEW)
def test_declared_exported_and_bound(built_lib, name):
    assert name in _declared(), "not declared in include/nntoolkitcore_hip.h"
    assert hasattr(built_lib, name), "not exported by the library"
    assert name in capi.SIGNATURES, "not bound in capi.py"
    res, args = capi.SIGNATURES[name]
    fn = getattr(built_lib, name)
    assert fn.restype is res and list(fn.argtypes) == list(args)


def test_signatures_have_the_documented_arity():
    import ctypes as C
    for cell in ("GRU", "LSTM", "RNN"):
        assert len(capi.SIGNATURES[cell + "BidirectionalApplyTrainingBatchDevice"][1]) == 6
        assert len(capi.SIGNATURES[cell + "BidirectionalCalculateGradientDevice"][1]) == 6
        assert len(capi.SIGNATURES[cell + "BidirectionalApplyTrainingBatch"][1]) == 6
        assert len(capi.SIGNATURES[cell + "BidirectionalCalculateGradient"][1]) == 6
    for name in NEW:
        assert capi.SIGNATURES[name][0] is C.c_int, name


def test_null_handles_and_bad_helper_arguments_fail_without_a_device(built_lib):
    """the checks that come before any device work: -1 and a message, on a machine without a GPU as well"""
    L = built_lib
    for cell in ("GRU", "LSTM", "RNN"):
        assert getattr(L, cell + "BidirectionalApplyTrainingBatchDevice")(None, None, None, None, None, 0) == -1
        assert "NULL handle" in capi.last_error()
        assert getattr(L, cell + "BidirectionalCalculateGradientDevice")(None, None, None, None, None, None) == -1
        assert "NULL handle" in capi.last_error()
        assert getattr(L, cell + "BidirectionalApplyTrainingBatch")(None, None, None, None, None, 0) == -1
        assert getattr(L, cell + "BidirectionalCalculateGradient")(None, None, None, None, None, None) == -1
        assert "NULL handle" in capi.last_error()
    cfg = capi.RecurrentConfig(4, 8, True, 5)
    assert L.bd_merge_concat_gradient_device(None, None, None, cfg, -1) == -1 and "batch" in capi.last_error()
    assert L.bd_accumulate_d_x_device(None, None, None, cfg, 2) == -1 and "NULL" in capi.last_error()
    assert L.bd_merge_gradient_varlen_device(None, None, None, cfg, 0, None, 7) == -1 and "merge" in capi.last_error()
    import numpy as np
    bad = np.array([1, 6], np.int32)
    one = capi.vp(16)          # never dereferenced: the lengths are refused first
    assert L.bd_accumulate_d_x_varlen_device(one, one, one, cfg, 2, bad.ctypes.data_as(capi.ip)) == -1
    assert "outside [0, 5]" in capi.last_error()
    assert L.bd_merge_gradient_varlen_device(one, one, one, cfg, 2, bad.ctypes.data_as(capi.ip), 0) == -1
    assert "outside [0, 5]" in capi.last_error()
    # batch 0: nothing to do, no device needed
    assert L.bd_merge_sum_gradient_device(None, None, None, cfg, 0) == 0 and capi.last_error() == ""
