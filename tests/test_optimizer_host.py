"""CPU-only: nntk_optimizer_create refuses bad arguments before it allocates or enqueues anything (so without a GPU), with NULL / -1 and
a message; the new entry points are declared, bound and exported (tests/test_abi_and_symbols.py enforces header == bindings == library)."""
import ctypes as C

import pytest

from nntoolkitcore_amd import capi

LAYERS = ("Conv1d", "BatchNorm", "GRU", "LSTM", "RNN", "Dense", "TimeDistributedDense")
GOOD = dict(kind=2, learning_rate=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8)


def _create(L, n_blocks=1, w=(0x1000,), g=(0x2000,), sizes=(8,), **over):
    cfg = capi.NntkOptimizerConfig(**dict(GOOD, **over))
    k = max(1, len(sizes))
    wp = (C.c_void_p * k)(*w) if w is not None else None
    gp = (C.c_void_p * k)(*g) if g is not None else None
    sz = (C.c_long * k)(*sizes) if sizes is not None else None
    return L.nntk_optimizer_create(cfg, n_blocks, wp, gp, sz)


BAD = [
    ("kind 3", dict(kind=3), {}, "unknown kind"),
    ("kind -1", dict(kind=-1), {}, "unknown kind"),
    ("n_blocks < 0", {}, dict(n_blocks=-1), "n_blocks"),
    ("negative size", {}, dict(sizes=(-1,)), "negative size"),
    ("NULL weights", {}, dict(w=(None,)), "NULL"),
    ("NULL gradient", {}, dict(g=(None,)), "NULL"),
    ("NULL tables", {}, dict(w=None, g=None), "NULL"),
    ("misaligned", {}, dict(w=(0x1002,)), "aligned"),
    ("beta1 = 1", dict(beta1=1.0), {}, "beta1"),
    ("beta1 < 0", dict(beta1=-0.1), {}, "beta1"),
    ("beta2 = 1", dict(beta2=1.0), {}, "beta2"),
    ("beta2 nan", dict(beta2=float("nan")), {}, "beta2"),
    ("epsilon < 0", dict(epsilon=-1e-8), {}, "epsilon"),
    ("clip_norm < 0", dict(clip_norm=-1.0), {}, "clip_norm"),
    ("weight_decay < 0", dict(weight_decay=-0.01), {}, "weight_decay"),
    ("momentum < 0", dict(kind=1, momentum=-0.5), {}, "momentum"),
]


@pytest.mark.parametrize("name,cfg,args,word", BAD, ids=[b[0] for b in BAD])
def test_create_refuses_bad_arguments_without_a_gpu(built_lib, name, cfg, args, word):
    h = _create(built_lib, **dict(args, **cfg))
    assert not h, name
    err = capi.last_error()
    assert "nntk_optimizer_create" in err and word in err, err
    assert "HIP error" not in err, "the check must come before anything touches the device: " + err


def test_null_handles_return_minus_one_with_a_message(built_lib):
    L = built_lib
    assert L.nntk_optimizer_step_device(None) == -1 and "NULL handle" in capi.last_error()
    assert L.nntk_optimizer_set_learning_rate(None, C.c_float(0.1)) == -1 and "NULL handle" in capi.last_error()
    assert not L.nntk_optimizer_info_device(None) and "NULL handle" in capi.last_error()
    m, v = C.c_void_p(), C.c_void_p()
    assert L.nntk_optimizer_state_device(None, 0, C.byref(m), C.byref(v)) == -1 and "NULL handle" in capi.last_error()
    L.nntk_optimizer_destroy(None)
    for layer in LAYERS:
        assert getattr(L, layer + "LoadWeightsDevice")(None, C.c_void_p(0x1000)) == -1, layer
        assert layer + "LoadWeightsDevice: NULL handle" in capi.last_error()


def test_new_symbols_are_declared_bound_and_exported(built_lib):
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nntoolkitcore_hip.h")).read()
    names = [layer + "LoadWeightsDevice" for layer in LAYERS] + ["nntk_optimizer_" + s for s in
                                                                 ("create", "step_device", "set_learning_rate", "info_device", "state_device", "destroy")]
    for n in names:
        assert n + "(" in header and n in capi.SIGNATURES and hasattr(built_lib, n), n


def test_config_struct_matches_the_header():
    """the by-value struct the binding passes has the header's fields in the header's order (all 4-byte members: no padding)"""
    assert [f for f, _ in capi.NntkOptimizerConfig._fields_] == ["kind", "learning_rate", "momentum", "nesterov", "beta1", "beta2", "epsilon",
                                                               "weight_decay", "decoupled", "grad_scale", "clip_norm", "zero_gradients"]
    assert C.sizeof(capi.NntkOptimizerConfig) == 48
