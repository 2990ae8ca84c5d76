"""The host side of training the prediction network (csrc/host/rnnt_pred.c): every refusal of the embedding calls and of the predictor
handle that can be provoked without a device -- each -1 / NULL with a message and nothing touched -- the workspace size, and the
counting sort of the table gradient against numpy's stable argsort.  The refusals that need a live handle (a handle allocates device
memory when it is created: labels, lengths, the order of the calls, the projection pointers) are in tests/test_gpu_rnnt_predictor.py.
No GPU."""
import ctypes as C

import numpy as np
import pytest

from nntoolkitcore_amd import capi

P = lambda v: None if v is None else C.c_void_p(v)
IP = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(capi.ip)

LOOKUP_GOOD = dict(table=0x10000, V=5, E=8, ids=[0, 4, -1], out=0x20000)
LOOKUP_BAD = [("NULL table", dict(table=None), "d_table is NULL"), ("NULL out", dict(out=None), "d_out is NULL"),
              ("NULL ids", dict(ids=None, rows=3), "ids is NULL"), ("V = 0", dict(V=0), "V 0 < 1"), ("E = 0", dict(E=0), "E 0"),
              ("E above the limit", dict(E=1025), "E 1025"), ("rows < 0", dict(rows=-1), "rows -1"),
              ("id = V", dict(ids=[0, 5, 1]), "ids[1] = 5"), ("id = -2", dict(ids=[-2]), "ids[0] = -2"),
              ("misaligned out", dict(out=0x20002), "d_out is not 4-byte aligned"),
              ("misaligned table", dict(table=0x10001), "d_table is not 4-byte aligned"),
              ("out inside the table", dict(out=0x10010), "overlaps")]


@pytest.mark.parametrize("name,change,word", LOOKUP_BAD, ids=[b[0] for b in LOOKUP_BAD])
def test_lookup_rejects_before_touching_a_device(name, change, word):
    """dummy device pointers: a call that got past the checks would fault or need a device, a refusal never looks at them"""
    a = dict(LOOKUP_GOOD, **change)
    rows = a.get("rows", 0 if a["ids"] is None else len(a["ids"]))
    rc = capi.load().nntk_embedding_lookup_device(P(a["table"]), a["V"], a["E"], IP(a["ids"]), rows, P(a["out"]))
    assert rc == -1 and word in capi.last_error(), (name, capi.last_error())


GRAD_GOOD = dict(dout=0x10000, ids=[0, 4, -1], V=5, E=8, dtable=0x20000, ws=0x30000)
GRAD_BAD = [("NULL dout", dict(dout=None), "d_dout is NULL"), ("NULL dtable", dict(dtable=None), "d_dtable is NULL"),
            ("NULL workspace", dict(ws=None), "d_workspace is NULL"), ("NULL ids", dict(ids=None, rows=3), "ids is NULL"),
            ("V = 0", dict(V=0), "V 0 < 1"), ("E = 0", dict(E=0), "E 0"), ("E above the limit", dict(E=1025), "E 1025"),
            ("rows < 0", dict(rows=-1), "rows -1"), ("id = V", dict(ids=[5]), "ids[0] = 5"), ("id = -2", dict(ids=[1, -2]), "ids[1] = -2"),
            ("misaligned dtable", dict(dtable=0x20002), "d_dtable is not 4-byte aligned"),
            ("workspace 4-byte aligned only", dict(ws=0x30004), "d_workspace is not 16-byte aligned"),
            ("dtable overlapping dout", dict(dtable=0x10020), "d_dtable overlaps d_dout")]


@pytest.mark.parametrize("name,change,word", GRAD_BAD, ids=[b[0] for b in GRAD_BAD])
def test_gradient_rejects_before_touching_a_device(name, change, word):
    a = dict(GRAD_GOOD, **change)
    rows = a.get("rows", 0 if a["ids"] is None else len(a["ids"]))
    rc = capi.load().nntk_embedding_gradient_device(P(a["dout"]), IP(a["ids"]), rows, a["V"], a["E"], P(a["dtable"]), P(a["ws"]))
    assert rc == -1 and word in capi.last_error(), (name, capi.last_error())


def test_workspace_is_monotone_and_holds_the_documented_parts():
    L = capi.load()
    w = L.nntk_embedding_workspace_floats
    for E in (1, 5, 512):
        for V in (1, 2, 37, 4096):
            sizes = [w(rows, V, E) for rows in range(0, 700)]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (V, E)
            # V + 1 offsets, the sorted rows, and one partial row of E floats per possible chunk of a heavy id
            assert all(s >= V + 1 + rows + (rows // 16) * E for rows, s in enumerate(sizes)), (V, E)
        for rows in (0, 1, 131, 2624):
            sizes = [w(rows, V, E) for V in range(1, 300)]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (rows, E)


@pytest.mark.parametrize("rows,V,p_pad", [(0, 1, 0.0), (1, 1, 0.0), (7, 3, 0.5), (300, 8, 0.1), (300, 8, 1.0), (1000, 4096, 0.2), (5000, 2, 0.01)])
def test_counting_sort_equals_numpys_stable_argsort(rows, V, p_pad):
    """offsets and row lists on random ids, -1 included: an id's rows in ascending order, the padding in no list"""
    rng = np.random.default_rng(rows * 31 + V)
    ids = rng.integers(0, V, rows).astype(np.int32)
    ids[rng.random(rows) < p_pad] = -1
    offsets, srt = np.full(V + 1, -7, np.int32), np.full(max(rows, 1), -7, np.int32)
    n = capi.load().nntk_embedding_sort_ids(IP(ids) if rows else None, rows, V, offsets.ctypes.data_as(capi.ip), srt.ctypes.data_as(capi.ip))
    order = np.argsort(ids, kind="stable")
    order = order[ids[order] >= 0]
    assert n == order.shape[0] == offsets[V]
    np.testing.assert_array_equal(srt[:n], order)
    np.testing.assert_array_equal(offsets, np.concatenate([[0], np.cumsum(np.bincount(ids[ids >= 0], minlength=V))]))
    assert (srt[n:] == -7).all()


def test_counting_sort_refuses_bad_arguments():
    L = capi.load()
    off, srt = np.zeros(4, np.int32), np.zeros(4, np.int32)
    o, s = off.ctypes.data_as(capi.ip), srt.ctypes.data_as(capi.ip)
    assert L.nntk_embedding_sort_ids(IP([0, 3]), 2, 3, o, s) == -1 and "ids[1] = 3" in capi.last_error()
    assert L.nntk_embedding_sort_ids(IP([0]), 1, 0, o, s) == -1 and "V 0" in capi.last_error()
    assert L.nntk_embedding_sort_ids(IP([0]), -1, 3, o, s) == -1 and "rows -1" in capi.last_error()
    assert L.nntk_embedding_sort_ids(IP([0]), 1, 3, None, s) == -1 and "NULL" in capi.last_error()


def test_host_layer_under_address_and_undefined_sanitizers(tmp_path):
    """csrc/host/rnnt_pred.c compiled with -fsanitize=address,undefined into a stand-alone program (tests/rnnt_pred_host_asan.c: stubs
    below the host layer, the plan of the gradient walked at its exact allocation) and run on the CPU"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "rnnt_pred_host_asan")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unused-parameter",
                           "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "nntoolkitcore_amd", "csrc", "host"),
                           os.path.join(root, "nntoolkitcore_amd", "csrc", "host", "rnnt_pred.c"),
                           os.path.join(root, "tests", "rnnt_pred_host_asan.c"), "-o", exe])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "rnnt_pred host checks: ok" in res.stdout, res.stdout[-3000:]
    assert "AddressSanitizer" not in res.stdout and "runtime error" not in res.stdout


GOOD = dict(V=5, E=7, H=12, J=20, blank=0, has_proj=1, batch=3, max_label_len=4)
BAD = [("V = 1", dict(V=1), "V 1"), ("V above the limit", dict(V=8193), "limit"), ("blank = V", dict(blank=5), "blank"),
       ("blank < 0", dict(blank=-1), "blank"), ("E = 0", dict(E=0), "at least 1"), ("H = 0", dict(H=0), "at least 1"),
       ("J < 0", dict(J=-2), "at least 1"), ("E above the limit", dict(E=1025), "limit"), ("H above the limit", dict(H=1025), "limit"),
       ("J above the limit", dict(J=1025), "limit"), ("no projection with H != J", dict(has_proj=0), "H 12 != J 20"),
       ("has_proj = 2", dict(has_proj=2), "has_proj"), ("batch = 0", dict(batch=0), "batch 0"),
       ("max_label_len < 0", dict(max_label_len=-1), "max_label_len -1")]


@pytest.mark.parametrize("name,change,word", BAD, ids=[b[0] for b in BAD])
def test_create_rejects_before_touching_a_device(name, change, word):
    a = dict(GOOD, **change)
    cfg = capi.NntkRnntPredictorConfig(a["V"], a["E"], a["H"], a["J"], a["blank"], a["has_proj"], a["batch"], a["max_label_len"])
    assert not capi.load().nntk_rnnt_predictor_create(cfg) and word in capi.last_error(), (name, capi.last_error())


def test_null_handles_are_refused():
    L = capi.load()
    lab = np.zeros(4, np.int32).ctypes.data_as(capi.ip)
    assert L.nntk_rnnt_predictor_load_weights_device(None, P(0x1000), P(0x2000), P(0x3000)) == -1 and "NULL handle" in capi.last_error()
    assert L.nntk_rnnt_predictor_forward_device(None, lab, lab, P(0x1000)) == -1 and "NULL handle" in capi.last_error()
    assert L.nntk_rnnt_predictor_backward_device(None, P(0x1000), P(0x2000), P(0x3000), P(0x4000)) == -1 and "NULL handle" in capi.last_error()
    assert L.nntk_rnnt_predictor_device_bytes(None) == 0
    L.nntk_rnnt_predictor_destroy(None)
