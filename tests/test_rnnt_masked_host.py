"""The premises of the -inf tests of the transducer losses (tests/test_gpu_rnnt_masked.py), checked without a device: the references of
tests/rnnt_reference.py / rnnt_pruned_reference.py / rnnt_fused_reference.py alone, on the cases of tests/rnnt_masked_cases.py.  The
float64 lattice equals enumeration on every masked variant of a batch small enough to enumerate, and its gradient equals central
differences; every case has the rows at +inf that it says it has, in float64 and in the float32 torch restatement, and neither holds a
NaN; a masked class is a deleted class; the fused cases' -inf sits exactly in the masked columns; and the constants the fused cases
mirror are the source text's.  A wrong case or a moved constant turns red here.  No GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch

import rnnt_cases as K
import rnnt_fused_reference as FR
import rnnt_masked_cases as M
import rnnt_pruned_reference as P
import rnnt_reference as R

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nntoolkitcore_amd", "csrc", "hip")
TINY_VB = [(5, 0), (5, 4)]


def _define(name, text):
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, text, re.M)
    assert m, name
    return int(m.group(1))


def test_the_mirrored_constants_are_the_source_texts():
    with open(os.path.join(HIP, "rnnt_fused.hip")) as f:
        hip = f.read()
    assert _define("FT_WAVES", hip) == M.FT_WAVES == 8 and M.FT_COLS == 256
    assert "for (int n0 = wv * 32; n0 < V; n0 += FT_WAVES * 32) {" in hip             # wave w: the blocks w, w + 8, ... of 32 columns
    assert _define("FT_THREADS", hip) == 64 * M.FT_WAVES
    with open(os.path.join(HIP, "ctc_xf.hpp")) as f:
        assert _define("CTC_THREADS", f.read()) == K.CTC_THREADS == 256
    with open(os.path.join(HIP, "rnnt_pruned.hip")) as f:
        assert "for (int t = threadIdx.x; t < T; t += 256) {" in f.read()             # the prune kernel's stride over the frames
    # the wave's blocks as the fused cases lay them out
    blocks = lambda w: [(n0, min(n0 + M.FT_BLOCK, M.FUSED_V)) for n0 in range(w * M.FT_BLOCK, M.FUSED_V, M.FT_COLS)]
    assert blocks(0) == [(0, 32), (256, 288)] and blocks(1) == [(32, 64), (288, 300)] and blocks(2) == [(64, 96)]
    assert M.FUSED_MASKS["first block"] == list(range(*blocks(0)[0]))
    assert M.FUSED_MASKS["whole wave"] == [k for lo, hi in blocks(1) for k in range(lo, hi)]
    assert M.FUSED_MASKS["tail"] == list(range(*blocks(1)[1])) and len(M.FUSED_MASKS["tail"]) < M.FT_BLOCK


@pytest.mark.parametrize("variant", M.STORED_VARIANTS)
@pytest.mark.parametrize("V,blank", TINY_VB)
def test_float64_lattice_equals_enumeration(V, blank, variant):
    c = M.stored(V, blank, variant, tiny=True)
    assert max(c["lens"]) <= 4 and max(len(l) for l in c["labels"]) <= 3
    loss, grad = R.rnnt_loss_and_grad(c["x"], c["labels"], c["lens"], blank)
    assert not np.isnan(grad).any()
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):
        want = R.brute_force_loss(c["x"][b, :n, :len(lab) + 1], lab, blank)
        assert np.isfinite(want) == c["finite"][b], (c["name"], b, want)
        if c["finite"][b]:
            assert abs(loss[b] - want) <= 1e-12 * max(1.0, abs(want)), (c["name"], b, loss[b], want)
        else:
            assert loss[b] == math.inf and want == math.inf and not grad[b].any()
    assert not grad[np.isneginf(c["x"])].any()


@pytest.mark.parametrize("variant", [v for v in M.STORED_VARIANTS if v not in ("wall", "last blank", "all rows")])
@pytest.mark.parametrize("V,blank", TINY_VB)
def test_float64_gradient_equals_central_differences(V, blank, variant):
    """on the finite entries of the finite-loss variants.  h = 1e-5 on a loss whose third derivatives are O(1): truncation 1e-10,
    rounding 1e-16 |loss| / h = 1e-10: 1e-7 is asked"""
    c = M.stored(V, blank, variant, tiny=True)
    assert all(c["finite"])
    x = c["x"].astype(np.float64)
    _, grad = R.rnnt_loss_and_grad(x, c["labels"], c["lens"], blank)
    h, n = 1e-5, 0
    for b, (Tb, lab) in enumerate(zip(c["lens"], c["labels"])):
        row = lambda y: R.rnnt_loss_and_grad(y[None], [lab], [Tb], blank)[0][0]
        for t in range(Tb):
            for u in range(len(lab) + 1):
                for v in range(V):
                    if not np.isfinite(x[b, t, u, v]):
                        continue
                    up, dn = x[b].copy(), x[b].copy()
                    up[t, u, v] += h
                    dn[t, u, v] -= h
                    d = (row(up) - row(dn)) / (2 * h)
                    assert abs(d - grad[b, t, u, v]) <= 1e-7, (c["name"], b, t, u, v, d, grad[b, t, u, v])
                    n += 1
    assert n >= (16 + 3 + 3) * (V - 1) - V                # the live cells' entries but for the masked ones


def _rows_as_the_case_says(c, r64, r32):
    assert np.isfinite(r64[0]).tolist() == np.isfinite(r32[0]).tolist() == c["finite"], (c["name"], r64[0], r32[0])
    for b, ok in enumerate(c["finite"]):
        if not ok:
            assert r64[0][b] == math.inf and r32[0][b] == math.inf, c["name"]
    for a in tuple(r64[1:]) + tuple(r32[1:]):
        assert not np.isnan(a).any(), c["name"]
        for b, ok in enumerate(c["finite"]):
            if not ok and a.ndim > 1:
                assert not a[b].any(), c["name"]


@pytest.mark.parametrize("variant", M.STORED_VARIANTS)
@pytest.mark.parametrize("V,blank", M.STORED_VB)
def test_stored_cases(V, blank, variant):
    c = M.stored(V, blank, variant)
    assert [len(r) for r in c["labels"]] == [3, 0, 5] and c["lens"] == [7, 4, 1] and c["labels"][0][0] == c["labels"][0][1]
    assert M.masked_class(V) not in [blank] + sum(c["labels"], []) and (V != 260 or M.masked_class(V) >= 256)
    x = K.with_nan_padding(c)
    assert np.isneginf(c["x"]).any() and np.isneginf(x).sum() == np.isneginf(c["x"]).sum()                   # -inf in live cells only
    assert sorted(set(np.nonzero(np.isneginf(c["x"]))[0].tolist())) == c["masked"]
    r64 = R.rnnt_loss_and_grad(x, c["labels"], c["lens"], blank)
    r32 = R.torch_rnnt(x, c["labels"], c["lens"], blank, torch.float32)
    _rows_as_the_case_says(c, r64, r32)
    assert not r64[1][np.isneginf(x)].any() and not r32[1][np.isneginf(x)].any()
    if variant == "dead cell":                                                  # P > 0, nothing passes through the cell
        t, u = M.dead_cell(c)
        assert 0 < t < c["lens"][0] - 1 and 0 < u < len(c["labels"][0]) and not r64[1][0, t, u].any()
    if variant == "last blank":                                                 # alpha positive everywhere: only the final factor is 0
        y = c["x"].copy()
        y[2, 0, 5, blank] = 0.0
        assert np.isfinite(R.rnnt_loss_and_grad(y, c["labels"], c["lens"], blank)[0]).all()
    if variant == "forced":                                                     # one path: every label in frame 0
        lp = R.log_softmax(c["x"][0])
        one = sum(lp[0, u, k] for u, k in enumerate(c["labels"][0])) + lp[:, 3, blank].sum()
        assert abs(r64[0][0] + one) <= 1e-12 * abs(one)
    if variant == "class":                                                      # a masked class is a deleted class
        m = M.masked_class(V)
        move = lambda k: k - (k > m)
        l2, _ = R.rnnt_loss_and_grad(np.delete(np.nan_to_num(x), m, -1), [[move(k) for k in lab] for lab in c["labels"]], c["lens"], move(blank))
        assert np.abs(r64[0] - l2).max() <= 1e-12 * np.abs(l2).max() and not r64[1][..., m].any()


@pytest.mark.parametrize("variant", M.SIMPLE_VARIANTS)
@pytest.mark.parametrize("V,blank", M.STORED_VB)
def test_simple_cases(V, blank, variant):
    c = M.simple(V, blank, variant)
    assert [len(r) for r in c["labels"]] == M.SLL and c["lens"] == M.SLENS and M.masked_class(V) not in [blank] + sum(c["labels"], [])
    am, lm = M.nan_padded_sum(c)
    assert np.isneginf(am).sum() == np.isneginf(c["am"]).sum() and np.isneginf(lm).sum() == np.isneginf(c["lm"]).sum()
    assert np.isneginf(am).any() or np.isneginf(lm).any()
    r64 = P.simple_loss(am, lm, c["labels"], c["lens"], blank)
    r32 = P.simple_loss(am, lm, c["labels"], c["lens"], blank, torch.float32)
    _rows_as_the_case_says(c, r64, r32)
    if variant == "dead cell":                # the one live cell whose sum is all -inf; P > 0, its occupancy exactly 0 in both references
        x = M.sum_tensor(c)[0, :c["lens"][0], :len(c["labels"][0]) + 1]
        dead = np.argwhere(np.isneginf(x).all(-1)).tolist()
        assert dead == [list(M.SIMPLE_DEAD_CELL)] and c["finite"] == [True, True, True]
        t, u = M.SIMPLE_DEAD_CELL
        assert r64[3][0, t, u] == 0.0 and r32[3][0, t, u] == 0.0 and r64[3][0, t - 1, u] > 0.0 and r64[3][0, t + 1, u] > 0.0
        assert 0 < t < c["lens"][0] - 1 and 0 < u < len(c["labels"][0])
    if variant == "dead column":              # every cell of the column; P = 0, so the reductions never come to these cells
        x = M.sum_tensor(c)[0, :c["lens"][0], :len(c["labels"][0]) + 1]
        assert np.isneginf(x).all(-1)[:, 2].all() and not c["finite"][0]
    # the stored reference on the float32 sum tensor says the same
    l0, g0 = R.rnnt_loss_and_grad(K.with_nan_padding(dict(c, x=M.sum_tensor(c))), c["labels"], c["lens"], blank)
    ok = np.array(c["finite"])
    assert np.array_equal(np.isfinite(l0), ok) and np.allclose(l0[ok], r64[0][ok], rtol=1e-12, atol=0)
    np.testing.assert_allclose(r64[1], g0.sum(2), atol=1e-12)
    np.testing.assert_allclose(r64[2], g0.sum(1), atol=1e-12)


@pytest.mark.parametrize("variant", M.FUSED_VARIANTS)
def test_fused_cases(variant):
    c = M.fused(variant)
    J, V = M.FUSED_J, M.FUSED_V
    assert c["enc"].shape == (3, 7, J) and c["pred"].shape == (3, 6, J) and c["out"].shape == (J * V + V,) and c["lens"] == [7, 4, 1]
    assert [len(r) for r in c["labels"]] == [3, 0, 5] and np.isfinite(c["out"][:J * V]).all()
    _, logits = FR.fused_forward(c["enc"], c["pred"], c["out"], c["labels"], c["lens"], c["kind"])
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):
        live = logits[b, :n, :len(lab) + 1]
        assert np.isneginf(live[..., c["mask"]]).all() and np.isfinite(np.delete(live, c["mask"], -1)).all()
    args = (c["enc"], c["pred"], c["out"], c["labels"], c["lens"], c["blank"], c["kind"])
    _rows_as_the_case_says(c, FR.fused_loss_and_grads(*args), FR.torch_fused(*args, torch.float32))
    if variant != "blank masked":
        lab = sum(c["labels"], [])
        assert any(256 <= k < 288 for k in lab) and any(64 <= k < 96 for k in lab)


@pytest.mark.parametrize("ML,nj", [(300, 2), (600, 0)])
def test_wide_cases(ML, nj):
    c = M.wide(ML)
    assert K.lattice_path(ML)[0] == nj and c["x"].shape == (2, 6, ML + 1, 5)
    r64 = R.rnnt_loss_and_grad(c["x"], c["labels"], c["lens"], c["blank"])
    r32 = R.torch_rnnt(c["x"], c["labels"], c["lens"], c["blank"], torch.float32)
    _rows_as_the_case_says(c, r64, r32)
    lp = R.log_softmax(c["x"][0])                                               # row 0: one path
    one = sum(lp[0, u, k] for u, k in enumerate(c["labels"][0])) + lp[:, len(c["labels"][0]), c["blank"]].sum()
    assert abs(r64[0][0] + one) <= 1e-12 * abs(one)
