"""The host side of the pruned transducer loss calls (csrc/host/rnnt.c: simple loss, prune ranges, banded joiner, banded loss) -- the
workspace sizes and every argument check, all made before anything is allocated, uploaded or enqueued -- and the float64 reference the
device tests rely on (tests/rnnt_pruned_reference.py): its range fix-up on random feasible rows, its two losses against the full
lattice of tests/rnnt_reference.py and against enumeration of the paths inside a band.  No GPU."""
import itertools
import math

import numpy as np
import pytest
import torch

import rnnt_cases as K
import rnnt_pruned_reference as P
import rnnt_reference as R
from nntoolkitcore_amd import capi

# K.GOOD's shape (batch 2, T 6, max_label_len 3, V 5, J 8; input lengths 6 / 4, label lengths 2 / 1) with S = 2 and dummy device pointers
GOOD = dict(K.GOOD, S=2, U1=4, am=0x100000, lm=0x200000, dam=0x500000, dlm=0x600000, occ=0x700000, rg=0x900000, jout=0xA00000,
            jdout=0xB00000, denc=0x500000, dpred=0x600000)
S_BAD = [("S = 0", dict(S=0), "S 0"), ("S = U1 + 1", dict(S=5), "S 5")]
SIMPLE_BAD = K.BAD + K.WS_BAD + [
    ("only d_dam", dict(dlm=None), "all NULL or all given"), ("only d_dlm", dict(dam=None), "all NULL or all given"),
    ("NULL am", dict(am=None), "NULL"), ("NULL lm", dict(lm=None), "NULL"), ("misaligned am", dict(am=0x100004), "aligned"),
    ("misaligned lm", dict(lm=0x200008), "aligned"), ("NULL loss", dict(loss=None), "NULL"), ("misaligned occ", dict(occ=0x700002), "aligned"),
    ("d_dam overlaps d_am", dict(dam=0x100000 + 16), "overlaps"), ("d_dlm overlaps d_dam", dict(dlm=0x500000 + 64), "overlaps"),
    ("d_occ overlaps the workspace", dict(occ=0x800000 + 32), "overlaps"), ("loss overlaps d_lm", dict(loss=0x200000 + 8), "overlaps")]
PRUNE_BAD = S_BAD + [
    ("the row T_b = 1, U_b = 5, S = 2", dict(ML=5, il=[6, 1], ll=[2, 5]), "infeasible"),
    ("input length > T", dict(il=[7, 4]), "input_lengths"), ("input length 0", dict(il=[6, 0]), "input_lengths"),
    ("label length > max", dict(ll=[4, 1]), "label_lengths"), ("label length < 0", dict(ll=[2, -1]), "label_lengths"),
    ("NULL label lengths", dict(ll=None), "NULL"), ("batch < 0", dict(B=-1), "negative"),
    ("max_label_len beyond the limit", dict(ML=4001, ll=[0, 0]), "max_label_len"), ("T + max_label_len beyond the limit", dict(T=65536 - 2, il=None), "diagonals"),
    ("NULL occ", dict(occ=None), "NULL"), ("NULL ranges", dict(rg=None), "NULL"), ("misaligned ranges", dict(rg=0x900002), "aligned"),
    ("NULL workspace", dict(ws=None), "NULL"), ("ranges overlap d_occ", dict(rg=0x700000 + 16), "overlaps")]
JOINT_BAD = S_BAD + [
    ("activation 3", dict(act=3), "activation"), ("J < 0", dict(J=-4), "J"), ("batch < 0", dict(B=-1), "negative"),
    ("NULL ranges", dict(rg=None), "NULL"), ("NULL enc / out_fwd", dict(enc=None, jout=None), "NULL"), ("misaligned ranges", dict(rg=0x900002), "aligned")]
LOSS_BAD = K.BAD + K.WS_BAD + K.PLAIN_ONLY + K.LOSS_ONLY + S_BAD + [
    ("NULL ranges", dict(rg=None), "NULL"), ("misaligned ranges", dict(rg=0x900001), "aligned"),
    ("gradient overlaps the workspace", dict(g=0x800000 + 64), "overlaps"), ("loss overlaps the ranges", dict(loss=0x900000 + 4), "overlaps")]


def _simple(L, a):
    p, i = K.ptr, K.ints
    return L.nntk_rnnt_simple_loss_device(p(a["am"]), p(a["lm"]), a["B"], a["T"], a["V"], i(a["il"]), i(a["lab"]), i(a["ll"]), a["ML"], a["blank"],
                                          p(a["loss"]), p(a["dam"]), p(a["dlm"]), p(a["occ"]), p(a["ws"]))


def _prune(L, a):
    p, i = K.ptr, K.ints
    return L.nntk_rnnt_prune_ranges_device(p(a["occ"]), a["B"], a["T"], i(a["il"]), i(a["ll"]), a["ML"], a["S"], p(a["rg"]), p(a["ws"]))


def _loss(L, a):
    p, i = K.ptr, K.ints
    return L.nntk_rnnt_pruned_loss_device(p(a["x"]), p(a["rg"]), a["B"], a["T"], a["S"], a["V"], i(a["il"]), i(a["lab"]), i(a["ll"]), a["ML"],
                                          a["blank"], p(a["loss"]), p(a["g"]), p(a["ws"]))


@pytest.mark.parametrize("name,change,word", SIMPLE_BAD, ids=K.ids(SIMPLE_BAD))
def test_simple_loss_rejects_before_touching_a_device(name, change, word):
    """dummy device pointers: a call that got past the checks would fault, a refusal never looks at them"""
    assert _simple(capi.load(), dict(GOOD, **change)) == -1 and word in capi.last_error(), (name, capi.last_error())


@pytest.mark.parametrize("name,change,word", PRUNE_BAD, ids=K.ids(PRUNE_BAD))
def test_prune_ranges_rejects_before_touching_a_device(name, change, word):
    assert _prune(capi.load(), dict(GOOD, **change)) == -1 and word in capi.last_error(), (name, capi.last_error())


def test_prune_ranges_feasibility_edge_is_decided_by_the_inequality():
    """(T_b - 1)(S - 1) >= U_b + 1 - S; the refusal names the row.  One label more than the band can cross is refused, the edge is not
    (that call would go on to the device: only the refusal is exercised here)"""
    L = capi.load()
    for Tb, Ub, S in ((1, 5, 2), (2, 3, 2), (3, 8, 3), (4, 1, 1)):
        assert not P.feasible(Tb, Ub, S)
        assert _prune(L, dict(GOOD, T=6, ML=8, il=[6, Tb], ll=[0, Ub], S=S)) == -1 and "row 1" in capi.last_error(), (Tb, Ub, S)
    assert P.feasible(2, 2, 2) and P.feasible(1, 4, 5) and P.feasible(5, 0, 1) and not P.feasible(1, 1, 1)


@pytest.mark.parametrize("name,change,word", JOINT_BAD, ids=K.ids(JOINT_BAD))
def test_banded_joiner_rejects_before_touching_a_device(name, change, word):
    L, p = capi.load(), K.ptr
    a = dict(GOOD, **change)
    assert L.nntk_rnnt_pruned_joint_device(p(a["enc"]), p(a["pred"]), p(a["rg"]), a["B"], a["T"], a["U1"], a["S"], a["J"], a["act"],
                                           p(a["jout"])) == -1 and word in capi.last_error(), (name, capi.last_error())
    assert L.nntk_rnnt_pruned_joint_backward_device(p(a["jout"]), p(a["jdout"]), p(a["rg"]), a["B"], a["T"], a["U1"], a["S"], a["J"], a["act"],
                                                    p(a["denc"]), p(a["dpred"])) == -1 and word in capi.last_error(), (name, capi.last_error())


def test_banded_joiner_outputs_must_not_overlap():
    L, p, a = capi.load(), K.ptr, GOOD
    assert L.nntk_rnnt_pruned_joint_device(p(a["enc"]), p(a["pred"]), p(a["rg"]), 2, 6, 4, 2, 8, 1, p(a["enc"] + 32)) == -1
    assert "overlaps" in capi.last_error()
    assert L.nntk_rnnt_pruned_joint_backward_device(p(a["jout"]), p(a["jdout"]), p(a["rg"]), 2, 6, 4, 2, 8, 1, p(a["denc"]), p(a["denc"] + 64)) == -1
    assert "overlaps" in capi.last_error()
    # an empty tensor is not an error
    assert L.nntk_rnnt_pruned_joint_device(None, None, None, 0, 6, 4, 2, 8, 1, None) == 0 and capi.last_error() == ""


@pytest.mark.parametrize("name,change,word", LOSS_BAD, ids=K.ids(LOSS_BAD))
def test_banded_loss_rejects_before_touching_a_device(name, change, word):
    assert _loss(capi.load(), dict(GOOD, **change)) == -1 and word in capi.last_error(), (name, capi.last_error())


HOST_BAD = K.BAD


@pytest.mark.parametrize("name,change,word", HOST_BAD + S_BAD, ids=K.ids(HOST_BAD + S_BAD))
def test_host_forms_reject_and_write_nothing(name, change, word):
    L, i = capi.load(), K.ints
    a = dict(GOOD, **change)
    n = 1 << 12                                           # never read: the refusal comes first
    x, rg = np.zeros(n, np.float32), np.zeros(n, np.int32)
    outs = [np.full(n, 7.0, np.float32) for _ in range(4)]
    f = lambda v: v.ctypes.data_as(capi.fp)
    rc = L.nntk_rnnt_pruned_loss(f(x), rg.ctypes.data_as(capi.ip), a["B"], a["T"], a["S"], a["V"], i(a["il"]), i(a["lab"]), i(a["ll"]), a["ML"],
                                 a["blank"], f(outs[0]), f(outs[1]))
    assert rc == -1 and word in capi.last_error(), (name, capi.last_error())
    if not name.startswith("S ="):                        # S is no argument of the simple loss
        rc = L.nntk_rnnt_simple_loss(f(x), f(x), a["B"], a["T"], a["V"], i(a["il"]), i(a["lab"]), i(a["ll"]), a["ML"], a["blank"], *map(f, outs))
        assert rc == -1 and word in capi.last_error(), (name, capi.last_error())
    assert all((o == 7.0).all() for o in outs)


def test_host_prune_ranges_rejects_and_the_empty_batch_is_no_error():
    L, i = capi.load(), K.ints
    occ, rg = np.zeros(64, np.float32), np.full(64, 7, np.int32)
    for change, word in ((dict(S=0), "S 0"), (dict(S=5), "S 5"), (dict(ML=5, il=[6, 1], ll=[2, 5]), "infeasible")):
        a = dict(GOOD, **change)
        assert L.nntk_rnnt_prune_ranges(occ.ctypes.data_as(capi.fp), a["B"], a["T"], i(a["il"]), i(a["ll"]), a["ML"], a["S"],
                                        rg.ctypes.data_as(capi.ip)) == -1 and word in capi.last_error()
    assert (rg == 7).all()
    assert L.nntk_rnnt_prune_ranges_device(None, 0, 6, None, None, 3, 2, None, None) == 0 and capi.last_error() == ""
    assert L.nntk_rnnt_simple_loss_device(None, None, 0, 6, 5, None, None, None, 3, 4, None, None, None, None, None) == 0
    assert L.nntk_rnnt_pruned_loss_device(None, None, 0, 6, 2, 5, None, None, None, 3, 4, None, None, None) == 0 and capi.last_error() == ""


def test_workspace_sizes():
    L = capi.load()
    full, simple, pruned, prune = (L.nntk_rnnt_workspace_floats, L.nntk_rnnt_simple_workspace_floats, L.nntk_rnnt_pruned_workspace_floats,
                                   L.nntk_rnnt_prune_workspace_floats)
    for B, T, ML in ((1, 1, 0), (3, 50, 7), (16, 200, 40)):
        cells = B * T * (ML + 1)
        assert simple(B, T, ML, 0) == full(B, T, ML, 0)                         # loss only: the per-cell scalars of the stored loss
        assert full(B, T, ML, 1) + 4 * cells <= simple(B, T, ML, 1) <= full(B, T, ML, 1) + 4 * cells + 8      # 16 bytes a cell more
        assert pruned(B, T, ML, 0) == full(B, T, ML, 0) and pruned(B, T, ML, 1) == full(B, T, ML, 1)
        assert prune(B) >= 2 * B and prune(B + 1) >= prune(B)
    assert simple(64, 1000, 4000, 1) > 2 ** 31 and simple(0, 0, 0, 1) > 0 and prune(0) > 0


# ---- the reference itself ----

def test_range_fix_up_on_random_feasible_rows():
    """r[0] = 0, r[T_b - 1] = fin, monotone, steps of at most S - 1 -- and the first choice untouched where it had those properties
    already (half the rows are built around a valid band so that it has)"""
    rng = np.random.default_rng(5)
    rows = kept = 0
    while rows < 400:
        Tb, Ub = int(rng.integers(1, 13)), int(rng.integers(0, 9))
        S = int(rng.integers(2, Ub + 2)) if Ub >= 1 else 2
        U1 = max(Ub + 1, S)
        if not P.feasible(Tb, Ub, S):
            continue
        rows += 1
        fin = max(0, Ub + 1 - S)
        occ = rng.uniform(0, 1, (Tb, U1)).astype(np.float32)
        if rows % 2:                                      # a random valid band, its windows heavier than anything else
            path, prev = [], 0
            for t in range(Tb):
                lo, hi = max(0, fin - (Tb - 1 - t) * (S - 1), prev), min(fin, t * (S - 1), prev + S - 1)
                prev = int(rng.integers(lo, hi + 1))
                path.append(prev)
                occ[t] *= 0.01
                occ[t, prev:prev + S] += 1.0
        s0 = P.first_choice(occ, Tb, Ub, S)
        r = P.fix_up(s0, Tb, Ub, S)
        assert r[0] == 0 and r[-1] == fin, (Tb, Ub, S, r)
        d = np.diff(r)
        assert (d >= 0).all() and (d <= S - 1).all(), (Tb, Ub, S, r)
        ds = np.diff(s0)
        if s0[0] == 0 and s0[-1] == fin and (ds >= 0).all() and (ds <= S - 1).all():
            kept += 1
            assert np.array_equal(r, s0), (Tb, Ub, S, s0, r)
        if rows % 2:
            assert np.array_equal(s0, path)
        assert np.array_equal(P.prune_ranges(occ[None], [Tb], [Ub], S)[0], r)
    print("rows whose first choice needed no fix-up: %d of %d" % (kept, rows))
    assert kept >= 200


def test_first_choice_takes_the_lowest_window_on_a_tie():
    occ = np.zeros((1, 6), np.float32)
    occ[0] = [0, 0.5, 0.5, 0, 0.5, 0.5]                   # windows of 2: 0.5, 1, 0.5, 0.5, 1 -- s = 1 and s = 4 tie; of 3: 1, 1, 1, 1
    assert P.first_choice(occ, 1, 5, 2)[0] == 1 and P.first_choice(occ, 1, 5, 3)[0] == 0


def _small(rng, B, T, U1, V, blank):
    lens = [T] + [int(k) for k in rng.integers(1, T + 1, B - 1)]
    labels = [K.labels(rng, U1 - 1, V, blank)] + [K.labels(rng, int(rng.integers(0, U1)), V, blank) for _ in range(B - 1)]
    return lens, labels


def test_simple_loss_reference_equals_the_stored_reference_on_the_sum_tensor():
    rng = np.random.default_rng(2)
    B, T, U1, V, blank = 3, 5, 4, 5, 1
    lens, labels = _small(rng, B, T, U1, V, blank)
    am, lm = rng.uniform(-3, 3, (B, T, V)).astype(np.float32), rng.uniform(-3, 3, (B, U1, V)).astype(np.float32)
    x = (am[:, :, None, :] + lm[:, None, :, :]).astype(np.float64)
    l0, g0 = R.rnnt_loss_and_grad(x, labels, lens, blank)
    loss, dam, dlm, occ = P.simple_loss(am, lm, labels, lens, blank)
    np.testing.assert_allclose(loss, l0, rtol=1e-12)
    np.testing.assert_allclose(dam, g0.sum(2), atol=1e-12)
    np.testing.assert_allclose(dlm, g0.sum(1), atol=1e-12)
    for b in range(B):                                    # every path crosses every anti-diagonal once
        for n in range(lens[b] + len(labels[b])):
            assert abs(sum(occ[b, t, n - t] for t in range(lens[b]) if 0 <= n - t <= len(labels[b])) - 1.0) < 1e-12
        assert not occ[b, lens[b]:].any() and not occ[b, :, len(labels[b]) + 1:].any()
    l64, am64, lm64, o64 = P.simple_loss(am, lm, labels, lens, blank, torch.float64)
    np.testing.assert_allclose(l64, loss, rtol=1e-12)
    for got, want in ((am64, dam), (lm64, dlm), (o64, occ)):
        np.testing.assert_allclose(got, want, atol=1e-12)


def test_banded_loss_reference_equals_enumeration_inside_the_band():
    rng = np.random.default_rng(4)
    V, blank, S = 3, 0, 2
    for T, U in itertools.product((2, 3, 4), (1, 2, 3)):
        if not P.feasible(T, U, S):
            continue
        lab = K.labels(rng, U, V, blank)
        x = rng.uniform(-2, 2, (1, T, U + 1, V)).astype(np.float32)
        ranges = P.prune_ranges(rng.uniform(0, 1, (1, T, U + 1)).astype(np.float32), [T], [U], S)
        band = np.stack([x[0, t, ranges[0, t]:ranges[0, t] + S] for t in range(T)])[None]
        loss, grad = P.pruned_loss(band, ranges, [lab], [T], blank, U + 1)
        lp, total = R.log_softmax(x[0]), [0.0]

        def walk(t, u, logp):
            if not ranges[0, t] <= u < ranges[0, t] + S:
                return
            if u < U:
                walk(t, u + 1, logp + lp[t, u, lab[u]])
            if t + 1 < T:
                walk(t + 1, u, logp + lp[t, u, blank])
            elif u == U:
                total[0] += math.exp(logp + lp[t, u, blank])

        walk(0, 0, 0.0)
        assert abs(loss[0] + math.log(total[0])) <= 1e-12 * max(1.0, abs(loss[0])), (T, U)
        assert loss[0] >= R.rnnt_loss_and_grad(x, [lab], [T], blank)[0][0] - 1e-12
        l64, g64 = P.pruned_loss(band, ranges, [lab], [T], blank, U + 1, torch.float64)
        np.testing.assert_allclose(l64, loss, rtol=1e-12)
        np.testing.assert_allclose(g64, grad, atol=1e-12)
    # the whole lattice as one band is the stored loss; a band that skips a label carries no mass
    x = rng.uniform(-2, 2, (1, 3, 3, V)).astype(np.float32)
    l0, g0 = R.rnnt_loss_and_grad(x, [[1, 2]], [3], blank)
    l1, g1 = P.pruned_loss(x, np.zeros((1, 3), int), [[1, 2]], [3], blank, 3)
    np.testing.assert_allclose(l1, l0, rtol=1e-13)
    np.testing.assert_allclose(g1, g0, atol=1e-13)
    l2, g2 = P.pruned_loss(x[:, :, :1], np.array([[0, 2, 2]]), [[1, 2]], [3], blank, 3)
    assert l2[0] == math.inf and not g2.any()


def test_banded_joiner_reference_equals_autograd():
    rng = np.random.default_rng(3)
    B, T, U1, S, J = 2, 4, 5, 2, 3
    enc, pred, dout = rng.uniform(-2, 2, (B, T, J)), rng.uniform(-2, 2, (B, U1, J)), rng.uniform(-1, 1, (B, T, S, J))
    ranges = np.array([[0, 1, 1, 3], [0, 0, 2, 9]])       # 9: clamped to U1 - S
    idx = torch.from_numpy(P.clamp_ranges(ranges, U1, S))[:, :, None] + torch.arange(S)[None, None, :]
    for kind, fn in (("identity", lambda z: z), ("tanh", torch.tanh), ("relu", torch.relu)):
        e, p = torch.from_numpy(enc).requires_grad_(True), torch.from_numpy(pred).requires_grad_(True)
        out = fn(e[:, :, None, :] + p[torch.arange(B)[:, None, None], idx])
        ge, gp = torch.autograd.grad((out * torch.from_numpy(dout)).sum(), (e, p))
        o = P.pruned_joint(enc, pred, ranges, S, kind)
        np.testing.assert_allclose(o, out.detach().numpy(), rtol=1e-14, atol=0)
        de, dpd = P.pruned_joint_backward(o, dout, ranges, U1, kind)
        np.testing.assert_allclose(de, ge.numpy(), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(dpd, gp.numpy(), rtol=1e-12, atol=1e-14)
