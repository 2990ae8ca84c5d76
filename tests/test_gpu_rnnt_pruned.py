"""The pruned transducer training loss (csrc/hip/rnnt_pruned.hip) against tests/rnnt_pruned_reference.py: the simple loss with its two
gradients and the occupancies, the prune ranges, the banded joiner, the banded loss with its gradient, and one training step end to end.

Tolerance: the project's transducer tolerance (tests/test_gpu_rnnt.py) -- per row and per output the device's error against float64 is
at most FACTOR x the error of a float32 torch restatement, or FLOOR where that is smaller; losses relative to |loss|, tensors relative
to the row's largest |value|.  Bit contracts are asserted with torch.equal / array_equal.

The base case: B = 3, T = 9, input lengths (9, 5, 2), max_label_len 4, label lengths (4, 0, 2): row 2 sits on the feasibility edge for
S = 2, row 1 has no labels.  V in {2, 5, 257, 260} covers the scalar and the 16-byte row paths of the emit and gradient bodies.

Beyond the base case: rnnt_prune_kernel's second and third pass of its 256 threads over the frames, with T_b on either side of 256
(test_prune_ranges_on_long_rows), its smallest shapes, and the simple loss's gradient on a lattice wider than 256
(test_simple_gradient_on_one_wide_lattice).  -inf scores and rows without a path: tests/test_gpu_rnnt_masked.py."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import rnnt_cases as K
import rnnt_pruned_reference as P
import rnnt_reference as R
from nntoolkitcore_amd import capi, layers as NL

pytestmark = pytest.mark.gpu

B0, T0, ML0, LENS0, LL0 = 3, 9, 4, [9, 5, 2], [4, 0, 2]
BASE = [(2, 0), (2, 1), (5, 0), (5, 4), (257, 0), (257, 256), (260, 0), (260, 259)]          # (V, blank): the blank first and last
KINDS = ("identity", "tanh", "relu")


@functools.lru_cache(maxsize=None)
def _base(V, blank):
    rng = np.random.default_rng(1000 * V + blank)
    labels = [K.labels(rng, n, V, blank) for n in LL0]
    am, lm = rng.uniform(-3, 3, (B0, T0, V)).astype(np.float32), rng.uniform(-3, 3, (B0, ML0 + 1, V)).astype(np.float32)
    for a in (am, lm):
        a.setflags(write=False)
    return dict(am=am, lm=lm, labels=labels, lens=LENS0, blank=blank)


def _nan_padded(c):
    am, lm = c["am"].copy(), c["lm"].copy()
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):
        am[b, n:] = np.nan
        lm[b, len(lab) + 1:] = np.nan
    return am, lm


@functools.lru_cache(maxsize=None)
def _simple_reference(V, blank):
    c = _base(V, blank)
    r64 = P.simple_loss(c["am"], c["lm"], c["labels"], c["lens"], blank)
    r32 = P.simple_loss(c["am"], c["lm"], c["labels"], c["lens"], blank, torch.float32)
    for a in r64 + r32:
        a.setflags(write=False)
    return r64, r32


def _close(tag, got, ref64, ref32, rel_to=None):
    """per row: |got - ref64| <= max(FACTOR |ref32 - ref64|, FLOOR), relative to the row's largest |ref64| (or to rel_to[b])"""
    got = np.asarray(got, np.float64)
    for b in range(got.shape[0]):
        sc = np.abs(ref64[b]).max() if rel_to is None else rel_to[b]
        if sc == 0:
            assert not np.asarray(got[b]).any(), (tag, b)
            continue
        e, e32 = np.abs(got[b] - ref64[b]).max() / sc, np.abs(ref32[b] - ref64[b]).max() / sc
        print("%s row %d (scale %.3g): err %.2e, torch f32 err %.2e" % (tag, b, sc, e, e32))
        assert e <= max(K.FACTOR * e32, K.FLOOR), (tag, b, e, e32)


def _simple(gpu, am, lm, c, **kw):
    """outputs prefilled with NaN: every element has to be written"""
    d_am, d_lm = torch.from_numpy(am.copy()).to(gpu), torch.from_numpy(lm.copy()).to(gpu)
    nan = lambda *s: torch.full(s, float("nan"), device=gpu)
    out = NL.rnnt_simple_loss_device(d_am, d_lm, c["labels"], input_lengths=c["lens"], blank=c["blank"], loss=nan(am.shape[0]),
                                     dam=nan(*am.shape), dlm=nan(*lm.shape), occ=nan(am.shape[0], am.shape[1], lm.shape[1]), **kw)
    torch.cuda.synchronize()
    return out


def _stored(gpu, x, c, want_grad=True):
    loss, g = NL.rnnt_loss_device(torch.from_numpy(np.ascontiguousarray(x)).to(gpu), c["labels"], input_lengths=c["lens"], blank=c["blank"],
                                  want_grad=want_grad)
    torch.cuda.synchronize()
    return loss, g


@pytest.mark.parametrize("V,blank", BASE)
def test_simple_loss(gpu, V, blank):
    c = _base(V, blank)
    am, lm = _nan_padded(c)
    loss, dam, dlm, occ = _simple(gpu, am, lm, c)
    # the bits of the stored loss on the float32 broadcast sum
    x = c["am"][:, :, None, :] + c["lm"][:, None, :, :]
    assert x.dtype == np.float32
    stored, _ = _stored(gpu, x, c, want_grad=False)
    assert torch.equal(loss, stored), (loss, stored)
    loss_only = _simple(gpu, am, lm, c, want_grad=False, want_occ=False)
    assert torch.equal(loss_only[0], loss) and loss_only[1] is None and loss_only[3] is None
    (l64, a64, m64, o64), (l32, a32, m32, o32) = _simple_reference(V, blank)
    assert not torch.isnan(dam).any() and not torch.isnan(dlm).any() and not torch.isnan(occ).any()
    _close("simple loss V %d" % V, loss.cpu().numpy()[:, None], l64[:, None], l32[:, None])
    _close("d_am V %d" % V, dam.cpu().numpy(), a64, a32)
    _close("d_lm V %d" % V, dlm.cpu().numpy(), m64, m32)
    _close("occ V %d" % V, occ.cpu().numpy(), o64, o32)
    o = occ.cpu().double().numpy()
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):
        assert not dam[b, n:].any() and not dlm[b, len(lab) + 1:].any() and not o[b, n:].any() and not o[b, :, len(lab) + 1:].any()
        for d in range(n + len(lab)):                     # every path crosses every anti-diagonal exactly once
            s = sum(o[b, t, d - t] for t in range(n) if 0 <= d - t <= len(lab))
            s64 = sum(o64[b, t, d - t] for t in range(n) if 0 <= d - t <= len(lab))
            s32 = sum(o32[b, t, d - t] for t in range(n) if 0 <= d - t <= len(lab))
            assert abs(s64 - 1.0) < 1e-12
            print("occ V %d row %d diagonal %d: |sum - 1| %.2e, torch f32 %.2e" % (V, b, d, abs(s - 1.0), abs(s32 - 1.0)))
            assert abs(s - 1.0) <= max(K.FACTOR * abs(s32 - 1.0), K.FLOOR), (b, d, s, s32)


def test_simple_loss_host_form_equals_the_device_form(gpu):
    c = _base(5, 4)
    dev = _simple(gpu, c["am"], c["lm"], c)
    host = NL.rnnt_simple_loss(c["am"], c["lm"], c["labels"], input_lengths=c["lens"], blank=c["blank"])
    for h, d in zip(host, dev):
        assert np.array_equal(h, d.cpu().numpy())


def _ranges(gpu, occ, S, lens=LENS0, ll=LL0):
    r = torch.full(occ.shape[:2], -77, dtype=torch.int32, device=gpu)
    NL.rnnt_prune_ranges_device(occ, ll, S, input_lengths=lens, ranges=r)
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("S", [2, 3, 5])
@pytest.mark.parametrize("V,blank", [(5, 0), (260, 259)])
def test_ranges_equal_the_reference_on_the_device_occupancies(gpu, V, blank, S):
    c = _base(V, blank)
    occ = _simple(gpu, *_nan_padded(c), c)[3]
    r = _ranges(gpu, occ, S)
    want = P.prune_ranges(occ.cpu().numpy(), LENS0, LL0, S)
    assert np.array_equal(r.cpu().numpy(), want), (r, want)
    assert P.feasible(2, 2, 2) and not P.feasible(2, 3, 2)          # row 2 on the edge for S = 2
    host = NL.rnnt_prune_ranges(occ.cpu().numpy(), LL0, S, input_lengths=LENS0)
    assert np.array_equal(host, want)


def test_ranges_take_the_lowest_window_on_a_tie(gpu):
    """a hand-made occupancy (T_b = 4, U_b = 5, S = 3, fin = 3): in frame 2 the windows from s = 1 and s = 3 weigh 0.75 each, the others
    less, and the fix-up admits both (r[1] = 1, so [1, 3]): the result shows which one was chosen"""
    occ = np.zeros((1, 4, 6), np.float32)
    occ[0, 0, 0] = occ[0, 1, 3] = occ[0, 3, 5] = 1.0
    occ[0, 2] = [0, 0.5, 0, 0.25, 0, 0.5]
    r = _ranges(gpu, torch.from_numpy(occ).to(gpu), 3, lens=[4], ll=[5])
    assert P.first_choice(occ[0], 4, 5, 3).tolist() == [0, 1, 1, 3]
    assert r.cpu().numpy().tolist() == P.prune_ranges(occ, [4], [5], 3).tolist() == [[0, 1, 1, 3]]
    occ[0, 2, 5] = 0.5 + 2.0 ** -20                       # ... and a heavier last window is taken
    r = _ranges(gpu, torch.from_numpy(occ).to(gpu), 3, lens=[4], ll=[5])
    assert r.cpu().numpy().tolist() == [[0, 1, 3, 3]]


# ---- the banded joiner ----

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("J", [5, 8])
def test_banded_joiner(gpu, kind, J):
    rng = np.random.default_rng(J)
    B, T, U1, S = 3, 9, 5, 2
    enc, pred, dout = (rng.uniform(-2, 2, s).astype(np.float32) for s in ((B, T, J), (B, U1, J), (B, T, S, J)))
    ranges = np.stack([np.sort(rng.integers(0, U1 - S + 1, T)) for _ in range(B)]).astype(np.int32)
    ranges[2, 3], ranges[2, 4] = -5, 1 << 30              # clamped into [0, U1 - S]
    e, p, d, r = (torch.from_numpy(a).to(gpu) for a in (enc, pred, dout, ranges))
    out = NL.rnnt_pruned_joint_device(e, p, r, S, kind, out=torch.full((B, T, S, J), float("nan"), device=gpu))
    full = NL.rnnt_joint_device(e, p, kind).cpu().numpy()
    rc = P.clamp_ranges(ranges, U1, S)
    want = np.stack([np.stack([full[b, t, rc[b, t]:rc[b, t] + S] for t in range(T)]) for b in range(B)])
    o = out.cpu()
    assert np.array_equal(o.numpy(), want)                # the bits of the full joiner, gathered
    denc = torch.full((B, T, J), float("nan"), device=gpu)
    dpred = torch.full((B, U1, J), float("nan"), device=gpu)
    NL.rnnt_pruned_joint_backward_device(out, d, r, U1, kind, denc=denc, dpred=dpred)
    torch.cuda.synchronize()
    r_enc, r_pred = P.pruned_joint_backward(o.double().numpy(), dout, ranges, U1, kind)
    # the float32 restatement, from the device's own forward output as the call takes it
    dd = torch.from_numpy(dout) * (1 - o * o if kind == "tanh" else (o > 0).float() if kind == "relu" else torch.ones_like(o))
    f_pred = torch.zeros((B, U1, J))
    for b in range(B):
        for t in range(T):
            f_pred[b, rc[b, t]:rc[b, t] + S] += dd[b, t]
    _close("banded joiner %s d_enc J %d" % (kind, J), denc.cpu().numpy(), r_enc, dd.sum(2).double().numpy())
    _close("banded joiner %s d_pred J %d" % (kind, J), dpred.cpu().numpy(), r_pred, f_pred.double().numpy())


# ---- the banded loss ----

def _band_logits(V, blank, S, seed=0):
    rng = np.random.default_rng(77 * V + blank + S + seed)
    x = rng.uniform(-3, 3, (B0, T0, S, V)).astype(np.float32)
    return x


def _pruned(gpu, x, ranges, c, ML=ML0, want_grad=True):
    d = torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    loss = torch.full((x.shape[0],), float("nan"), device=gpu)
    g = torch.full_like(d, float("nan")) if want_grad else None
    r = ranges if torch.is_tensor(ranges) else torch.from_numpy(np.ascontiguousarray(ranges, np.int32)).to(gpu)
    NL.rnnt_pruned_loss_device(d, r, c["labels"], ML, input_lengths=c["lens"], blank=c["blank"], want_grad=want_grad, loss=loss, dlogits=g)
    torch.cuda.synchronize()
    return loss.cpu(), (g.cpu() if want_grad else None)


@pytest.mark.parametrize("V,blank", BASE)
def test_banded_loss_with_the_whole_lattice_is_the_stored_loss(gpu, V, blank):
    """S = U1: loss and gradient bits of nntk_rnnt_loss_device, whatever the ranges hold (the clamp leaves 0 only)"""
    c = _base(V, blank)
    x = K.with_nan_padding(dict(x=_band_logits(V, blank, ML0 + 1), labels=c["labels"], lens=c["lens"]))
    stored_l, stored_g = _stored(gpu, x, c)
    for ranges in (np.zeros((B0, T0), np.int32), np.full((B0, T0), 3, np.int32)):
        loss, g = _pruned(gpu, x, ranges, c)
        assert torch.equal(loss, stored_l.cpu()) and torch.equal(g, stored_g.cpu())
    loss_only, none = _pruned(gpu, x, np.zeros((B0, T0), np.int32), c, want_grad=False)
    assert none is None and torch.equal(loss_only, stored_l.cpu())


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("V,blank", BASE)
def test_banded_loss_matches_float64(gpu, V, blank, S):
    c = _base(V, blank)
    occ = _simple(gpu, *_nan_padded(c), c)[3]
    r = _ranges(gpu, occ, S)
    ranges = r.cpu().numpy()
    x = _band_logits(V, blank, S)
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):              # NaN in all padding of the band
        x[b, n:] = np.nan
        for t in range(n):
            x[b, t, max(0, len(lab) + 1 - ranges[b, t]):] = np.nan
    loss, g = _pruned(gpu, x, r, c)
    l64, g64 = P.pruned_loss(x, ranges, c["labels"], c["lens"], blank, ML0 + 1)
    l32, g32 = P.pruned_loss(x, ranges, c["labels"], c["lens"], blank, ML0 + 1, torch.float32)
    assert np.isfinite(l64).all() and torch.isfinite(loss).all() and not torch.isnan(g).any()
    _close("banded loss V %d S %d" % (V, S), loss.numpy()[:, None], l64[:, None], l32[:, None])
    _close("banded gradient V %d S %d" % (V, S), g.numpy(), g64, g32)
    assert not g.numpy()[np.isnan(x)].any()                                  # exact zeros in the padding
    # never below the loss of the whole lattice, whose scores the band's cells are a part of
    full = np.zeros((B0, T0, ML0 + 1, V), np.float32)
    for b in range(B0):
        for t in range(T0):
            full[b, t, ranges[b, t]:ranges[b, t] + S] = np.nan_to_num(x[b, t])
    lf, _ = R.rnnt_loss_and_grad(full, c["labels"], c["lens"], blank)
    assert (l64 >= lf - 1e-9).all() and (loss.double().numpy() >= lf * (1 - K.FLOOR) - K.FLOOR).all(), (loss, lf)


@pytest.mark.parametrize("V,blank,S", [(5, 4, 2), (260, 0, 3)])
def test_banded_loss_host_form_equals_the_device_form(gpu, V, blank, S):
    """logits | ranges | loss rows share one device block in the host form: V = 5 puts the ranges behind a part that is rounded up"""
    c = _base(V, blank)
    occ = _simple(gpu, c["am"], c["lm"], c)[3]
    ranges = _ranges(gpu, occ, S).cpu().numpy()
    x = _band_logits(V, blank, S)
    loss, g = _pruned(gpu, x, ranges, c)
    hl, hg = NL.rnnt_pruned_loss(x, ranges, c["labels"], ML0, input_lengths=c["lens"], blank=blank)
    assert np.array_equal(hl, loss.numpy()) and np.array_equal(hg, g.numpy())
    hl2, none = NL.rnnt_pruned_loss(x, ranges, c["labels"], ML0, input_lengths=c["lens"], blank=blank, want_grad=False)
    assert none is None and np.array_equal(hl2, hl)


def test_hostile_ranges_stay_inside_the_tensors(gpu):
    """A bounds contract: ranges are device data no host check sees, so the kernels clamp every value into [0, U1 - S] (rnnt_range in
    rnnt_pruned.hip, applied before every index that a range enters).  Negative and huge values and a band that skips a label: the call
    returns, the row reports +inf with a zero gradient, and the other rows keep the bits of a call without the hostile row."""
    V, blank, S = 5, 4, 2
    c = _base(V, blank)
    occ = _simple(gpu, c["am"], c["lm"], c)[3]
    good = _ranges(gpu, occ, S).cpu().numpy()
    x = _band_logits(V, blank, S)
    ref_l, ref_g = _pruned(gpu, x, good, c)
    assert torch.isfinite(ref_l).all()
    hostile = {"negative": [-1, -2 ** 31, -7, -1, -3, -1, -1, -1, -1], "huge": [2 ** 31 - 1] * 9, "skips a label": [0, 0, 2, 2, 3, 3, 3, 3, 3],
               "starts late": [1, 1, 2, 2, 3, 3, 3, 3, 3]}
    for name, row in hostile.items():
        r = good.copy()
        r[0] = np.array(row, np.int64).astype(np.int32)
        loss, g = _pruned(gpu, x, r, c)
        assert math.isinf(float(loss[0])) and float(loss[0]) > 0 and not g[0].any(), (name, loss)
        assert torch.equal(loss[1:], ref_l[1:]) and torch.equal(g[1:], ref_g[1:]), name
        l64, _ = P.pruned_loss(x, r, c["labels"], c["lens"], blank, ML0 + 1)
        assert l64[0] == math.inf
        sub = dict(c, labels=c["labels"][1:], lens=c["lens"][1:])           # ... the bits of a call without the hostile row
        l1, g1 = _pruned(gpu, x[1:], r[1:], sub)
        assert torch.equal(l1, ref_l[1:]) and torch.equal(g1, ref_g[1:]), name
    # the joiner under the same ranges: the clamped gather, nothing else
    rng = np.random.default_rng(9)
    enc, pred = rng.uniform(-1, 1, (1, 9, 8)).astype(np.float32), rng.uniform(-1, 1, (1, 5, 8)).astype(np.float32)
    for row in hostile.values():
        rr = np.array([row], np.int64).astype(np.int32)
        out = NL.rnnt_pruned_joint_device(torch.from_numpy(enc).to(gpu), torch.from_numpy(pred).to(gpu), torch.from_numpy(rr).to(gpu), S, "identity")
        want = P.pruned_joint(enc, pred, rr, S, "identity")
        assert np.array_equal(out.cpu().numpy(), want.astype(np.float32))


@functools.lru_cache(maxsize=None)
def _wide():
    rng = np.random.default_rng(300)
    T, U, V, blank = 50, 300, 5, 2
    labels = [K.labels(rng, U, V, blank)]
    return dict(am=rng.uniform(-2, 2, (1, T, V)).astype(np.float32), lm=rng.uniform(-2, 2, (1, U + 1, V)).astype(np.float32), labels=labels,
                lens=[T], blank=blank)


def test_one_wide_lattice(gpu):
    """B = 1, T = 50, U = 300, S = 8, V = 5: beyond the 256-lane instantiation of the lattice kernel; the band is scattered into a lattice far
    wider than itself"""
    c, S, U = _wide(), 8, 300
    assert K.lattice_path(U)[0] == 2 and P.feasible(50, U, S)
    loss, _, _, occ = _simple(gpu, c["am"], c["lm"], c, want_grad=False)
    x = c["am"][:, :, None, :] + c["lm"][:, None, :, :]
    assert torch.equal(loss, _stored(gpu, x, c, want_grad=False)[0])
    r = _ranges(gpu, occ, S, lens=[50], ll=[U])
    ranges = r.cpu().numpy()
    assert np.array_equal(ranges, P.prune_ranges(occ.cpu().numpy(), [50], [U], S))
    assert ranges[0, 0] == 0 and ranges[0, -1] == U + 1 - S
    band = np.stack([x[0, t, ranges[0, t]:ranges[0, t] + S] for t in range(50)])[None]
    bl, bg = _pruned(gpu, band, r, c, ML=U)
    l64, g64 = P.pruned_loss(band, ranges, c["labels"], c["lens"], c["blank"], U + 1)
    l32, g32 = P.pruned_loss(band, ranges, c["labels"], c["lens"], c["blank"], U + 1, torch.float32)
    _close("wide banded loss", bl.numpy()[:, None], l64[:, None], l32[:, None])
    _close("wide banded gradient", bg.numpy(), g64, g32)
    assert float(bl[0]) >= float(loss[0]) * (1 - K.FLOOR)


def test_simple_gradient_on_one_wide_lattice(gpu):
    """the same case, with the gradient and the occupancies: rnnt_simple_reduce_kernel sums 301 terms into every d_am element and 50
    into every d_lm element (the base case: 5 and 9), and the cell kernel runs on a lattice wider than 256"""
    c = _wide()
    loss, dam, dlm, occ = _simple(gpu, c["am"], c["lm"], c)
    assert torch.equal(loss, _simple(gpu, c["am"], c["lm"], c, want_grad=False)[0])
    r64 = P.simple_loss(c["am"], c["lm"], c["labels"], c["lens"], c["blank"])
    r32 = P.simple_loss(c["am"], c["lm"], c["labels"], c["lens"], c["blank"], torch.float32)
    assert not torch.isnan(dam).any() and not torch.isnan(dlm).any() and not torch.isnan(occ).any()
    _close("wide simple loss", loss.cpu().numpy()[:, None], r64[0][:, None], r32[0][:, None])
    _close("wide d_am", dam.cpu().numpy(), r64[1], r32[1])
    _close("wide d_lm", dlm.cpu().numpy(), r64[2], r32[2])
    _close("wide occ", occ.cpu().numpy(), r64[3], r32[3])


# ---- the prune kernel beyond one pass of its 256 threads over the frames ----

PRUNE_THREADS = 256                                   # of rnnt_prune_kernel, mirrored (tests/test_rnnt_masked_host.py reads the source)


def _band_is_connected(r, lens, ll, S):
    for b, (Tb, Ub) in enumerate(zip(lens, ll)):
        fin = max(0, Ub + 1 - S)
        assert r[b, 0] == 0 and r[b, Tb - 1] == fin and (r[b, Tb:] == fin).all(), b
        assert all(0 <= r[b, t + 1] - r[b, t] <= S - 1 for t in range(Tb - 1)), b


def test_prune_ranges_on_long_rows(gpu):
    """T = 600: the threads go over t three times; T_b = 600, 257 (one frame into the second pass) and 256 (the first pass exactly)"""
    B, T, ML, lens, ll, S = 3, 600, 6, [600, 257, 256], [6, 0, 4], 3
    assert T > 2 * PRUNE_THREADS and sorted(lens)[:2] == [PRUNE_THREADS, PRUNE_THREADS + 1] and all(P.feasible(n, u, S) for n, u in zip(lens, ll))
    # random, plus a ridge that climbs over the whole row: the ranges never go down, so on noise alone they would reach their end within
    # a few frames and stay, whatever the later frames chose
    occ = np.random.default_rng(600).uniform(0, 1, (B, T, ML + 1)).astype(np.float32)
    for b, (n, u) in enumerate(zip(lens, ll)):
        for t in range(n):
            s = int(round(max(0, u + 1 - S) * t / (n - 1)))
            occ[b, t, s:s + S] += 4.0
    want = P.prune_ranges(occ, lens, ll, S)
    r = _ranges(gpu, torch.from_numpy(occ).to(gpu), S, lens=lens, ll=ll).cpu().numpy()
    assert np.array_equal(r, want), np.nonzero(r != want)
    _band_is_connected(r, lens, ll, S)
    assert len(set(want[0, PRUNE_THREADS:].tolist())) > 1             # the later passes decide something
    # NaN in the padding (t >= T_b, u > U_b) changes nothing: no window of a row with U_b + 1 >= S holds such a cell, and a row with
    # fewer positions than S (row 1) has the one window s = 0, whatever it weighs
    nan = occ.copy()
    for b, (n, u) in enumerate(zip(lens, ll)):
        nan[b, n:] = np.nan
        nan[b, :, u + 1:] = np.nan
    r2 = _ranges(gpu, torch.from_numpy(nan).to(gpu), S, lens=lens, ll=ll).cpu().numpy()
    assert np.array_equal(r2, want)
    assert np.array_equal(NL.rnnt_prune_ranges(occ, ll, S, input_lengths=lens), want)


def test_prune_ranges_at_the_smallest_shapes(gpu):
    """one frame on the feasibility edge (T_b = 1, U_b = 1, S = 2); S = 1 on a batch whose labels are all empty.  fin is 0 at both
    shapes, so 0 is the only answer a correct walk can give: what this guards is that the call is accepted at these sizes, that every
    element of the ranges is written (they are prefilled with -77), frames past T_b included, and that a window of S = U1 positions
    and steps of S - 1 = 0 stay inside the tensors.  It cannot tell one choice of window from another; test_prune_ranges_on_long_rows
    and the tie test do that"""
    assert P.feasible(1, 1, 2) and not P.feasible(1, 2, 2)
    occ = np.array([[[0.25, 0.75]]], np.float32)
    r = _ranges(gpu, torch.from_numpy(occ).to(gpu), 2, lens=[1], ll=[1]).cpu().numpy()
    assert r.tolist() == P.prune_ranges(occ, [1], [1], 2).tolist() == [[0]]
    occ = np.ones((2, 5, 1), np.float32)
    occ[1, 3:] = np.nan
    r = _ranges(gpu, torch.from_numpy(occ).to(gpu), 1, lens=[5, 3], ll=[0, 0]).cpu().numpy()
    assert r.tolist() == P.prune_ranges(occ, [5, 3], [0, 0], 1).tolist() == [[0] * 5, [0] * 5]


def test_repeat_and_batch_position(gpu):
    """the same call twice: the same bits; a row's outputs do not move when the batch is permuted"""
    V, blank, S = 260, 0, 3
    c = _base(V, blank)
    am, lm = _nan_padded(c)
    first = _simple(gpu, am, lm, c)
    again = _simple(gpu, am, lm, c)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    r = _ranges(gpu, first[3], S)
    x = _band_logits(V, blank, S)
    l1, g1 = _pruned(gpu, x, r, c)
    l2, g2 = _pruned(gpu, x, r, c)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    perm = [2, 0, 1]
    pc = dict(c, labels=[c["labels"][i] for i in perm], lens=[c["lens"][i] for i in perm])
    moved = _simple(gpu, am[perm], lm[perm], pc)
    assert all(torch.equal(m, f[perm]) for m, f in zip(moved, first))
    rp = _ranges(gpu, moved[3], S, lens=pc["lens"], ll=[LL0[i] for i in perm])
    assert torch.equal(rp, r[perm])
    lp_, gp_ = _pruned(gpu, x[perm], rp, pc)
    assert torch.equal(lp_, l1[perm]) and torch.equal(gp_, g1[perm])
    e, p = (torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, s).astype(np.float32)).to(gpu) for s in ((B0, T0, 8), (B0, ML0 + 1, 8)))
    j1 = NL.rnnt_pruned_joint_device(e, p, r, S)
    jp = NL.rnnt_pruned_joint_device(e[perm].contiguous(), p[perm].contiguous(), rp, S)
    assert torch.equal(jp, j1[perm])
    d = torch.from_numpy(np.random.default_rng(2).uniform(-1, 1, tuple(j1.shape)).astype(np.float32)).to(gpu)
    b1 = NL.rnnt_pruned_joint_backward_device(j1, d, r, ML0 + 1)
    bp = NL.rnnt_pruned_joint_backward_device(jp, d[perm].contiguous(), rp, ML0 + 1)
    assert torch.equal(bp[0], b1[0][perm]) and torch.equal(bp[1], b1[1][perm])


def test_end_to_end_one_training_step(gpu):
    """simple loss -> ranges -> banded joiner -> the library's training Dense on batch T S rows -> banded loss and gradient -> Dense gradient
    -> banded joiner backward, against torch float64 autograd on the same composition with the ranges held fixed; the float32 restatement
    is the same composition in torch float32"""
    L = capi.load()
    rng = np.random.default_rng(21)
    J, V, blank, S, U1 = 8, 5, 0, 2, ML0 + 1
    c = _base(V, blank)
    labels, lens = c["labels"], c["lens"]
    dp = lambda t: C.c_void_p(t.data_ptr())
    enc, pred = rng.uniform(-1, 1, (B0, T0, J)).astype(np.float32), rng.uniform(-1, 1, (B0, U1, J)).astype(np.float32)
    w = rng.uniform(-0.5, 0.5, J * V + V).astype(np.float32)
    _, _, _, occ = _simple(gpu, c["am"], c["lm"], c)
    r = _ranges(gpu, occ, S)
    ranges = r.cpu().numpy()
    d_enc, d_pred, d_w = (torch.from_numpy(a).to(gpu) for a in (enc, pred, w))
    rows = B0 * T0 * S
    dense = L.DenseCreateForTraining(L.DenseConfigCreate(J, V, None), capi.ConvTrainingConfig(rows))
    assert dense, capi.last_error()
    assert L.DenseLoadWeightsDevice(dense, dp(d_w)) == 0, capi.last_error()
    joint = NL.rnnt_pruned_joint_device(d_enc, d_pred, r, S, "tanh")
    logits = torch.empty((B0, T0, S, V), device=gpu)
    assert L.DenseApplyTrainingBatchDevice(dense, dp(joint), dp(logits)) == 0, capi.last_error()
    loss, dlogits = NL.rnnt_pruned_loss_device(logits, r, labels, ML0, input_lengths=lens, blank=blank)
    gw, djoint = torch.zeros_like(d_w), torch.empty_like(joint)
    assert L.DenseCalculateGradientDevice(dense, dp(gw), dp(djoint), dp(dlogits)) == 0, capi.last_error()
    denc, dpred = NL.rnnt_pruned_joint_backward_device(joint, djoint, r, U1, "tanh")
    torch.cuda.synchronize()
    L.DenseDestroy(dense)

    def compose(dtype):
        e, p, ww = (torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (enc, pred, w))
        idx = torch.from_numpy(P.clamp_ranges(ranges, U1, S))[:, :, None] + torch.arange(S)[None, None, :]
        z = torch.tanh(e[:, :, None, :] + p[torch.arange(B0)[:, None, None], idx])
        x = z @ ww[:J * V].view(J, V) + ww[J * V:]
        total, rows_ = 0, []
        for b in range(B0):
            Tb, Ub = lens[b], len(labels[b])
            alpha = {}
            for t in range(Tb):
                lp = torch.log_softmax(x[b, t], -1)
                for s in range(S):
                    u = int(ranges[b, t]) + s
                    if u > Ub:
                        continue
                    terms = []
                    if (t, u) == (0, 0):
                        terms.append(torch.zeros((), dtype=dtype))
                    if (t - 1, u) in alpha:
                        terms.append(alpha[(t - 1, u)][0] + alpha[(t - 1, u)][1])
                    if (t, u - 1) in alpha:
                        terms.append(alpha[(t, u - 1)][0] + alpha[(t, u - 1)][2])
                    if terms:
                        a = terms[0] if len(terms) == 1 else torch.logaddexp(terms[0], terms[1])
                        alpha[(t, u)] = (a, lp[s, blank], lp[s, labels[b][u]] if u < Ub else None)
            a, lb, _ = alpha[(Tb - 1, Ub)]
            rows_.append(-(a + lb))
            total = total + rows_[-1]
        ge, gp, gww = torch.autograd.grad(total, (e, p, ww))
        return [np.array([float(v.detach()) for v in rows_])] + [g.double().numpy() for g in (ge, gp, gww)]

    r64, r32 = compose(torch.float64), compose(torch.float32)
    got = [loss.cpu().numpy(), denc.cpu().numpy(), dpred.cpu().numpy(), gw.cpu().numpy()[None]]
    r64[3], r32[3] = r64[3][None], r32[3][None]
    _close("end to end loss", got[0][:, None], r64[0][:, None], r32[0][:, None])
    for name, g, a, b in zip(("d_enc", "d_pred", "d_W|b"), got[1:], r64[1:], r32[1:]):
        _close("end to end " + name, g, a, b)
    assert float(gw.abs().sum()) > 0 and float(denc.abs().sum()) > 0 and float(dpred.abs().sum()) > 0
