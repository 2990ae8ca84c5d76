"""The four transducer loss forms (stored: csrc/hip/rnnt.hip; fused: rnnt_fused.hip; simple and banded: rnnt_pruned.hip) on -inf scores,
on rows without a path (P = 0) and on cells whose scores are all -inf: the cases of tests/rnnt_masked_cases.py (premises:
tests/test_rnnt_masked_host.py) against the -inf-safe float64 lattice of tests/rnnt_reference.py.

Tolerance: the project's transducer tolerance (tests/test_gpu_rnnt.py), nothing new -- per row and per output the device's error against
float64 is at most FACTOR x the error of the float32 torch restatement, or FLOOR where that is smaller; the loss relative to |loss|,
tensors relative to the row's largest |reference value| (d_out of the fused form: over the whole block).  Infinities, zeros and
NaN-freedom are exact assertions: a row the case calls P = 0 reports +inf and has zero rows in every gradient output, and no output
element is NaN (every output is prefilled with NaN, the padding of every input holds NaN).

Which branch these cases are the first to reach:
  rnnt_emission, the !(x > -INFINITY) arm: every case
  rnnt_lattice_kernel, ab.m == 0 ? INFINITY: wall, last blank, dead column, all rows, blank masked; zero emissions inside the
    NJ = 1 instantiation: every stored and simple case, NJ = 2 / NJ = 0: test_wide_lattices
  rnnt_grad_kernel / rnnt_band_grad_kernel, !(mP > 0): the P = 0 rows of the stored cases (the banded loss at S = U1 runs them too)
  rnnt_simple_cell_kernel / rnnt_simple_reduce_kernel<true / false>, the mP > 0 / hdr > 0 arms: the P = 0 rows of the simple cases
  rnnt_grad_value with an occupancy of exactly 0 and lse = NaN: dead cell -- in rnnt_grad_kernel (stored), rnnt_band_grad_kernel
    (banded, at S = U1 and on the narrow band) and both rnnt_simple_reduce_kernels (simple: the NaN went into d_am[0][4][:] and
    d_lm[0][1][:]).  dead column (simple) has such cells too, but its row is at P = 0 and the reductions skip it.  The fused
    backward's copy of the selection (ft_g_block) is reached by no case with lse = NaN: a fused cell is all -inf only if every
    bias entry is, and then the batch is at P = 0 and skipped; there the change is checked for unchanged bits only
  rnnt_band_emit_kernel / rnnt_band_grad_kernel on a band narrower than the lattice with -inf in it: test_banded_loss_on_a_narrow_band
  rnnt_fused_forward_kernel, the M[v] > -INFINITY reset: first block (wave 0 meets an all -inf block, then a finite one); the
    s_M[w] > -INFINITY guard of the merge: whole wave; a partial block masked entirely: tail; ft_tile_cells<true>, P = 0: blank masked"""
import functools
import math

import numpy as np
import pytest
import torch

import rnnt_cases as K
import rnnt_fused_reference as FR
import rnnt_masked_cases as M
import rnnt_pruned_reference as P
import rnnt_reference as R
from nntoolkitcore_amd import layers as NL

pytestmark = pytest.mark.gpu


def _check(tag, c, names, got, r64, r32, whole=()):
    """got / r64 / r32: per output an array whose first axis is the batch row (outputs named in `whole`: one block for the batch)"""
    for nm, g, a, b in zip(names, got, r64, r32):
        g, a, b = (np.asarray(v.cpu().numpy() if torch.is_tensor(v) else v, np.float64) for v in (g, a, b))
        assert not np.isnan(g).any(), (tag, nm, "NaN")
        assert not np.isnan(a).any() and not np.isnan(b).any(), (tag, nm, "NaN in a reference")
        rows = [None] if nm in whole else range(g.shape[0])
        for i in rows:
            gi, ai, bi = (g, a, b) if i is None else (g[i], a[i], b[i])
            if i is not None and not c["finite"][i]:             # P = 0: +inf, and exact zeros in every gradient row
                if nm == "loss":
                    assert ai == math.inf and bi == math.inf and gi == math.inf, (tag, i, gi)
                else:
                    assert not ai.any() and not gi.any(), (tag, nm, i)
                continue
            sc = np.abs(ai).max()
            assert np.isfinite(sc), (tag, nm, i)
            if sc == 0:
                assert not gi.any(), (tag, nm, i)
                continue
            e, e32 = np.abs(gi - ai).max() / sc, np.abs(bi - ai).max() / sc
            print("%s %s row %s (scale %.3g): err %.2e, torch f32 err %.2e" % (tag, nm, i, sc, e, e32))
            assert e <= max(K.FACTOR * e32, K.FLOOR), (tag, nm, i, e, e32)


def _equal(a, b):
    return all((x is None and y is None) or torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


# ---- the stored form, and the banded form on the whole lattice ----

@functools.lru_cache(maxsize=None)
def _stored_refs(V, blank, variant):
    c = M.stored(V, blank, variant)
    r = R.rnnt_loss_and_grad(c["x"], c["labels"], c["lens"], blank) + R.torch_rnnt(c["x"], c["labels"], c["lens"], blank, torch.float32)
    for a in r:
        a.setflags(write=False)
    return c, r[:2], r[2:]


def _stored(gpu, x, c, want_grad=True):
    """outputs prefilled with NaN: every element has to be written"""
    d = torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    loss = torch.full((x.shape[0],), float("nan"), device=gpu)
    g = torch.full_like(d, float("nan")) if want_grad else None
    NL.rnnt_loss_device(d, c["labels"], input_lengths=c["lens"], blank=c["blank"], want_grad=want_grad, loss=loss, dlogits=g)
    torch.cuda.synchronize()
    return loss.cpu(), (g.cpu() if want_grad else None)


def _banded(gpu, x, ranges, c, ML, want_grad=True):
    d = torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    loss = torch.full((x.shape[0],), float("nan"), device=gpu)
    g = torch.full_like(d, float("nan")) if want_grad else None
    r = ranges if torch.is_tensor(ranges) else torch.from_numpy(np.ascontiguousarray(ranges, np.int32)).to(gpu)
    NL.rnnt_pruned_loss_device(d, r, c["labels"], ML, input_lengths=c["lens"], blank=c["blank"], want_grad=want_grad, loss=loss, dlogits=g)
    torch.cuda.synchronize()
    return loss.cpu(), (g.cpu() if want_grad else None)


def _padding_is_zero(c, g):
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):
        assert not g[b, n:].any() and not g[b, :, len(lab) + 1:].any(), (c["name"], b)


@pytest.mark.parametrize("variant", M.STORED_VARIANTS)
@pytest.mark.parametrize("V,blank", M.STORED_VB)
def test_stored_and_banded_loss(gpu, V, blank, variant):
    c, r64, r32 = _stored_refs(V, blank, variant)
    x = K.with_nan_padding(c)
    loss, g = _stored(gpu, x, c)
    _check(c["name"], c, ("loss", "gradient"), (loss[:, None], g), (r64[0][:, None], r64[1]), (r32[0][:, None], r32[1]))
    assert np.isneginf(x).any() and not g.numpy()[np.isneginf(x)].any()          # a -inf score: a gradient of exactly 0
    _padding_is_zero(c, g)
    if variant == "all rows":
        assert torch.isposinf(loss).all() and not g.any()
    assert _equal((loss, g), _stored(gpu, x, c))                                 # the same call twice
    assert _equal(_stored(gpu, x, c, want_grad=False), (loss, None))             # the loss bits with and without a gradient
    rest, keep = M.without_rows(dict(c, x=x), c["masked"])                       # the other rows: the bits of a call without the masked ones
    if keep:
        l1, g1 = _stored(gpu, rest["x"], rest)
        assert _equal((l1, g1), (loss[keep], g[keep])), c["name"]
    # the banded loss with the whole lattice as its band: the stored loss's bits, gradient included
    bl, bg = _banded(gpu, x, np.zeros(x.shape[:2], np.int32), c, x.shape[2] - 1)
    assert _equal((bl, bg), (loss, g)), c["name"]
    assert _equal(_banded(gpu, x, np.zeros(x.shape[:2], np.int32), c, x.shape[2] - 1, want_grad=False), (loss, None))


def test_stored_host_form_equals_the_device_form(gpu):
    """as test_simple_host_form_equals_the_device_form: the host path on a P = 0 row and on a dead cell, and no NaN comes back"""
    c = M.stored(5, 4, "wall")
    loss, g = _stored(gpu, c["x"], c)
    hl, hg = NL.rnnt_loss(c["x"], c["labels"], input_lengths=c["lens"], blank=c["blank"])
    assert np.array_equal(hl, loss.numpy()) and np.array_equal(hg, g.numpy()) and hl[0] == math.inf and np.isfinite(hl[1:]).all()
    c = M.stored(260, 0, "dead cell")
    loss, g = _stored(gpu, c["x"], c)
    hl, hg = NL.rnnt_loss(c["x"], c["labels"], input_lengths=c["lens"], blank=c["blank"])
    assert np.array_equal(hl, loss.numpy()) and np.array_equal(hg, g.numpy(), equal_nan=True) and not np.isnan(hg).any()


@pytest.mark.parametrize("ML,nj", [(300, 2), (600, 0)])
def test_wide_lattices(gpu, ML, nj):
    """rnnt_lattice_kernel<2> and <0> with zero emissions: a forced row (one path, 300 labels in frame 0) and a walled row in one batch"""
    c = M.wide(ML)
    assert K.lattice_path(ML)[0] == nj and c["finite"] == [True, False]
    r64 = R.rnnt_loss_and_grad(c["x"], c["labels"], c["lens"], c["blank"])
    r32 = R.torch_rnnt(c["x"], c["labels"], c["lens"], c["blank"], torch.float32)
    x = K.with_nan_padding(c)
    loss, g = _stored(gpu, x, c)
    _check(c["name"], c, ("loss", "gradient"), (loss[:, None], g), (r64[0][:, None], r64[1]), (r32[0][:, None], r32[1]))
    assert not g.numpy()[np.isneginf(x)].any()
    _padding_is_zero(c, g)
    assert _equal(_stored(gpu, x, c, want_grad=False), (loss, None))


# ---- the simple form ----

SIMPLE_NAMES = ("loss", "d_am", "d_lm", "occ")


@functools.lru_cache(maxsize=None)
def _simple_refs(V, blank, variant):
    c = M.simple(V, blank, variant)
    r64 = P.simple_loss(c["am"], c["lm"], c["labels"], c["lens"], blank)
    r32 = P.simple_loss(c["am"], c["lm"], c["labels"], c["lens"], blank, torch.float32)
    for a in r64 + r32:
        a.setflags(write=False)
    return c, r64, r32


def _simple(gpu, am, lm, c, **kw):
    d_am, d_lm = torch.from_numpy(am.copy()).to(gpu), torch.from_numpy(lm.copy()).to(gpu)
    nan = lambda *s: torch.full(s, float("nan"), device=gpu)
    out = NL.rnnt_simple_loss_device(d_am, d_lm, c["labels"], input_lengths=c["lens"], blank=c["blank"], loss=nan(am.shape[0]),
                                     dam=nan(*am.shape), dlm=nan(*lm.shape), occ=nan(am.shape[0], am.shape[1], lm.shape[1]), **kw)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu() for t in out)


@pytest.mark.parametrize("variant", M.SIMPLE_VARIANTS)
@pytest.mark.parametrize("V,blank", M.STORED_VB)
def test_simple_loss(gpu, V, blank, variant):
    c, r64, r32 = _simple_refs(V, blank, variant)
    am, lm = M.nan_padded_sum(c)
    got = _simple(gpu, am, lm, c)
    loss, dam, dlm, occ = got
    _check(c["name"], c, SIMPLE_NAMES, (loss[:, None],) + got[1:], (r64[0][:, None],) + r64[1:], (r32[0][:, None],) + r32[1:])
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):                   # exact zeros in the padding
        assert not dam[b, n:].any() and not dlm[b, len(lab) + 1:].any() and not occ[b, n:].any() and not occ[b, :, len(lab) + 1:].any()
    assert not dam.numpy()[np.isneginf(am)].any() and not dlm.numpy()[np.isneginf(lm)].any()
    if variant == "all rows":
        assert torch.isposinf(loss).all() and not dam.any() and not dlm.any() and not occ.any()
    # the bits of the stored loss on the float32 broadcast sum
    x = K.with_nan_padding(dict(c, x=M.sum_tensor(c)))
    assert torch.equal(loss, _stored(gpu, x, c, want_grad=False)[0]), c["name"]
    assert _equal(_simple(gpu, am, lm, c), got)
    only = _simple(gpu, am, lm, c, want_grad=False, want_occ=False)
    assert _equal(only, (loss, None, None, None))
    rest, keep = M.without_rows(dict(c, am=am, lm=lm), c["masked"])
    if keep:
        assert _equal(_simple(gpu, rest["am"], rest["lm"], rest), tuple(t[keep] for t in got)), c["name"]


def test_simple_host_form_equals_the_device_form(gpu):
    """the host-pointer form uploads, runs the device form and downloads: this guards that path's sizes and copies on inputs that hold
    -inf (a P = 0 row, a masked class), not the kernels -- a wrong kernel gives both forms the same wrong bits"""
    for variant in ("wall", "class am"):
        c = M.simple(260, 259, variant)
        dev = _simple(gpu, c["am"], c["lm"], c)
        host = NL.rnnt_simple_loss(c["am"], c["lm"], c["labels"], input_lengths=c["lens"], blank=c["blank"])
        for h, d in zip(host, dev):
            assert np.array_equal(h, d.numpy()) and not np.isnan(h).any()


def test_pruned_chain_on_a_dead_row(gpu):
    """simple loss with a wall -> occupancies all zero in row 0 -> every window ties at zero and the lowest wins, so the forward pass
    alone shapes the band -> the banded loss on finite scores through those ranges is finite again"""
    V, blank, S = 5, 0, 2
    c, r64, _ = _simple_refs(V, blank, "wall")
    am, lm = M.nan_padded_sum(c)
    occ = _simple(gpu, am, lm, c)[3]
    assert not occ[0].any() and occ[1].any() and occ[2].any() and not r64[3][0].any()
    d_occ = occ.to(gpu)
    ranges = torch.full(occ.shape[:2], -77, dtype=torch.int32, device=gpu)
    NL.rnnt_prune_ranges_device(d_occ, M.SLL, S, input_lengths=c["lens"], ranges=ranges)
    torch.cuda.synchronize()
    r = ranges.cpu().numpy()
    want = P.prune_ranges(occ.numpy(), c["lens"], M.SLL, S)
    assert np.array_equal(r, want), (r, want)
    Tb, Ub = c["lens"][0], M.SLL[0]
    assert P.first_choice(occ.numpy()[0], Tb, Ub, S).tolist() == [0] * Tb            # the tie at zero: the lowest window
    assert r[0, 0] == 0 and r[0, Tb - 1] == Ub + 1 - S and all(0 <= r[0, t + 1] - r[0, t] <= S - 1 for t in range(Tb - 1))     # connected
    rng = np.random.default_rng(6)
    x = rng.uniform(-3, 3, (M.SB, M.ST, S, V)).astype(np.float32)
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):                   # NaN in all padding of the band
        x[b, n:] = np.nan
        for t in range(n):
            x[b, t, max(0, len(lab) + 1 - r[b, t]):] = np.nan
    loss, g = _banded(gpu, x, ranges, c, M.SML)
    l64, g64 = P.pruned_loss(x, r, c["labels"], c["lens"], blank, M.SML + 1)
    l32, g32 = P.pruned_loss(x, r, c["labels"], c["lens"], blank, M.SML + 1, torch.float32)
    assert np.isfinite(l64).all() and torch.isfinite(loss).all()
    _check("banded loss after a dead row", dict(c, finite=[True] * 3), ("loss", "gradient"), (loss[:, None], g), (l64[:, None], g64), (l32[:, None], g32))
    assert not g.numpy()[np.isnan(x)].any()


@pytest.mark.parametrize("variant", ["class", "wall", "dead cell"])
@pytest.mark.parametrize("V,blank", M.STORED_VB)
def test_banded_loss_on_a_narrow_band(gpu, V, blank, variant):
    """S = 2 < U1, the band from the device's own ranges on the unmasked simple case; -inf goes into the band's scores: the masked
    class in every live band cell; label y_2 of row 0 in every band cell at u = 1 (P = 0); every score of the upper band cell
    (t, r[t] + 1) of row 0 in a frame where the band stands still, r[t-1] = r[t] = r[t+1] (there is one: row 0's ranges rise by 3
    over 8 steps of at most 1, so two of the 5 level steps are neighbours): a path goes round it by (t-1, r) -> (t, r) -> (t+1, r),
    and every cell of a connected band of two is reached from (0, 0) and reaches (T_b - 1, U_b), so P > 0"""
    S = 2
    c = M.simple_base(V, blank)
    occ = _simple(gpu, c["am"], c["lm"], c)[3]
    ranges = torch.full(occ.shape[:2], -77, dtype=torch.int32, device=gpu)
    NL.rnnt_prune_ranges_device(occ.to(gpu), M.SLL, S, input_lengths=c["lens"], ranges=ranges)
    torch.cuda.synchronize()
    r = ranges.cpu().numpy()
    x = np.random.default_rng(V + blank).uniform(-3, 3, (M.SB, M.ST, S, V)).astype(np.float32)
    live = np.zeros(x.shape[:3], bool)
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):
        for t in range(n):
            live[b, t, :max(0, len(lab) + 1 - r[b, t])] = True
    finite = [True, True, True]
    if variant == "class":
        x[..., M.masked_class(V)] = M.NINF
    elif variant == "wall":
        for t in range(c["lens"][0]):
            if r[0, t] <= 1 < r[0, t] + S:
                x[0, t, 1 - r[0, t], c["labels"][0][1]] = M.NINF
        finite[0] = False
    else:
        still = [t for t in range(1, c["lens"][0] - 1) if r[0, t - 1] == r[0, t] == r[0, t + 1]]
        assert still and live[0, still[0], 1], r[0]
        dead = (0, still[0], 1)
        x[dead] = M.NINF
    x[~live] = np.nan                                                             # NaN in all padding of the band
    assert np.isneginf(x).any()
    l64, g64 = P.pruned_loss(x, r, c["labels"], c["lens"], blank, M.SML + 1)
    l32, g32 = P.pruned_loss(x, r, c["labels"], c["lens"], blank, M.SML + 1, torch.float32)
    if variant == "dead cell":
        assert not g64[dead].any()
    assert np.isfinite(l64).tolist() == finite == np.isfinite(l32).tolist()
    case = dict(c, finite=finite)
    loss, g = _banded(gpu, x, ranges, case, M.SML)
    _check("banded %s V %d blank %d" % (variant, V, blank), case, ("loss", "gradient"), (loss[:, None], g), (l64[:, None], g64), (l32[:, None], g32))
    assert not g.numpy()[np.isneginf(x)].any() and not g.numpy()[np.isnan(x)].any()
    assert _equal(_banded(gpu, x, ranges, case, M.SML), (loss, g))
    assert _equal(_banded(gpu, x, ranges, case, M.SML, want_grad=False), (loss, None))
    if variant != "class":                                                        # rows 1 and 2: the bits of a call without row 0
        rest = dict(case, labels=c["labels"][1:], lens=c["lens"][1:])
        assert _equal(_banded(gpu, x[1:], r[1:], rest, M.SML), (loss[1:], g[1:]))


# ---- the fused form ----

FUSED_NAMES = ("loss", "d_enc", "d_pred", "d_out")


def _fused(gpu, enc, pred, c, want_grad=True):
    e, p, o = (torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in (enc, pred, c["out"]))
    nan = lambda t: torch.full_like(t, float("nan"))
    loss = torch.full((enc.shape[0],), float("nan"), device=gpu)
    g = (nan(e), nan(p), nan(o)) if want_grad else (None, None, None)
    NL.rnnt_fused_loss_device(e, p, o, c["labels"], input_lengths=c["lens"], blank=c["blank"], activation=c["kind"], want_grad=want_grad,
                              loss=loss, denc=g[0], dpred=g[1], dout=g[2])
    torch.cuda.synchronize()
    return (loss.cpu(),) + tuple(t.cpu() if want_grad else None for t in g)


@pytest.mark.parametrize("variant", M.FUSED_VARIANTS)
def test_fused_loss(gpu, variant):
    """`tail` has no guard of its own in the kernel: the masked partial block [288, 300) shares its 32-column block with the columns
    past V, which the forward sets to -inf itself, so it asks that a block can be all -inf AFTER the wave has a finite maximum
    (expf(-inf - M) = 0 adds nothing) and that the masked columns get a zero gradient in W and b"""
    c = M.fused(variant)
    J, V = M.FUSED_J, M.FUSED_V
    enc, pred = K.with_nan_padding(c)
    got = _fused(gpu, enc, pred, c)
    args = (c["enc"], c["pred"], c["out"], c["labels"], c["lens"], c["blank"], c["kind"])
    r64, r32 = FR.fused_loss_and_grads(*args), FR.torch_fused(*args, torch.float32)
    _check(c["name"], c, FUSED_NAMES, (got[0][:, None],) + got[1:], (r64[0][:, None],) + r64[1:], (r32[0][:, None],) + r32[1:], whole=("d_out",))
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):                   # exact zeros in the padding
        assert not got[1][b, n:].any() and not got[2][b, len(lab) + 1:].any()
    dW, db = got[3][:J * V].view(J, V), got[3][J * V:]
    if variant == "blank masked":                                                # a batch with no mass moves no weight
        assert torch.isposinf(got[0]).all() and not got[1].any() and not got[2].any() and not got[3].any()
    else:                                                                        # a masked class: no mass, no gradient, in W's column and in b
        assert not dW[:, c["mask"]].any() and not db[c["mask"]].any() and dW.any() and db.any()
    assert _equal(_fused(gpu, enc, pred, c), got)
    assert _equal(_fused(gpu, enc, pred, c, want_grad=False), (got[0], None, None, None))
    if variant == "blank masked":
        return
    # the stored loss on logits made by the library's own joiner and a float32 matmul with the same bias: a NaN (or anything else)
    # leaking out of the running log-sum-exp would part the two
    z = NL.rnnt_joint_device(torch.from_numpy(enc).to(gpu), torch.from_numpy(pred).to(gpu), c["kind"]).cpu()
    W, bias = torch.from_numpy(c["out"][:J * V]).view(J, V), torch.from_numpy(c["out"][J * V:])
    logits = (torch.nan_to_num(z, nan=0.0) @ W + bias).numpy()
    assert logits.dtype == np.float32 and np.isneginf(logits[..., c["mask"]]).all() and np.isfinite(np.delete(logits, c["mask"], -1)).all()
    stored, _ = _stored(gpu, K.with_nan_padding(dict(c, x=logits)), c, want_grad=False)
    for b in range(3):
        d = abs(float(got[0][b]) - float(stored[b])) / r64[0][b]
        e32 = abs(r32[0][b] - r64[0][b]) / r64[0][b]
        print("%s row %d: fused %.9g, stored on the library's logits %.9g: difference %.2e, torch f32 err %.2e" % (c["name"], b, got[0][b], stored[b], d, e32))
        assert d <= max(K.FACTOR * e32, K.FLOOR), (c["name"], b, d, e32)
