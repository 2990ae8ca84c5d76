"""Training a bidirectional GRU / LSTM / RNN layer in one call per pass (*BidirectionalApplyTrainingBatch[Device],
*BidirectionalCalculateGradient[Device]) and the device forms of the bidirectional gradient helpers, through the C boundary.

References: the recipe composed from the existing device calls on twin handles (bits), a masked torch float64 loop with autograd over both
directions, numpy statements of the helpers' formulas (bits).  Tolerances are the project's own (tests/test_gpu_training.py,
tests/test_gpu_train_varlen.py): forward rtol 2e-5 / atol 2e-6, gradients 2e-7 sqrt(B T) max(1, |ref|max); the sum-merged output and d_X
add two such terms and get twice that bound."""
import ctypes as C

import numpy as np
import pytest

from nntoolkitcore_amd import capi, layers as NL

pytestmark = pytest.mark.gpu
P = lambda a: None if a is None else a.ctypes.data_as(capi.fp)
IP = lambda a: None if a is None else a.ctypes.data_as(capi.ip)
dp = lambda t: C.c_void_p(t.data_ptr())
NG = {"gru": 3, "lstm": 4, "rnn": 1}
MERGE = {"concat": 0, "sum": 1}
SENTINEL = 7.0

# (B, T, in, H): register-resident forward + persistent BPTT, B not a multiple of 16 | three 16-row tiles | H not a multiple of 16 (per-step
# kernels) and widths that are no multiple of 4 (the scalar forms of the data-movement kernels)
SHAPES = [(20, 9, 16, 64), (37, 12, 40, 64), (5, 7, 6, 12)]
CASES = [(k, m, s) + sh for k in ("gru", "lstm", "rnn") for m in ("concat", "sum") for s in (True, False) for sh in SHAPES]
IDS = ["%s-%s-%s-B%d-T%d-in%d-H%d" % (k, m, "seq" if s else "last", B, T, i, H) for k, m, s, B, T, i, H in CASES]
cases = pytest.mark.parametrize("kind,merge,seq,B,T,n_in,H", CASES, ids=IDS)


def u(r, *shape, sc=1.0):
    return r.uniform(-sc, sc, shape).astype(np.float32)


def lengths_for(B, T, seed):
    """T, 0, 1, T in the first four rows; above 16 rows one 16-row tile whose rows are all shorter than T; the rest a random draw"""
    r = np.random.default_rng(seed)
    ln = r.integers(0, T + 1, B).astype(np.int32)
    ln[:3] = (T, 0, 1)
    if B > 16:
        ln[16:32] = r.integers(0, T, min(16, B - 16))
    if B > 3:
        ln[3] = T
    return ln


class Dir:
    """one direction: a training handle with fixed random weights (default activations)"""

    def __init__(self, kind, B, T, n_in, H, seq, seed, train=True):
        L = self.L = capi.load()
        self.kind, self.B, self.T, self.n_in, self.H, self.seq = kind, B, T, n_in, H, seq
        g = NG[kind]
        r = np.random.default_rng(seed)
        self.W, self.U = u(r, n_in, g * H, sc=n_in ** -0.5), u(r, H, g * H, sc=H ** -0.5)
        self.bi, self.bh = u(r, g * H, sc=0.1), u(r, g * H, sc=0.1)
        self.tc = capi.ConvTrainingConfig(B)
        self.pre = kind.upper()
        if kind == "gru":
            self.acts = L.GRUActivationsCreateDefault(H)
            self.cfg = L.GRUConfigCreate(n_in, H, seq, T, self.acts)
        elif kind == "lstm":
            self.acts = L.LSTMActivationsCreateDefault(H)
            self.cfg = L.LSTMConfigCreate(n_in, H, seq, T, True, self.acts)
        else:
            self.acts = L.ActivationFunctionCreateTanh(H)
            self.cfg = L.RNNConfigCreate(n_in, H, seq, T, True, self.acts)
        self.h = self.f("CreateForTraining")(self.cfg, self.tc) if train else self.f("CreateForInference")(self.cfg)
        assert self.h, capi.last_error()
        w = self.f("GetWeights")(self.h).contents
        for dst, src in ((w.W, self.W), (w.U, self.U), (w.b_i, self.bi), (w.b_h, self.bh)):
            C.memmove(dst, src.ctypes.data, src.nbytes)
        self.dir_shape = (B, T, H) if seq else (B, H)
        self.nblk = self.W.size + self.U.size + 2 * g * H

    def f(self, name):
        return getattr(self.L, self.pre + name)

    def forward_dev(self, xd, yd, ln):
        """the existing unidirectional call, no states"""
        args = (None,) * 4 if self.kind == "lstm" else (None,) * 2
        assert self.f("ApplyTrainingBatchDeviceVarLen")(self.h, dp(xd), dp(yd), IP(ln), *args) == 0, capi.last_error()

    def gradient_dev(self, gd, gx, dd):
        args = (None,) * 4 if self.kind == "lstm" else (None,) * 2
        assert self.f("CalculateGradientDeviceVarLen")(self.h, dp(gd), dp(gx), dp(dd), *args) == 0, capi.last_error()

    def close(self):
        self.f("Destroy")(self.h)
        {"gru": self.L.GRUActivationsDestroy, "lstm": self.L.LSTMActivationsDestroy, "rnn": self.L.ActivationFunctionDestroy}[self.kind](self.acts)


class Pair:
    def __init__(self, kind, B, T, n_in, H, seq, merge, seed=3):
        self.fw, self.bw = Dir(kind, B, T, n_in, H, seq, seed), Dir(kind, B, T, n_in, H, seq, seed + 100)
        self.kind, self.B, self.T, self.n_in, self.H, self.seq, self.merge = kind, B, T, n_in, H, seq, merge
        self.L, self.pre, self.m = self.fw.L, self.fw.pre, MERGE[merge]
        Wd = 2 * H if merge == "concat" else H
        self.out_shape = (B, T, Wd) if seq else (B, Wd)
        self.nblk = self.fw.nblk

    def f(self, name):
        return getattr(self.L, self.pre + "Bidirectional" + name)

    def forward_dev(self, xd, ln, out=None):
        import torch
        yd = torch.full(self.out_shape, SENTINEL, device="cuda") if out is None else out
        assert self.f("ApplyTrainingBatchDevice")(self.fw.h, self.bw.h, dp(xd), dp(yd), IP(ln), self.m) == 0, capi.last_error()
        return yd

    def gradient_dev(self, dd, gf=None, gb=None):
        """(d_X, forward block, backward block) as device tensors; the blocks start from zeros unless given"""
        import torch
        gf = torch.zeros(self.nblk, device="cuda") if gf is None else gf
        gb = torch.zeros(self.nblk, device="cuda") if gb is None else gb
        gx = torch.full((self.B, self.T, self.n_in), SENTINEL, device="cuda")
        assert self.f("CalculateGradientDevice")(self.fw.h, self.bw.h, dp(gf), dp(gb), dp(gx), dp(dd)) == 0, capi.last_error()
        return gx, gf, gb

    def close(self):
        self.fw.close(); self.bw.close()


# ---- numpy statements of the data movement: L = lengths[b] (None: T) ----

def _len(ln, B, T):
    return np.full(B, T, np.int32) if ln is None else ln


def np_merge(of, obr, ln, seq, merge):
    if not seq:
        return np.concatenate([of, obr], -1) if merge == "concat" else of + obr
    B, T, H = of.shape
    out = np.zeros((B, T, 2 * H if merge == "concat" else H), np.float32)
    for b, L in enumerate(_len(ln, B, T)):
        ob = obr[b, :L][::-1]
        out[b, :L] = np.concatenate([of[b, :L], ob], -1) if merge == "concat" else of[b, :L] + ob
    return out


def np_scatter(dout, ln, H, seq, merge, reverse=True):
    fpart, bpart = (dout[..., :H], dout[..., H:]) if merge == "concat" else (dout, dout)
    if not seq:
        return np.ascontiguousarray(fpart), np.ascontiguousarray(bpart)
    B, T = dout.shape[:2]
    d_of, d_ob = np.zeros((B, T, H), np.float32), np.zeros((B, T, H), np.float32)
    for b, L in enumerate(_len(ln, B, T)):
        d_of[b, :L] = fpart[b, :L]
        d_ob[b, :L] = bpart[b, :L][::-1] if reverse else bpart[b, :L]
    return d_of, d_ob


def np_accumulate(dxf, dxbr, ln):
    B, T, _ = dxf.shape
    out = np.zeros_like(dxf)
    for b, L in enumerate(_len(ln, B, T)):
        out[b, :L] = dxf[b, :L] + dxbr[b, :L][::-1]
    return out


def _data(p, seed):
    r = np.random.default_rng(seed)
    return u(r, p.B, p.T, p.n_in), u(r, *p.out_shape)


# ---- 1. the composed recipe, bit for bit ----

def _recipe(tw, x, dout, ln):
    """bd_reverse_input_batch[_varlen]_device, the unidirectional VarLen training calls on the twin handles, numpy for split / reversal / add;
    gradient blocks from zeros"""
    import torch
    L = capi.load()
    B, T, n_in, H = tw.B, tw.T, tw.n_in, tw.H
    xd = torch.from_numpy(x).cuda()
    xr = torch.full_like(xd, SENTINEL)
    cfg_in = capi.RecurrentConfig(n_in, n_in, True, T)
    if ln is None:
        assert L.bd_reverse_input_batch_device(dp(xd), dp(xr), cfg_in, B) == 0, capi.last_error()
    else:
        assert L.bd_reverse_input_batch_varlen_device(dp(xd), dp(xr), cfg_in, B, IP(ln)) == 0, capi.last_error()
    of, obr = (torch.full(tw.fw.dir_shape, SENTINEL, device="cuda") for _ in range(2))
    tw.fw.forward_dev(xd, of, ln)
    tw.bw.forward_dev(xr, obr, ln)
    out = np_merge(of.cpu().numpy(), obr.cpu().numpy(), ln, tw.seq, tw.merge)
    d_of, d_obr = np_scatter(dout, ln, H, tw.seq, tw.merge)
    gf, gb = torch.zeros(tw.nblk, device="cuda"), torch.zeros(tw.nblk, device="cuda")
    dxf, dxb = (torch.full((B, T, n_in), SENTINEL, device="cuda") for _ in range(2))
    tw.fw.gradient_dev(gf, dxf, torch.from_numpy(d_of).cuda())
    tw.bw.gradient_dev(gb, dxb, torch.from_numpy(d_obr).cuda())
    assert L.nntk_hip_synchronize() == 0
    return out, np_accumulate(dxf.cpu().numpy(), dxb.cpu().numpy(), ln), gf.cpu().numpy(), gb.cpu().numpy(), L.nntk_hip_last_recurrent_kernel()


@cases
def test_equals_the_composed_recipe_bit_for_bit(gpu, kind, merge, seq, B, T, n_in, H):
    """output, d_X and both gradient blocks (accumulated from zeros) equal the recipe on twin handles, ragged and with lengths = NULL; the
    host-memory forms equal the device forms"""
    _assert_equals_the_recipe(kind, merge, seq, B, T, n_in, H)


# bd_train.hip:97-102 (grid_for): at most 2048 workgroups of 256 lanes, one unit (V floats) per lane and trip
BD_GRID_UNITS = 2048 * 256


def test_merge_at_grid_stride_size_equals_the_composed_recipe(gpu):
    """the forward merge kernel has no helper of its own: one bidirectional RNN layer (the cheapest cell) whose merged output has more
    four-float units than the grid has lanes"""
    B, T, n_in, H = 40, 131, 8, 404
    assert H % 4 == 0 and 2 * B * T * H // 4 == 1_058_480 > BD_GRID_UNITS == 524_288       # bd_train.hip:129-130: V = 4, no / 4 units
    _assert_equals_the_recipe("rnn", "concat", True, B, T, n_in, H)


def _assert_equals_the_recipe(kind, merge, seq, B, T, n_in, H):
    import torch
    L = capi.load()
    p, tw = Pair(kind, B, T, n_in, H, seq, merge), Pair(kind, B, T, n_in, H, seq, merge)
    x, dout = _data(p, 11)
    xd, dd = torch.from_numpy(x).cuda(), torch.from_numpy(dout).cuda()
    for ln in (lengths_for(B, T, 7), None):
        ref = _recipe(tw, x, dout, ln)
        yd = p.forward_dev(xd, ln)
        fwd_kernel = L.nntk_hip_last_recurrent_kernel()
        gx, gf, gb = p.gradient_dev(dd)
        assert L.nntk_hip_synchronize() == 0
        got = [t.cpu().numpy() for t in (yd, gx, gf, gb)]
        for nm, a, b_ in zip(("out", "dX", "forward block", "backward block"), got, ref):
            assert np.isfinite(a).all(), nm
            np.testing.assert_array_equal(a, b_, err_msg="%s (lengths %s)" % (nm, "ragged" if ln is not None else "NULL"))
        assert fwd_kernel != b"" and L.nntk_hip_last_recurrent_kernel() == ref[4]        # each direction on its unidirectional call's kernel
        # host-memory forms
        y = np.full(p.out_shape, SENTINEL, np.float32)
        assert p.f("ApplyTrainingBatch")(p.fw.h, p.bw.h, P(x), P(y), IP(ln), p.m) == 0, capi.last_error()
        g1, g2 = (p.fw.f("GradientCreate")(p.fw.cfg, p.fw.tc) for _ in range(2))
        dX = np.full(x.shape, SENTINEL, np.float32)
        assert p.f("CalculateGradient")(p.fw.h, p.bw.h, g1, g2, P(dX), P(dout)) == 0, capi.last_error()
        np.testing.assert_array_equal(y, got[0])
        np.testing.assert_array_equal(dX, got[1])
        for g, want in ((g1, got[2]), (g2, got[3])):
            np.testing.assert_array_equal(np.ctypeslib.as_array(g.contents.d_W, shape=(p.nblk,)), want)
            L.RecurrentGradientDestroy(g)
    p.close(); tw.close()


# ---- 2. float64 autograd ----

def _cell64(d, xt, msk):
    """masked float64 loop over one direction from zero state: (sequence output with zeros past a length, final state), leaves"""
    import torch
    kind, H = d.kind, d.H
    B, T = xt.shape[:2]
    leaves = [torch.tensor(v).double().requires_grad_(True) for v in (d.W, d.U, d.bi, d.bh)]
    Wt, Ut, bit, bht = leaves
    hp, cp, outs = torch.zeros(B, H).double(), torch.zeros(B, H).double(), []
    sg, th = torch.sigmoid, torch.tanh
    for t in range(T):
        m = msk[:, t:t + 1]
        xw = xt[:, t] @ Wt + bit
        if kind == "gru":
            hu = hp @ Ut + bht
            z, rr = sg(xw[:, :H] + hu[:, :H]), sg(xw[:, H:2 * H] + hu[:, H:2 * H])
            hn = (1 - z) * th(rr * hu[:, 2 * H:] + xw[:, 2 * H:]) + z * hp
        elif kind == "lstm":
            Z = xw + hp @ Ut + bht
            i, f, g_, o = sg(Z[:, :H]), sg(Z[:, H:2 * H]), th(Z[:, 2 * H:3 * H]), sg(Z[:, 3 * H:])
            cn = f * cp + i * g_
            hn = o * th(cn)
            cp = torch.where(m, cn, cp)
        else:
            hn = th(xw + hp @ Ut + bht)
        hp = torch.where(m, hn, hp)
        outs.append(torch.where(m, hn, torch.zeros_like(hn)))
    return torch.stack(outs, 1), hp, leaves


def _ref64(p, x, dout, ln):
    import torch
    B, T = p.B, p.T
    lt = torch.tensor(_len(ln, B, T).astype(np.int64))
    ar = torch.arange(T)[None, :]
    msk = ar < lt[:, None]
    idx = torch.where(msk, lt[:, None] - 1 - ar, ar)                       # the per-row reversal of the first L steps (its own inverse)
    rev = lambda v: torch.where(msk[:, :, None], v.gather(1, idx[:, :, None].expand(-1, -1, v.shape[2])), torch.zeros_like(v))
    xt = torch.tensor(np.where(msk.numpy()[:, :, None], x, 0.0)).double().requires_grad_(True)
    hf, hf_T, lf = _cell64(p.fw, xt, msk)
    hb, hb_T, lb = _cell64(p.bw, rev(xt), msk)
    a, b_ = (hf, rev(hb)) if p.seq else (hf_T, hb_T)
    out = torch.cat([a, b_], -1) if p.merge == "concat" else a + b_
    dm = np.where(msk.numpy()[:, :, None], dout, 0.0) if p.seq else dout
    (out * torch.tensor(dm).double()).sum().backward()
    blk = lambda leaves: [v.grad.numpy() for v in leaves]
    return out.detach().numpy(), xt.grad.numpy(), blk(lf), blk(lb)


@cases
def test_matches_float64_autograd(gpu, kind, merge, seq, B, T, n_in, H):
    import torch
    p = Pair(kind, B, T, n_in, H, seq, merge)
    x, dout = _data(p, 21)
    ln = lengths_for(B, T, 8)
    yd = p.forward_dev(torch.from_numpy(x).cuda(), ln)
    gx, gf, gb = p.gradient_dev(torch.from_numpy(dout).cuda())
    assert capi.load().nntk_hip_synchronize() == 0
    ref_out, ref_dx, ref_f, ref_b = _ref64(p, x, dout, ln)
    k = 2.0 if merge == "sum" else 1.0
    y = yd.cpu().numpy()
    print("%s forward: max abs err %.2e" % (kind, float(np.abs(y - ref_out).max())))
    np.testing.assert_allclose(y, ref_out, rtol=k * 2e-5, atol=k * 2e-6)
    tol = 2e-7 * np.sqrt(B * T)

    def check(tag, a, b_, factor):
        sc = max(1.0, float(np.abs(b_).max()))
        err = float(np.abs(a - b_).max())
        print("%s %s: %.2e (scale %.1f, bound %.2e)" % (kind, tag, err, sc, factor * tol * sc))
        assert np.isfinite(a).all() and err <= factor * tol * sc, (tag, err, factor * tol * sc)

    check("dX", gx.cpu().numpy(), ref_dx, 2.0)
    d = p.fw
    sizes = (d.W.size, d.U.size, d.bi.size, d.bh.size)
    for side, blk, ref in (("forward", gf.cpu().numpy(), ref_f), ("backward", gb.cpu().numpy(), ref_b)):
        for nm, part, r_ in zip(("dW", "dU", "dbi", "dbh"), np.split(blk, np.cumsum(sizes)[:-1]), ref):
            check("%s %s" % (side, nm), part, r_.ravel(), 1.0)
    p.close()


# ---- 3. padding cannot leak ----

@cases
def test_padding_cannot_leak(gpu, kind, merge, seq, B, T, n_in, H):
    """x[b][t >= L] and d_dout[b][t >= L] NaN against zeros, output and d_X pre-filled with a sentinel: every bit equal, finite, and rows
    t >= L of the output and d_X exact zeros"""
    import torch
    p = Pair(kind, B, T, n_in, H, seq, merge)
    x, dout = _data(p, 31)
    ln = lengths_for(B, T, 9)
    pad = np.arange(T)[None, :] >= ln[:, None]
    runs = []
    for fill in (0.0, np.nan):
        xf, df = x.copy(), dout.copy()
        xf[pad] = fill
        if seq:
            df[pad] = fill
        yd = p.forward_dev(torch.from_numpy(xf).cuda(), ln)
        gx, gf, gb = p.gradient_dev(torch.from_numpy(df).cuda())
        assert capi.load().nntk_hip_synchronize() == 0
        runs.append([t.cpu().numpy() for t in (yd, gx, gf, gb)])
    for nm, a, b_ in zip(("out", "dX", "forward block", "backward block"), *runs):
        assert np.isfinite(b_).all(), nm
        np.testing.assert_array_equal(a, b_, err_msg=nm)
    if seq:
        assert not runs[1][0][pad].any()
    assert not runs[1][1][pad].any()
    p.close()


# ---- 4. accumulation ----

@cases
def test_second_gradient_call_accumulates(gpu, kind, merge, seq, B, T, n_in, H):
    """a second call onto the same zero-initialised blocks: exactly twice the first call's values, d_X unchanged"""
    import torch
    p = Pair(kind, B, T, n_in, H, seq, merge)
    x, dout = _data(p, 41)
    ln = lengths_for(B, T, 10)
    dd = torch.from_numpy(dout).cuda()
    p.forward_dev(torch.from_numpy(x).cuda(), ln)
    gx1, gf, gb = p.gradient_dev(dd)
    first = [t.clone() for t in (gx1, gf, gb)]
    gx2, gf, gb = p.gradient_dev(dd, gf, gb)
    assert capi.load().nntk_hip_synchronize() == 0
    assert first[1].abs().max() > 0 and first[2].abs().max() > 0
    np.testing.assert_array_equal(gf.cpu().numpy(), 2 * first[1].cpu().numpy())
    np.testing.assert_array_equal(gb.cpu().numpy(), 2 * first[2].cpu().numpy())
    np.testing.assert_array_equal(gx2.cpu().numpy(), first[0].cpu().numpy())
    p.close()


# ---- 5. argument errors write nothing ----

@pytest.mark.parametrize("kind", ["gru", "lstm", "rnn"])
def test_argument_errors_write_nothing(gpu, kind):
    import torch
    L = capi.load()
    B, T, n_in, H = 5, 7, 6, 12
    p = Pair(kind, B, T, n_in, H, True, "concat")
    x, dout = _data(p, 51)
    xd, dd = torch.from_numpy(x).cuda(), torch.from_numpy(dout).cuda()
    yd = torch.full(p.out_shape, SENTINEL, device="cuda")
    gf, gb = torch.full((p.nblk,), SENTINEL, device="cuda"), torch.full((p.nblk,), SENTINEL, device="cuda")
    gx = torch.full((B, T, n_in), SENTINEL, device="cuda")
    fwd, grad = p.f("ApplyTrainingBatchDevice"), p.f("CalculateGradientDevice")

    def refused(rc, what):
        assert rc == -1, what
        assert capi.last_error() != "", what
        assert L.nntk_hip_synchronize() == 0
        for t in (yd, gf, gb, gx):
            assert bool((t == SENTINEL).all()), what + ": something was written"

    ok = lengths_for(B, T, 3)
    # a gradient call before any bidirectional forward on this pair
    refused(grad(p.fw.h, p.bw.h, dp(gf), dp(gb), dp(gx), dp(dd)), "gradient without a forward")
    inf = Dir(kind, B, T, n_in, H, True, 1, train=False)
    others = {"input size": Dir(kind, B, T, n_in + 2, H, True, 1), "hidden size": Dir(kind, B, T, n_in, H + 4, True, 1),
              "timesteps": Dir(kind, B, T + 1, n_in, H, True, 1), "return_sequences": Dir(kind, B, T, n_in, H, False, 1),
              "mini_batch_size": Dir(kind, B + 1, T, n_in, H, True, 1)}
    big_x = torch.zeros((B + 1) * (T + 1) * (n_in + 2), device="cuda")        # large enough for every mismatching handle's idea of the input

    def forward_errors():
        refused(fwd(None, p.bw.h, dp(xd), dp(yd), IP(ok), 0), "NULL forward handle")
        refused(fwd(p.fw.h, None, dp(xd), dp(yd), IP(ok), 0), "NULL backward handle")
        refused(fwd(inf.h, p.bw.h, dp(xd), dp(yd), IP(ok), 0), "inference forward handle")
        refused(fwd(p.fw.h, inf.h, dp(xd), dp(yd), IP(ok), 0), "inference backward handle")
        refused(fwd(p.fw.h, p.fw.h, dp(xd), dp(yd), IP(ok), 0), "the same handle twice")
        for what, d in others.items():
            refused(fwd(p.fw.h, d.h, dp(big_x), dp(yd), IP(ok), 0), "handles differ in " + what)
            refused(fwd(d.h, p.bw.h, dp(big_x), dp(yd), IP(ok), 0), "handles differ in " + what)
        for bad in (-1, T + 1):
            ln = ok.copy()
            ln[2] = bad
            refused(fwd(p.fw.h, p.bw.h, dp(xd), dp(yd), IP(ln), 0), "length %d" % bad)
        for m in (-1, 2):
            refused(fwd(p.fw.h, p.bw.h, dp(xd), dp(yd), IP(ok), m), "merge %d" % m)
        refused(fwd(p.fw.h, p.bw.h, None, dp(yd), IP(ok), 0), "NULL input")
        refused(fwd(p.fw.h, p.bw.h, dp(xd), None, IP(ok), 0), "NULL output")
        both = torch.full((x.size + B * T * 2 * H,), SENTINEL, device="cuda")
        rc = fwd(p.fw.h, p.bw.h, dp(both), C.c_void_p(both.data_ptr() + 4 * (x.size - 4)), IP(ok), 0)
        refused(rc, "output overlapping the input")
        assert bool((both == SENTINEL).all())

    forward_errors()
    # still no forward: the refused calls must not have left a remembered batch behind
    refused(grad(p.fw.h, p.bw.h, dp(gf), dp(gb), dp(gx), dp(dd)), "gradient after refused forwards only")
    # a good forward, then every refused call again: the remembered state must survive them
    out = p.forward_dev(xd, ok)
    want = [t.clone() for t in p.gradient_dev(dd)]
    forward_errors()
    refused(grad(None, p.bw.h, dp(gf), dp(gb), dp(gx), dp(dd)), "NULL handle")
    refused(grad(p.fw.h, p.fw.h, dp(gf), dp(gb), dp(gx), dp(dd)), "the same handle twice")
    refused(grad(p.bw.h, p.fw.h, dp(gf), dp(gb), dp(gx), dp(dd)), "the pair in the other order")
    refused(grad(p.fw.h, inf.h, dp(gf), dp(gb), dp(gx), dp(dd)), "inference handle")
    refused(grad(p.fw.h, others["hidden size"].h, dp(gf), dp(gb), dp(gx), dp(dd)), "another handle")
    refused(grad(p.fw.h, p.bw.h, None, dp(gb), dp(gx), dp(dd)), "NULL block")
    refused(grad(p.fw.h, p.bw.h, dp(gf), dp(gf), dp(gx), dp(dd)), "one block for both directions")
    refused(grad(p.fw.h, p.bw.h, dp(gf), dp(gb), dp(gf), dp(dd)), "d_dX inside a gradient block")
    refused(grad(p.fw.h, p.bw.h, dp(gf), dp(gb), dp(gx), None), "NULL d_dout")
    again = p.gradient_dev(dd)
    assert L.nntk_hip_synchronize() == 0
    for a, b_ in zip(want, again):
        assert torch.equal(a, b_), "a refused call changed what the pair remembers"
    # a unidirectional forward on one of the handles ends the pairing
    p.bw.forward_dev(xd, torch.empty(p.bw.dir_shape, device="cuda"), ok)
    refused(grad(p.fw.h, p.bw.h, dp(gf), dp(gb), dp(gx), dp(dd)), "gradient after a unidirectional forward on the backward handle")
    # the host-memory forms refuse the same way
    y = np.full(p.out_shape, SENTINEL, np.float32)
    assert p.f("ApplyTrainingBatch")(p.fw.h, p.fw.h, P(x), P(y), IP(ok), 0) == -1 and capi.last_error() != ""
    ln = ok.copy()
    ln[0] = T + 1
    assert p.f("ApplyTrainingBatch")(p.fw.h, p.bw.h, P(x), P(y), IP(ln), 0) == -1 and capi.last_error() != ""
    assert (y == SENTINEL).all()
    del out
    inf.close()
    for d in others.values():
        d.close()
    p.close()


# ---- 6. the helpers ----

@pytest.mark.parametrize("B,T,n_in,H", [(3, 5, 6, 12), (4, 8, 16, 32)])
@pytest.mark.parametrize("seq", [True, False])
def test_fixed_length_helpers_equal_the_host_forms(gpu, B, T, n_in, H, seq):
    import torch
    L = capi.load()
    r = np.random.default_rng(61)
    cfg = capi.RecurrentConfig(n_in, H, seq, T)
    rows = (B, T) if seq else (B,)
    dout2, dout1 = u(r, *rows, 2 * H), u(r, *rows, H)
    dev = lambda a: torch.from_numpy(a).cuda()
    # concat
    hf, hb = np.full(rows + (H,), SENTINEL, np.float32), np.full(rows + (H,), SENTINEL, np.float32)
    L.bd_merge_concat_gradient(P(dout2), P(hf), P(hb), cfg, B, None)
    assert capi.last_error() == ""
    df, db = torch.full(rows + (H,), SENTINEL, device="cuda"), torch.full(rows + (H,), SENTINEL, device="cuda")
    assert L.bd_merge_concat_gradient_device(dp(dev(dout2)), dp(df), dp(db), cfg, B) == 0, capi.last_error()
    np.testing.assert_array_equal(df.cpu().numpy(), hf)
    np.testing.assert_array_equal(db.cpu().numpy(), hb)
    np.testing.assert_array_equal(hb, dout2[..., H:])                        # not reversed: the reference's contract
    # sum
    L.bd_merge_sum_gradient(P(dout1), P(hf), P(hb), cfg, B)
    df.fill_(SENTINEL); db.fill_(SENTINEL)
    assert L.bd_merge_sum_gradient_device(dp(dev(dout1)), dp(df), dp(db), cfg, B) == 0, capi.last_error()
    np.testing.assert_array_equal(df.cpu().numpy(), hf)
    np.testing.assert_array_equal(db.cpu().numpy(), hb)
    # accumulate (always over [B][T][in])
    fx, bx = u(r, B, T, n_in), u(r, B, T, n_in)
    ho = np.full((B, T, n_in), SENTINEL, np.float32)
    L.bd_accumulate_d_x(P(fx), P(bx), P(ho), cfg, B)
    assert capi.last_error() == ""
    do = torch.full((B, T, n_in), SENTINEL, device="cuda")
    assert L.bd_accumulate_d_x_device(dp(dev(fx)), dp(dev(bx)), dp(do), cfg, B) == 0, capi.last_error()
    np.testing.assert_array_equal(do.cpu().numpy(), ho)
    np.testing.assert_array_equal(ho, fx + bx[:, ::-1])


@pytest.mark.parametrize("B,T,n_in,H", [(5, 7, 6, 12), (20, 9, 16, 64), (3, 5, 6, 12)])
@pytest.mark.parametrize("merge", ["concat", "sum"])
@pytest.mark.parametrize("seq", [True, False])
def test_varlen_helpers_equal_their_formulas(gpu, B, T, n_in, H, merge, seq):
    """against the numpy statement, NaN in the ignored region, exact zeros past L; lengths NULL = every row T"""
    import torch
    L = capi.load()
    cfg = capi.RecurrentConfig(n_in, H, seq, T)
    _assert_varlen_helpers(B, T, n_in, H, merge, seq)
    # refused before anything is written
    ln = lengths_for(B, T, 5).copy()
    ln[0] = T + 1
    do = torch.full((B, T, n_in), SENTINEL, device="cuda")
    assert L.bd_accumulate_d_x_varlen_device(dp(do), dp(do), dp(do), cfg, B, IP(ln)) == -1 and capi.last_error() != ""
    assert L.bd_merge_gradient_varlen_device(dp(do), dp(do), dp(do), cfg, B, None, 3) == -1 and capi.last_error() != ""
    assert bool((do == SENTINEL).all())


def _assert_varlen_helpers(B, T, n_in, H, merge, seq, accumulate=True):
    import torch
    L = capi.load()
    r = np.random.default_rng(71)
    cfg = capi.RecurrentConfig(n_in, H, seq, T)
    Wd = 2 * H if merge == "concat" else H
    dev = lambda a: torch.from_numpy(a).cuda()
    for ln in (lengths_for(B, T, 5), None):
        pad = np.arange(T)[None, :] >= _len(ln, B, T)[:, None]
        dout = u(r, *((B, T, Wd) if seq else (B, Wd)))
        if seq:
            dout[pad] = np.nan
        shape = (B, T, H) if seq else (B, H)
        df, db = torch.full(shape, SENTINEL, device="cuda"), torch.full(shape, SENTINEL, device="cuda")
        dd = dev(dout)                                   # (named: a temporary's memory would be free again before the call)
        assert L.bd_merge_gradient_varlen_device(dp(dd), dp(df), dp(db), cfg, B, IP(ln), MERGE[merge]) == 0, capi.last_error()
        wf, wb = np_scatter(dout, ln, H, seq, merge)
        np.testing.assert_array_equal(df.cpu().numpy(), wf)
        np.testing.assert_array_equal(db.cpu().numpy(), wb)
        if seq:
            assert not df.cpu().numpy()[pad].any() and not db.cpu().numpy()[pad].any()
        if not accumulate:
            continue
        fx, bx = u(r, B, T, n_in), u(r, B, T, n_in)
        fx[pad] = np.nan
        bx[pad] = np.nan
        do = torch.full((B, T, n_in), SENTINEL, device="cuda")
        dfx, dbx = dev(fx), dev(bx)
        assert L.bd_accumulate_d_x_varlen_device(dp(dfx), dp(dbx), dp(do), cfg, B, IP(ln)) == 0, capi.last_error()
        got = do.cpu().numpy()
        np.testing.assert_array_equal(got, np_accumulate(fx, bx, ln))
        assert np.isfinite(got).all() and not got[pad].any()


@pytest.mark.parametrize("width", [404, 403], ids=["V4", "V1"])
@pytest.mark.parametrize("merge", ["concat", "sum"])
def test_varlen_helpers_past_one_trip_of_the_grid(gpu, width, merge):
    """more units than the grid has lanes: the second trip of the scatter's and the accumulation's grid-stride loops, in the four-float
    form (width 404) and the scalar form (403), ragged and with lengths NULL.  The final-state scatter (seq = False) runs at the same
    widths too; its 16,160 floats stay inside the first trip"""
    B, T = 40, 131
    n = B * T * width
    if width % 4 == 0:
        assert n == 2_116_960 and n // 4 == 529_240 > BD_GRID_UNITS          # bd_train.hip:145-146 and :160-161: V = 4, n / 4 units
    else:
        assert n > BD_GRID_UNITS                                              # bd_train.hip:149 and :163: V = 1, n units
    _assert_varlen_helpers(B, T, width, width, merge, True)
    _assert_varlen_helpers(B, T, width, width, merge, False, accumulate=False)


def _off16(n, tail=0, fill=SENTINEL):
    """a tensor of n floats that starts 4 bytes past a 16-byte boundary: (the view, its buffer with one word before and `tail` behind)"""
    import torch
    buf = torch.full((n + 1 + tail,), fill, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[1:n + 1]
    assert view.data_ptr() % 16 == 4
    return view, buf


def test_misaligned_pointers_at_widths_that_are_multiples_of_4(gpu):
    """H = 12 and F = 8 would take the 16-byte form; at pointers 4 bytes past a 16-byte boundary the shim must fall back to the scalar one
    (bd_train.hip:104, aligned16).  Same bits as the aligned call, and the words around the views keep their sentinels"""
    import torch
    L = capi.load()
    B, T, n_in, H = 5, 7, 8, 12
    assert H % 4 == 0 and n_in % 4 == 0
    r = np.random.default_rng(81)
    ln = lengths_for(B, T, 5)
    pad = np.arange(T)[None, :] >= ln[:, None]
    cfg = capi.RecurrentConfig(n_in, H, True, T)
    for merge in ("concat", "sum"):
        dout = u(r, B, T, 2 * H if merge == "concat" else H)
        dout[pad] = np.nan
        dd = torch.from_numpy(dout).cuda()
        df, db = (torch.full((B, T, H), SENTINEL, device="cuda") for _ in range(2))
        assert L.bd_merge_gradient_varlen_device(dp(dd), dp(df), dp(db), cfg, B, IP(ln), MERGE[merge]) == 0, capi.last_error()
        (mdd, bdd), (mdf, bdf), (mdb, bdb) = _off16(dout.size), _off16(B * T * H, 1), _off16(B * T * H, 1)
        mdd.copy_(dd.reshape(-1))
        assert L.bd_merge_gradient_varlen_device(dp(mdd), dp(mdf), dp(mdb), cfg, B, IP(ln), MERGE[merge]) == 0, capi.last_error()
        wf, wb = np_scatter(dout, ln, H, True, merge)
        np.testing.assert_array_equal(df.cpu().numpy(), wf)
        np.testing.assert_array_equal(db.cpu().numpy(), wb)
        assert torch.equal(mdf, df.reshape(-1)) and torch.equal(mdb, db.reshape(-1)), merge
        assert float(bdd[0]) == SENTINEL and all(float(b_[0]) == SENTINEL and float(b_[-1]) == SENTINEL for b_ in (bdf, bdb)), merge
    fx, bx = u(r, B, T, n_in), u(r, B, T, n_in)
    fx[pad] = np.nan
    bx[pad] = np.nan
    do = torch.full((B, T, n_in), SENTINEL, device="cuda")
    dfx, dbx = torch.from_numpy(fx).cuda(), torch.from_numpy(bx).cuda()
    assert L.bd_accumulate_d_x_varlen_device(dp(dfx), dp(dbx), dp(do), cfg, B, IP(ln)) == 0, capi.last_error()
    (mfx, bfx), (mbx, bbx), (mdo, bdo) = _off16(fx.size), _off16(bx.size), _off16(fx.size, 1)
    mfx.copy_(torch.from_numpy(fx).reshape(-1)); mbx.copy_(torch.from_numpy(bx).reshape(-1))
    assert L.bd_accumulate_d_x_varlen_device(dp(mfx), dp(mbx), dp(mdo), cfg, B, IP(ln)) == 0, capi.last_error()
    np.testing.assert_array_equal(do.cpu().numpy(), np_accumulate(fx, bx, ln))
    assert torch.equal(mdo, do.reshape(-1))
    assert float(bfx[0]) == SENTINEL and float(bbx[0]) == SENTINEL and float(bdo[0]) == SENTINEL and float(bdo[-1]) == SENTINEL
    # the forward merge: its inputs are the handles' own scratch, the output is the caller's
    for merge in ("concat", "sum"):
        p = Pair("rnn", B, T, n_in, H, True, merge)
        xd = torch.from_numpy(u(r, B, T, n_in)).cuda()
        y = p.forward_dev(xd, ln)
        my, by = _off16(y.numel(), 1)
        p.forward_dev(xd, ln, out=my)
        assert L.nntk_hip_synchronize() == 0
        assert torch.equal(my, y.reshape(-1)) and float(by[0]) == SENTINEL and float(by[-1]) == SENTINEL, merge
        p.close()


def test_accumulate_with_64_bit_indices(gpu):
    """2049 x 1024 x 1024 floats reach 2^31: the kernel<V, long> instantiation (bd_train.hip:111).  Small integers, so every sum is
    exact; filled, run (over d_dxf, which the shim allows) and checked on the device in slices of 64 rows: 16 GiB at the peak"""
    import torch
    L = capi.load()
    B, T, F = 2049, 1024, 1024
    assert B * T * F == 2_148_532_224 >= 2 ** 31 and F % 4 == 0
    ln = lengths_for(B, T, 13)
    ln[-3:] = (T, 0, 1)                                   # (row 2048 is the one whose floats lie past 2^31)
    assert tuple(ln[:3]) == (T, 0, 1)
    dev = torch.device("cuda")
    tt, ff = torch.arange(T, device=dev, dtype=torch.int32)[None, :, None], torch.arange(F, device=dev, dtype=torch.int32)[None, None, :]
    fval = lambda bb, t_: ((bb * 3 + t_ * 5 + ff) % 17 - 8).float()
    bval = lambda bb, t_: ((bb * 7 + t_ * 11 + ff * 3) % 19 - 9).float()
    dxf, dxb = torch.empty((B, T, F), device=dev), torch.empty((B, T, F), device=dev)
    lens = torch.from_numpy(ln).to(dev)
    slices = [(b0, min(b0 + 64, B)) for b0 in range(0, B, 64)]
    nan = torch.tensor(float("nan"), device=dev)
    for b0, b1 in slices:
        bb, live = torch.arange(b0, b1, device=dev, dtype=torch.int32)[:, None, None], tt < lens[b0:b1, None, None]
        dxf[b0:b1] = torch.where(live, fval(bb, tt), nan)             # NaN in the ignored region
        dxb[b0:b1] = torch.where(live, bval(bb, tt), nan)
    cfg = capi.RecurrentConfig(F, F, True, T)
    assert L.bd_accumulate_d_x_varlen_device(dp(dxf), dp(dxb), dp(dxf), cfg, B, IP(ln)) == 0, capi.last_error()
    assert L.nntk_hip_synchronize() == 0
    for b0, b1 in slices:
        bb, Lr = torch.arange(b0, b1, device=dev, dtype=torch.int32)[:, None, None], lens[b0:b1, None, None]
        want = torch.where(tt < Lr, fval(bb, tt) + bval(bb, (Lr - 1 - tt).clamp(min=0)), torch.zeros((), device=dev))
        assert torch.equal(dxf[b0:b1], want), "rows %d..%d" % (b0, b1 - 1)
    del dxf, dxb, want
    torch.cuda.empty_cache()


# ---- 7. a whole step learns ----

B7, T7, IN7, H7, V7 = 8, 12, 16, 32, 6
N_DIR, N_TDD = IN7 * 4 * H7 + H7 * 4 * H7 + 8 * H7, 2 * H7 * V7 + V7


def _train(gpu, steps=40):
    """BiLSTM (concat, ragged) -> softmax TimeDistributedDense -> CTC under the library's Adam: the mean loss before every step and
    after the last one"""
    import torch
    L = capi.load()
    rng = np.random.default_rng(17)
    x = torch.from_numpy(rng.uniform(-1, 1, (B7, T7, IN7)).astype(np.float32)).to(gpu)
    ln = np.array([12, 9, 12, 7, 10, 12, 8, 11], np.int32)
    labels = [list(rng.integers(1, V7, rng.integers(1, 4))) for _ in range(B7)]        # fixed random labels, length 1..3, blank = 0
    w = [torch.from_numpy(rng.uniform(-0.3, 0.3, n).astype(np.float32)).to(gpu) for n in (N_DIR, N_DIR, N_TDD)]
    g = [torch.zeros_like(t) for t in w]
    fw, bw = NL.LSTM(IN7, H7, True, T7, mini_batch=B7), NL.LSTM(IN7, H7, True, T7, mini_batch=B7)
    soft = L.ActivationFunctionCreateSoftmax(1, V7)
    tdd = L.TimeDistributedDenseCreateForTraining(L.TimeDistributedDenseConfigCreate(T7, L.DenseConfigCreate(2 * H7, V7, soft)),
                                                  capi.ConvTrainingConfig(B7))
    assert fw.h and bw.h and tdd, capi.last_error()
    opt = NL.Optimizer("adam", list(zip(w, g)), zero_gradients=1, learning_rate=0.02, clip_norm=1.0, grad_scale=1.0 / B7)

    def load():
        fw.load_weights_device(w[0]); bw.load_weights_device(w[1])
        assert L.TimeDistributedDenseLoadWeightsDevice(tdd, dp(w[2])) == 0, capi.last_error()

    load()
    probs, dh = torch.empty(B7, T7, V7, device=gpu), torch.empty(B7, T7, 2 * H7, device=gpu)
    losses = []
    for step in range(steps + 1):                   # the last round only measures the loss after the last step
        h = NL.bidirectional_train_forward_device(fw, bw, x, lengths=ln, merge="concat")
        assert L.TimeDistributedDenseApplyTrainingBatchDevice(tdd, dp(h), dp(probs)) == 0, capi.last_error()
        loss, dprobs = NL.ctc_loss_device(probs, labels, input_lengths=ln)
        losses.append(loss.mean())
        if step == steps:
            break
        assert L.TimeDistributedDenseCalculateGradientDevice(tdd, dp(g[2]), dp(dh), dp(dprobs)) == 0, capi.last_error()
        NL.bidirectional_train_backward_device(fw, bw, dh, g[0], g[1])
        opt.step()
        load()
    info = opt.info()
    assert info[3] == steps and info[2] == 0.0, info
    losses = [float(v) for v in torch.stack(losses).cpu()]
    opt.destroy(); fw.destroy(); bw.destroy()
    L.TimeDistributedDenseDestroy(tdd); L.ActivationFunctionDestroy(soft)
    return losses


def test_a_whole_step_learns(gpu):
    a, b_ = _train(gpu), _train(gpu)
    print("mean CTC loss: first %.4f, last %.4f" % (a[0], a[-1]))
    assert np.isfinite(a).all()
    assert a[-1] < a[0]
    assert a == b_, "two runs from the same seed differ"
