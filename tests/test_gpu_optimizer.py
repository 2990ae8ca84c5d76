"""The device-side optimizer (csrc/hip/optim.hip, nntk_optimizer_*) and <Layer>LoadWeightsDevice.

Reference: torch.optim.SGD / Adam / AdamW plus torch.nn.utils.clip_grad_norm_ in float64 on the CPU, fed the float32 gradients the library
receives and the hyper-parameters rounded to float32 (what the C struct holds).

Block set: eleven blocks of 1, 0, 3, 4, 5, 255, 256, 257, 4099, 65537 and 2^20 + 3 floats carved from one allocation, the block pointers at
every 16-byte phase (and the gradient pointers at phases that partly differ from their weights'), every word outside a block a sentinel.

A second set (5, 6 000 003, 0, 4099 and 3 000 001 floats, laid out the same way) has more chunks than either pass has workgroups; a third
(67 108 864 + 4099 and 5 floats) is past the size at which the chunk doubles, and is checked on the device.

Tolerance (per element): |library - float64| <= FACTOR x (the largest error of torch's own float32 CPU optimizer against float64 on the same
inputs, over all elements) + one float32 ulp of the weight.  The issue allows FACTOR = 4.
Measured on an MI355X (12 steps; library error / torch float32 error, both against float64): ratio 1.00 in all twelve cases (errors
1.1e-6 .. 4.1e-6; DESIGN.md "Optimizer"): the kernel rounds where PyTorch's single-tensor CPU path rounds.
Measured on an MI355X at the large sets: the 2201-chunk set (Adam, scaled and clipped, 3 steps) library error 6.4e-7 against torch float32's
5.9e-7, ratio 1.09; the 8192-float-chunk set (SGD) norm within 4e-8 relative of the float64 sum in both steps, clip factor 0.499999762
against 0.499999766, largest weight error 0.500 ulp (the bound is 1)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from nntoolkitcore_amd import capi, layers as NL

pytestmark = pytest.mark.gpu

FACTOR = 4.0
SIZES = (1, 0, 3, 4, 5, 255, 256, 257, 4099, 65537, 2 ** 20 + 3)
STEPS = 12
SENTINEL = -7.0e-33
f32 = lambda v: float(np.float32(v))


def _layout(phases, sizes=SIZES):
    """offsets of the blocks in one buffer: at least four sentinel words before each block, block i at 16-byte phase phases[i]"""
    offs, cur = [], 0
    for n, ph in zip(sizes, phases):
        o = ((cur + 3) // 4) * 4 + 4 + ph
        offs.append(o)
        cur = o + n
    return offs, ((cur + 3) // 4) * 4 + 8


_w_phases = lambda n: [(3 * i) % 4 for i in range(n)]                 # 0 3 2 1 0 ...
_g_phases = lambda n: [(3 * i + (i % 2)) % 4 for i in range(n)]       # equal to the weights' phase for even i, different for odd i


# the second block set: more chunks than pass 1 and pass 2 have workgroups, so their grid-stride loops make a second trip
BIG_SIZES = (5, 6_000_003, 0, 4_099, 3_000_001)
BIG_STEPS = 3
OPT_CHUNK, OPT_MAX_CHUNKS, OPT_MAX_GRID = 4096, 16384, 2048       # optim.hip:223, :224 and :29


def _chunk_floats(total):
    ch = OPT_CHUNK                                                # optim.hip:222-226 (nntk_shim_optim_chunk_floats)
    while total // ch > OPT_MAX_CHUNKS and ch < 2 ** 30:
        ch *= 2
    return ch


def _n_chunks(sizes, phases):
    ch = _chunk_floats(sum(sizes))
    return sum((ph + n + ch - 1) // ch for n, ph in zip(sizes, phases) if n)     # train.c:238 (nntk_optimizer_create)


def _make_inputs(sizes, steps):
    """initial weights and steps + 1 gradient sets (CPU float32)"""
    gen = torch.Generator().manual_seed(2024)
    w0 = [torch.randn(n, generator=gen) for n in sizes]
    grads = [[torch.randn(n, generator=gen) * (1e-3 * (1 + t % 3)) for n in sizes] for t in range(steps + 1)]
    return w0, grads


@functools.lru_cache(None)
def _inputs():
    """the SIZES set: shared by every test and never modified (the large set is made where it is used and not kept)"""
    return _make_inputs(SIZES, STEPS)


class Buffers:
    """the weights and gradient allocations on the GPU with their sentinels; the weights are w0 (default: the SIZES set's), or with
    fill = False left to the caller"""

    def __init__(self, gpu, sizes=SIZES, w0=None, w_ph=None, g_ph=None, fill=True):
        if fill and w0 is None:
            assert sizes == SIZES
            w0, _ = _inputs()
        self.w_ph = _w_phases(len(sizes)) if w_ph is None else w_ph
        self.g_ph = _g_phases(len(sizes)) if g_ph is None else g_ph
        w_off, w_len = _layout(self.w_ph, sizes)
        g_off, g_len = _layout(self.g_ph, sizes)
        self.W = torch.full((w_len,), SENTINEL, device=gpu)
        self.G = torch.full((g_len,), SENTINEL, device=gpu)
        assert self.W.data_ptr() % 16 == 0 and self.G.data_ptr() % 16 == 0
        self.w = [self.W[o:o + n] for o, n in zip(w_off, sizes)]
        self.g = [self.G[o:o + n] for o, n in zip(g_off, sizes)]
        for t, ph in list(zip(self.w, self.w_ph)) + list(zip(self.g, self.g_ph)):
            assert not t.numel() or (t.data_ptr() // 4) % 4 == ph
        if fill:
            for dst, src in zip(self.w, w0):
                dst.copy_(src)
        for dst in self.g:
            dst.zero_()
        self.mask_w = torch.ones(w_len, dtype=torch.bool)
        self.mask_g = torch.ones(g_len, dtype=torch.bool)
        for o, n in zip(w_off, sizes):
            self.mask_w[o:o + n] = False
        for o, n in zip(g_off, sizes):
            self.mask_g[o:o + n] = False

    def set_grads(self, grads):
        for dst, src in zip(self.g, grads):
            dst.copy_(src)

    def weights(self):
        return [t.cpu() for t in self.w]

    def assert_guards(self):
        W, G = self.W.cpu(), self.G.cpu()
        s = torch.tensor(SENTINEL)
        assert torch.equal(W[self.mask_w], s.expand(int(self.mask_w.sum()))), "a word outside the weight blocks was written"
        assert torch.equal(G[self.mask_g], s.expand(int(self.mask_g.sum()))), "a word outside the gradient blocks was written"


KINDS = {
    "sgd": ("sgd", dict(learning_rate=f32(0.05))),
    "momentum": ("momentum", dict(learning_rate=f32(0.05), momentum=f32(0.9))),
    "nesterov": ("momentum", dict(learning_rate=f32(0.05), momentum=f32(0.9), nesterov=1)),
    "adam": ("adam", dict(learning_rate=f32(1e-3), beta1=f32(0.9), beta2=f32(0.999), epsilon=f32(1e-8))),
    "adam_l2": ("adam", dict(learning_rate=f32(1e-3), beta1=f32(0.9), beta2=f32(0.999), epsilon=f32(1e-8), weight_decay=f32(0.01))),
    "adamw": ("adam", dict(learning_rate=f32(1e-3), beta1=f32(0.9), beta2=f32(0.999), epsilon=f32(1e-8), weight_decay=f32(0.01), decoupled=1)),
}
GS = f32(0.125)
# the gradient norm of step t is about 1.06e-3 (1 + t % 3) sqrt(total): clip at 1.5 x the smallest, so steps with t % 3 == 0 pass unclipped
CLIP = f32(1.5 * 1e-3 * np.sqrt(sum(SIZES)) * GS)
BIG_CLIP = f32(1.5 * 1e-3 * np.sqrt(sum(BIG_SIZES)) * GS)


def _torch_optimizer(params, cfg):
    lr = cfg["learning_rate"]
    if "beta1" in cfg:
        cls = torch.optim.AdamW if cfg.get("decoupled") else torch.optim.Adam
        return cls(params, lr=lr, betas=(cfg["beta1"], cfg["beta2"]), eps=cfg["epsilon"], weight_decay=cfg.get("weight_decay", 0.0), foreach=False)
    return torch.optim.SGD(params, lr=lr, momentum=cfg.get("momentum", 0.0), nesterov=bool(cfg.get("nesterov")), foreach=False)


@functools.lru_cache(None)
def _reference(name, clipped, dtype):
    return _trajectory(name, clipped, dtype, _inputs(), STEPS, CLIP)


def _trajectory(name, clipped, dtype, inputs, steps, clip):
    """the trajectory on the CPU: (final weights, [norm, clip factor] per step)"""
    w0, grads = inputs
    _, cfg = KINDS[name]
    params = [torch.nn.Parameter(w.to(dtype).clone()) for w in w0]            # (a copy: .to() of the same dtype shares storage)
    opt = _torch_optimizer(params, cfg)
    info = []
    for t in range(steps):
        for p, g in zip(params, grads[t]):
            p.grad = g.to(dtype) * (GS if clipped else 1.0)
        if clipped:
            norm = float(torch.nn.utils.clip_grad_norm_(params, clip, foreach=False))
            info.append((norm, min(1.0, clip / (norm + 1e-6))))
        else:
            info.append((float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params))), 1.0))
        opt.step()
    return [p.detach().clone() for p in params], info


def _library(gpu, name, clipped, order=None, steps=STEPS, inputs=None, clip=CLIP, **extra):
    w0, grads = _inputs() if inputs is None else inputs
    sizes = tuple(w.numel() for w in w0)
    kind, cfg = KINDS[name]
    cfg = dict(cfg, **extra)
    if clipped:
        cfg.update(grad_scale=GS, clip_norm=clip)
    buf = Buffers(gpu, sizes, w0)
    order = list(range(len(sizes))) if order is None else order
    opt = NL.Optimizer(kind, [(buf.w[i], buf.g[i]) for i in order], **cfg)
    info = []
    for t in range(steps):
        buf.set_grads(grads[t])
        opt.step()
        info.append(opt.info())
    state = {i: opt.state(k) for k, i in enumerate(order)}
    torch.cuda.synchronize()
    opt.destroy()
    return buf, info, state


def _assert_trajectory(gpu, name, clipped, inputs=None, steps=STEPS, clip=CLIP):
    if inputs is None:
        (r64, info64), (r32, _) = _reference(name, clipped, torch.float64), _reference(name, clipped, torch.float32)
    else:
        (r64, info64), (r32, _) = (_trajectory(name, clipped, dt, inputs, steps, clip) for dt in (torch.float64, torch.float32))
    buf, info, _ = _library(gpu, name, clipped, steps=steps, inputs=inputs, clip=clip)
    buf.assert_guards()
    if clipped:
        factors = [c for _, c in info64]
        assert any(c < 1.0 for c in factors) and any(c == 1.0 for c in factors), "the case must clip some steps and pass others"
    for t, (got, (norm, clip)) in enumerate(zip(info, info64)):
        assert abs(got[0] - norm) <= 1e-6 * norm, ("norm", t, got[0], norm)
        assert abs(got[1] - clip) <= 2e-6, ("clip factor", t, got[1], clip)
        assert got[2] == 0.0 and got[3] == t + 1
    e32 = max(float((a.double() - b).abs().max()) for a, b in zip(r32, r64) if a.numel())
    worst = 0.0
    for i, (got, a64) in enumerate(zip(buf.weights(), r64)):
        if not got.numel():
            continue
        err = (got.double() - a64).abs()
        ulp = torch.from_numpy(np.spacing(a64.abs().float().numpy())).double()
        worst = max(worst, float(err.max()))
        assert bool((err <= FACTOR * e32 + ulp).all()), (name, i, float(err.max()), e32)
    print("%s %s: library err %.3e, torch float32 err %.3e, ratio %.2f" % (name, "clipped" if clipped else "plain", worst, e32, worst / e32 if e32 else 0.0))


@pytest.mark.parametrize("clipped", [False, True], ids=["plain", "scaled_clipped"])
@pytest.mark.parametrize("name", list(KINDS))
def test_trajectory_matches_torch_float64(gpu, name, clipped):
    _assert_trajectory(gpu, name, clipped)


# ---- more chunks than workgroups: the grid-stride loops of both passes ----

def _assert_grid_stride_premise():
    assert _chunk_floats(sum(BIG_SIZES)) == OPT_CHUNK
    assert _n_chunks(BIG_SIZES, _w_phases(len(BIG_SIZES))) == 2201 > OPT_MAX_GRID          # 153 workgroups of each pass take a second chunk


def test_grid_stride_trajectory_matches_torch_float64(gpu):
    """three Adam steps with grad_scale and a clip_norm that passes step 0 and clips steps 1 and 2, on 2201 chunks"""
    _assert_grid_stride_premise()
    _assert_trajectory(gpu, "adam", True, _make_inputs(BIG_SIZES, BIG_STEPS), BIG_STEPS, BIG_CLIP)


def test_grid_stride_zero_gradients(gpu):
    _assert_grid_stride_premise()
    buf, info, _ = _library(gpu, "adam", True, steps=1, inputs=_make_inputs(BIG_SIZES, 1), clip=BIG_CLIP, zero_gradients=1)
    assert info[0][2] == 0.0 and info[0][3] == 1.0
    for g in buf.g:
        gc = g.cpu()
        assert torch.equal(gc, torch.zeros_like(gc)) and not bool(torch.signbit(gc).any()), "every gradient element must be +0.0"
    buf.assert_guards()


def test_grid_stride_independent_of_the_block_order(gpu):
    _assert_grid_stride_premise()
    inputs = _make_inputs(BIG_SIZES, BIG_STEPS)
    a, ia, sa = _library(gpu, "adam", True, steps=BIG_STEPS, inputs=inputs, clip=BIG_CLIP)
    r, ir, sr = _library(gpu, "adam", True, steps=BIG_STEPS, inputs=inputs, clip=BIG_CLIP, order=list(reversed(range(len(BIG_SIZES)))))
    assert all(np.array_equal(x, y) for x, y in zip(ia, ir))
    assert all(torch.equal(x, y) for x, y in zip(a.weights(), r.weights()))
    for k in range(len(BIG_SIZES)):
        if BIG_SIZES[k]:
            assert np.array_equal(sa[k][0], sr[k][0]) and np.array_equal(sa[k][1], sr[k][1])
    r.assert_guards()


# ---- a total beyond 4096 x 16384 floats: chunks of 8192 floats.  Everything stays on the device ----

HUGE_SIZES = (OPT_CHUNK * OPT_MAX_CHUNKS + 4_099, 5)


def _ulp(a):
    """one float32 ulp of |a| (a float64 tensor), as float64"""
    a32 = a.abs().float()
    return (torch.nextafter(a32, torch.full_like(a32, float("inf"))) - a32).double()


def test_chunk_larger_than_4096(gpu):
    """SGD over 67 M + 4104 floats.  Step one (no scale, no clip) equals nntk_sgd_optimize_device bit for bit; step two (grad_scale and a
    clip_norm below the norm): norm and clip factor against a float64 sum on the device, every weight within 1 float32 ulp of
    w - lr * clip * gs * g in float64 -- the update is three float32 roundings of products under one subtraction, and the weights are
    O(1) (0.5 <= |w| < 1.5) against an update of O(1e-4), so one ulp of the weight covers it"""
    L = capi.load()
    total = sum(HUGE_SIZES)
    assert total == 67_112_968 > OPT_CHUNK * OPT_MAX_CHUNKS and _chunk_floats(total) == 2 * OPT_CHUNK
    w_ph, g_ph = [3, 2], [3, 0]
    assert _n_chunks(HUGE_SIZES, w_ph) == 8194 > OPT_MAX_GRID
    lr = f32(0.05)
    gen = torch.Generator(device=gpu).manual_seed(67)
    buf, ref = (Buffers(gpu, HUGE_SIZES, None, w_ph, g_ph, fill=False) for _ in range(2))
    for w, wr in zip(buf.w, ref.w):
        w.copy_((torch.rand(w.numel(), generator=gen, device=gpu) + 0.5) * (torch.randint(0, 2, (w.numel(),), generator=gen, device=gpu) * 2 - 1))
        wr.copy_(w)

    def set_grads(scale):
        for g, gr in zip(buf.g, ref.g):
            g.copy_(torch.randn(g.numel(), generator=gen, device=gpu) * scale)
            gr.copy_(g)

    def guards(b):
        for full, mask in ((b.W, b.mask_w), (b.G, b.mask_g)):
            assert bool((full[mask.to(gpu)] == SENTINEL).all()), "a word outside the blocks was written"

    # step one
    set_grads(1e-3)
    opt = NL.Optimizer("sgd", list(zip(buf.w, buf.g)), learning_rate=lr)
    opt.step()
    info = [float(v) for v in opt.info()]                 # (python floats: the comparisons below are made in float64)
    opt.destroy()
    for w, g in zip(ref.w, ref.g):
        assert L.nntk_sgd_optimize_device(capi.SGD(lr), C.c_void_p(g.data_ptr()), C.c_void_p(w.data_ptr()), w.numel()) == 0, capi.last_error()
    torch.cuda.synchronize()
    norm64 = float(torch.sqrt(sum(g.double().square().sum() for g in buf.g)))
    print("step 1: norm %.9g, float64 %.9g, relative error %.2e" % (info[0], norm64, abs(info[0] - norm64) / norm64))
    assert abs(info[0] - norm64) <= 1e-6 * norm64 and info[1] == 1.0 and info[2] == 0.0 and info[3] == 1.0, info
    assert all(torch.equal(x, y) for x, y in zip(buf.w, ref.w)), "kind 0 without scale and clip differs from nntk_sgd_optimize_device"
    # step two
    set_grads(2e-3)
    norm64 = float(torch.sqrt(sum((g.double() * GS).square().sum() for g in buf.g)))
    clip_norm = f32(0.5 * norm64)
    clip64 = min(1.0, clip_norm / (norm64 + 1e-6))
    want = [w.double() - lr * clip64 * GS * g.double() for w, g in zip(buf.w, buf.g)]
    opt = NL.Optimizer("sgd", list(zip(buf.w, buf.g)), learning_rate=lr, grad_scale=GS, clip_norm=clip_norm)
    opt.step()
    info = [float(v) for v in opt.info()]                 # (python floats: the comparisons below are made in float64)
    opt.destroy()
    print("step 2: norm %.9g, float64 %.9g, relative error %.2e; clip factor %.9g, float64 %.9g"
          % (info[0], norm64, abs(info[0] - norm64) / norm64, info[1], clip64))
    assert abs(info[0] - norm64) <= 1e-6 * norm64, ("norm", info[0], norm64)
    assert clip64 < 1.0 and abs(info[1] - clip64) <= 2e-6, ("clip factor", info[1], clip64)
    assert info[2] == 0.0 and info[3] == 1.0
    for got, w64, before in zip(buf.w, want, ref.w):
        err = (got.double() - w64).abs() / _ulp(w64)
        print("step 2: %d weights, largest error %.3f ulp" % (got.numel(), float(err.max())))
        assert bool((err <= 1.0).all()) and not torch.equal(got, before)
    for g, gr in zip(buf.g, ref.g):
        assert torch.equal(g, gr), "without zero_gradients the gradients are untouched"
    guards(buf); guards(ref)
    del want, buf, ref
    torch.cuda.empty_cache()


def test_clip_boundary(gpu):
    """a norm just below the limit leaves the gradients alone, bit for bit; a norm above it is scaled"""
    _, grads = _inputs()
    norm = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads[0])))
    res = {}
    for tag, clip in (("none", 0.0), ("below", f32(norm * 1.001)), ("above", f32(norm * 0.5))):
        buf = Buffers(gpu)
        opt = NL.Optimizer("adam", list(zip(buf.w, buf.g)), learning_rate=f32(1e-3), clip_norm=clip)
        buf.set_grads(grads[0])
        opt.step()
        res[tag] = (buf.weights(), opt.info())
        opt.destroy()
    assert res["below"][1][1] == 1.0 and res["none"][1][1] == 1.0
    assert all(torch.equal(a, b) for a, b in zip(res["below"][0], res["none"][0]))
    assert 0.0 < res["above"][1][1] < 1.0 and abs(res["above"][1][1] - 0.5) < 1e-3
    assert not all(torch.equal(a, b) for a, b in zip(res["above"][0], res["none"][0]))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_gradient_skips_the_step(gpu, bad):
    _, grads = _inputs()
    i65537 = SIZES.index(65537)

    def run(with_bad):
        buf = Buffers(gpu)
        opt = NL.Optimizer("adam", list(zip(buf.w, buf.g)), learning_rate=f32(1e-3), clip_norm=CLIP, zero_gradients=1)
        for t in (0, 1):
            buf.set_grads(grads[t])
            opt.step()
        snap = None
        if with_bad:
            before = (buf.weights(), [opt.state(k) for k in range(len(SIZES))], opt.info())
            buf.set_grads(grads[2])
            buf.g[i65537][65537 // 2] = bad
            opt.step()
            info = opt.info()
            assert info[2] == 1.0 and info[3] == 2.0 and info[3] == before[2][3], info
            assert all(torch.equal(a, b) for a, b in zip(buf.weights(), before[0])), "a skipped step changed the weights"
            for k, (m, v) in enumerate(opt.state(k) for k in range(len(SIZES))):
                if SIZES[k]:
                    assert np.array_equal(m, before[1][k][0]) and np.array_equal(v, before[1][k][1]), "a skipped step changed the moments"
            for g in buf.g:
                gc = g.cpu()
                assert torch.equal(gc, torch.zeros_like(gc)) and not bool(torch.signbit(gc).any()), "zero_gradients after a skipped step"
            snap = info
        buf.set_grads(grads[3])
        opt.step()
        out = (buf.weights(), [opt.state(k) for k in range(len(SIZES))], opt.info())
        buf.assert_guards()
        opt.destroy()
        return out

    a, b = run(True), run(False)
    assert a[2][2] == 0.0 and a[2][3] == 3.0 and np.array_equal(a[2], b[2])
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])), "the step after a skipped one is not step t + 1 of a clean run"
    for k in range(len(SIZES)):
        if SIZES[k]:
            assert np.array_equal(a[1][k][0], b[1][k][0]) and np.array_equal(a[1][k][1], b[1][k][1])


def test_zero_gradients(gpu):
    _, grads = _inputs()
    for zero in (1, 0):
        buf = Buffers(gpu)
        opt = NL.Optimizer("momentum", list(zip(buf.w, buf.g)), learning_rate=f32(0.05), momentum=f32(0.9), zero_gradients=zero)
        buf.set_grads(grads[0])
        opt.step()
        assert opt.info()[2] == 0.0
        for g, g0 in zip(buf.g, grads[0]):
            gc = g.cpu()
            if zero:
                assert torch.equal(gc, torch.zeros_like(gc)) and not bool(torch.signbit(gc).any()), "every gradient element must be +0.0"
            else:
                assert torch.equal(gc, g0), "without zero_gradients the gradients are untouched"
        buf.assert_guards()
        opt.destroy()


def test_deterministic_and_independent_of_the_block_order(gpu):
    a, ia, sa = _library(gpu, "adam", True, steps=3)
    b, ib, sb = _library(gpu, "adam", True, steps=3)
    r, ir, sr = _library(gpu, "adam", True, steps=3, order=list(reversed(range(len(SIZES)))))
    for other, io, so, what in ((b, ib, sb, "the same steps twice"), (r, ir, sr, "the blocks listed in reverse")):
        assert all(np.array_equal(x, y) for x, y in zip(ia, io)), what
        assert all(torch.equal(x, y) for x, y in zip(a.weights(), other.weights())), what
        for k in range(len(SIZES)):
            if SIZES[k]:
                assert np.array_equal(sa[k][0], so[k][0]) and np.array_equal(sa[k][1], so[k][1]), what
    r.assert_guards()


def test_kind_0_equals_sgd_optimize_device_bit_for_bit(gpu):
    _, grads = _inputs()
    L = capi.load()
    lr = f32(0.05)
    buf, ref = Buffers(gpu), Buffers(gpu)
    opt = NL.Optimizer("sgd", list(zip(buf.w, buf.g)), learning_rate=lr)
    for t in range(2):
        buf.set_grads(grads[t]); ref.set_grads(grads[t])
        opt.step()
        for w, g in zip(ref.w, ref.g):
            if w.numel():
                assert L.nntk_sgd_optimize_device(capi.SGD(lr), C.c_void_p(g.data_ptr()), C.c_void_p(w.data_ptr()), w.numel()) == 0
    assert opt.state(3) == (None, None)
    assert all(torch.equal(x, y) for x, y in zip(buf.weights(), ref.weights()))
    opt.destroy()


def test_set_learning_rate_and_empty_optimizer(gpu):
    _, grads = _inputs()
    buf, ref = Buffers(gpu), Buffers(gpu)
    a = NL.Optimizer("sgd", list(zip(buf.w, buf.g)), learning_rate=f32(0.05))
    b = NL.Optimizer("sgd", list(zip(ref.w, ref.g)), learning_rate=f32(0.01))
    a.set_learning_rate(f32(0.01))
    buf.set_grads(grads[0]); ref.set_grads(grads[0])
    a.step(); b.step()
    assert all(torch.equal(x, y) for x, y in zip(buf.weights(), ref.weights()))
    a.destroy(); b.destroy()
    e = NL.Optimizer("adam", [], learning_rate=f32(1e-3))
    e.step()
    info = e.info()
    assert info[0] == 0.0 and info[2] == 0.0 and info[3] == 1.0
    e.destroy()


# ---- <Layer>LoadWeightsDevice -------------------------------------------------------------------------------------------------------

def _host_block(ptr, n):
    return np.ctypeslib.as_array(ptr, shape=(n,))


def _families(gpu):
    L = capi.load()
    B = 3
    dp = lambda t: C.c_void_p(t.data_ptr())

    def dense_fwd(layer, x):
        out = x.new_empty((x.shape[0], 4))
        assert L.DenseApplyDevice(layer.h, dp(x), dp(out), x.shape[0]) == 0, capi.last_error()
        return out

    fam = {
        "Conv1d": (lambda: NL.Conv1d(5, 7, 3, 1, 11), 7 * 5 * 3 + 7, (B, 11, 5), lambda l, x: l.apply_device(x), L.Conv1dGetWeights, "W"),
        "BatchNorm": (lambda: NL.BatchNorm(7, 1e-3, 9), 4 * 7, (B, 9, 7), lambda l, x: l.apply_device(x), L.BatchNormGetWeights, "gamma"),
        "GRU": (lambda: NL.GRU(6, 10, True, 5), 6 * 30 + 10 * 30 + 60, (B, 5, 6), lambda l, x: l.apply_device(x), L.GRUGetWeights, "W"),
        "LSTM": (lambda: NL.LSTM(6, 10, True, 5), 6 * 40 + 10 * 40 + 80, (B, 5, 6), lambda l, x: l.apply_device(x), L.LSTMGetWeights, "W"),
        "RNN": (lambda: NL.RNN(6, 10, True, 5), 6 * 10 + 10 * 10 + 20, (B, 5, 6), lambda l, x: l.apply_device(x), L.RNNGetWeights, "W"),
        "Dense": (lambda: NL.Dense(9, 4), 9 * 4 + 4, (B, 9), dense_fwd, L.DenseGetWeights, "W"),
        "TimeDistributedDense": (lambda: NL.TimeDistributedDense(3, 9, 4), 9 * 4 + 4, (B, 3, 9), lambda l, x: l.apply_device(x),
                                 L.TimeDistributedDenseGetWeights, "W"),
    }
    return fam


@pytest.mark.parametrize("family", ["Conv1d", "BatchNorm", "GRU", "LSTM", "RNN", "Dense", "TimeDistributedDense"])
def test_load_weights_device(gpu, family):
    make, n, xshape, fwd, get, first = _families(gpu)[family]
    rng = np.random.default_rng(5)
    old, new = rng.uniform(-0.5, 0.5, n).astype(np.float32), rng.uniform(-0.5, 0.5, n).astype(np.float32)
    if family == "BatchNorm":
        old[21:], new[21:] = np.abs(old[21:]) + 0.5, np.abs(new[21:]) + 0.5          # the variances
    x = torch.from_numpy(rng.uniform(-1, 1, xshape).astype(np.float32)).to(gpu)
    a, fresh = make(), make()
    host = _host_block(getattr(get(a.h).contents, first), n)
    host[:] = old
    sync = getattr(capi.load(), family + "SyncWeights")
    assert sync(a.h) == 0, capi.last_error()
    y_old = fwd(a, x).clone()
    d_new = torch.from_numpy(new).to(gpu)
    assert torch.equal(fwd(a, x), y_old), "before the call the forward uses the old weights"
    a.load_weights_device(d_new)
    assert np.array_equal(host, new), "GetWeights() shows the device block"
    y_new = fwd(a, x).clone()
    _host_block(getattr(get(fresh.h).contents, first), n)[:] = new
    assert sync(fresh.h) == 0, capi.last_error()
    y_fresh = fwd(fresh, x)
    torch.cuda.synchronize()
    assert torch.equal(y_new, y_fresh) and not torch.equal(y_new, y_old)
    a.destroy(); fresh.destroy()


# ---- the closed loop: LSTM -> softmax TimeDistributedDense -> CTC, Adam with clipping, the weights never leave the device --------------

B_, T_, IN_, H_, V_ = 4, 12, 8, 16, 5
LABELS = [[1, 2, 3], [2, 4], [3, 1, 1], [4, 2, 3, 1]]
N_LSTM, N_TDD = IN_ * 4 * H_ + H_ * 4 * H_ + 8 * H_, H_ * V_ + V_
ADAM = dict(learning_rate=f32(0.02), beta1=f32(0.9), beta2=f32(0.999), epsilon=f32(1e-8), clip_norm=f32(1.0), grad_scale=f32(1.0 / B_))


class _Model:
    def __init__(self, L):
        self.L = L
        self.acts = L.LSTMActivationsCreateDefault(H_)
        self.lstm = L.LSTMCreateForTraining(L.LSTMConfigCreate(IN_, H_, True, T_, True, self.acts), capi.ConvTrainingConfig(B_))
        self.soft = L.ActivationFunctionCreateSoftmax(1, V_)
        self.tdd = L.TimeDistributedDenseCreateForTraining(L.TimeDistributedDenseConfigCreate(T_, L.DenseConfigCreate(H_, V_, self.soft)),
                                                           capi.ConvTrainingConfig(B_))
        assert self.lstm and self.tdd, capi.last_error()

    def load(self, wl, wt):
        assert self.L.LSTMLoadWeightsDevice(self.lstm, C.c_void_p(wl.data_ptr())) == 0, capi.last_error()
        assert self.L.TimeDistributedDenseLoadWeightsDevice(self.tdd, C.c_void_p(wt.data_ptr())) == 0, capi.last_error()

    def forward(self, x):
        dp = lambda t: C.c_void_p(t.data_ptr())
        self.x, self.hseq, self.probs = x, x.new_empty((B_, T_, H_)), x.new_empty((B_, T_, V_))
        assert self.L.LSTMApplyTrainingBatchDevice(self.lstm, dp(x), dp(self.hseq)) == 0, capi.last_error()
        assert self.L.TimeDistributedDenseApplyTrainingBatchDevice(self.tdd, dp(self.hseq), dp(self.probs)) == 0, capi.last_error()
        return self.probs

    def backward(self, dprobs, gl, gt):
        dp = lambda t: C.c_void_p(t.data_ptr())
        dh, dx = torch.empty_like(self.hseq), torch.empty_like(self.x)
        assert self.L.TimeDistributedDenseCalculateGradientDevice(self.tdd, dp(gt), dp(dh), dp(dprobs)) == 0, capi.last_error()
        assert self.L.LSTMCalculateGradientDevice(self.lstm, dp(gl), dp(dx), dp(dh)) == 0, capi.last_error()

    def destroy(self):
        self.L.LSTMDestroy(self.lstm); self.L.TimeDistributedDenseDestroy(self.tdd)
        self.L.LSTMActivationsDestroy(self.acts); self.L.ActivationFunctionDestroy(self.soft)


def _closed_loop(gpu, driver, steps=30):
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.uniform(-1, 1, (B_, T_, IN_)).astype(np.float32)).to(gpu)
    wl = torch.from_numpy(rng.uniform(-0.3, 0.3, N_LSTM).astype(np.float32)).to(gpu)
    wt = torch.from_numpy(rng.uniform(-0.3, 0.3, N_TDD).astype(np.float32)).to(gpu)
    gl, gt = torch.zeros_like(wl), torch.zeros_like(wt)
    model = _Model(capi.load())
    model.load(wl, wt)
    if driver == "library":
        opt = NL.Optimizer("adam", [(wl, gl), (wt, gt)], zero_gradients=1, **ADAM)
    else:
        params = [torch.nn.Parameter(wl.cpu().double()), torch.nn.Parameter(wt.cpu().double())]
        opt = torch.optim.Adam(params, lr=ADAM["learning_rate"], betas=(ADAM["beta1"], ADAM["beta2"]), eps=ADAM["epsilon"])
    losses = []
    for _ in range(steps):
        loss, dprobs = NL.ctc_loss_device(model.forward(x), LABELS)
        losses.append(loss.sum())
        model.backward(dprobs, gl, gt)
        if driver == "library":
            opt.step()
        else:
            for p, g in zip(params, (gl, gt)):
                p.grad = g.cpu().double() * ADAM["grad_scale"]
                g.zero_()
            torch.nn.utils.clip_grad_norm_(params, ADAM["clip_norm"])
            opt.step()
            wl.copy_(params[0].detach().float()); wt.copy_(params[1].detach().float())
        model.load(wl, wt)
    final = model.forward(x).clone()
    if driver == "library":
        info = opt.info()
        assert info[3] == steps and info[2] == 0.0, info
        opt.destroy()
    fresh = _Model(capi.load())
    hw = _host_block(capi.load().LSTMGetWeights(fresh.lstm).contents.W, N_LSTM)
    ht = _host_block(capi.load().TimeDistributedDenseGetWeights(fresh.tdd).contents.W, N_TDD)
    hw[:], ht[:] = wl.cpu().numpy(), wt.cpu().numpy()
    assert capi.load().LSTMSyncWeights(fresh.lstm) == 0 and capi.load().TimeDistributedDenseSyncWeights(fresh.tdd) == 0, capi.last_error()
    same = torch.equal(final, fresh.forward(x))
    losses = [float(v) for v in torch.stack(losses).cpu()]
    model.destroy(); fresh.destroy()
    return losses, same


def test_closed_training_loop(gpu):
    """30 steps of step -> LoadWeightsDevice: the loss falls, as it does (with margin) when torch's float64 Adam drives the same gradient calls"""
    ref, _ = _closed_loop(gpu, "torch64")
    got, same = _closed_loop(gpu, "library")
    print("summed CTC loss: first %.4f, last %.4f (library); first %.4f, last %.4f (torch float64 optimizer)" % (got[0], got[-1], ref[0], ref[-1]))
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    assert ref[-1] < 0.9 * ref[0], "the case must train with margin under the reference optimizer"
    assert got[-1] < got[0]
    assert abs(got[-1] - ref[-1]) < 0.05 * ref[0], "the two optimizers follow the same trajectory"
    assert same, "the handle's forward after the last LoadWeightsDevice differs from a fresh handle with the final weights"
