"""nntk_attention_backward_device against torch autograd in float64 on the dense formula (masked with attention_reference.visible),
fed with the out and lse that layers.attention_device wrote, so the pair is tested as it will be used.

Tolerance.  The error of a tensor is max |x - ref64| / max |ref64| over a call.  The same formula under torch autograd in f32 on the
CPU reaches, over the cases of test_against_float64, 1.26e-6 (dq), 1.03e-6 (dk) and 9.6e-7 (dv) at the most; TOL lies under 8
times the smallest of the three (7.7e-6), which covers another summation order and the device's exp.  The kernels' own largest errors over
these cases: 1.83e-6 (dq), 1.10e-6 (dk), 1.08e-6 (dv).

Block sizes behind the shapes: 128 queries (dq) or 128 keys (dk / dv) per workgroup, walked in sub-blocks of 32."""
import numpy as np
import pytest
import torch

import attention_reference as R
from nntoolkitcore_amd import layers as NL

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu")]

TOL = 7.5e-6
MASKS = {"full": {}, "causal": dict(right=0), "window": dict(left=20, right=3), "chunked": dict(chunk=16, left=2, right=0, pos0=5)}


def reference(q, k, v, dout, heads, lengths=None, scale=None, dtype=torch.float64, **kw):
    """(dq, dk, dv) of sum(out * dout) by autograd on the dense masked formula; zeros for invalid queries and unseen keys"""
    B, Tq, HD = q.shape
    Tk, d = k.shape[1], HD // heads
    leaves = [torch.tensor(np.ascontiguousarray(x), dtype=dtype, requires_grad=True) for x in (q, k, v)]
    qh, kh, vh = (x.reshape(B, -1, heads, d).transpose(1, 2) for x in leaves)
    vis = torch.from_numpy(np.stack([R.visible(Tq, Tk, Tk if lengths is None else lengths[b], **kw) for b in range(B)]))[:, None]
    s = ((d ** -0.5 if scale is None else scale) * (qh @ kh.transpose(2, 3))).masked_fill(~vis, float("-inf"))
    p = torch.softmax(s.masked_fill(~vis.any(-1, keepdim=True), 0.0), -1) * vis               # an invalid query: a row of zeros
    (p @ vh).backward(torch.tensor(np.ascontiguousarray(dout), dtype=dtype).reshape(B, Tq, heads, d).transpose(1, 2))
    return [x.grad.numpy() for x in leaves]


def run(buf, dout, heads, HD, Tq=None, pad=3, **kw):
    """forward and backward on the q / k / v views of the fused device buffer (Tq: the queries are the Tq frames from q_offset on); the
    gradients go into one fused [B, T, 3 HD + pad] buffer prefilled with NaN (dq into a second one of Tq frames when Tq is given: its
    batch stride is Tq frames) -> numpy (dq, dk, dv), everything outside the three slices checked to be NaN still"""
    x = torch.from_numpy(buf).cuda()
    q, k, v = (x[:, :, i * HD:(i + 1) * HD] for i in range(3))
    if Tq:
        q = q[:, kw["q_offset"]:kw["q_offset"] + Tq]
    out, lse = NL.attention_device(q, k, v, heads, **kw)
    g = torch.full((x.shape[0], x.shape[1], 3 * HD + pad), float("nan"), device="cuda")
    gq = torch.full((x.shape[0], Tq, 3 * HD + pad), float("nan"), device="cuda") if Tq else g
    grads = gq[:, :, :HD], g[:, :, HD:2 * HD], g[:, :, 2 * HD:3 * HD]
    NL.attention_backward_device(q, k, v, out, lse, torch.from_numpy(dout).cuda(), heads, dq=grads[0], dk=grads[1], dv=grads[2], **kw)
    got = [t.cpu().numpy() for t in grads]
    assert not any(np.isnan(t).any() for t in got), "an element was not written"
    assert torch.isnan(g[:, :, 3 * HD:]).all() and torch.isnan(gq[:, :, 3 * HD:]).all(), "the padding was written"
    assert not Tq or (torch.isnan(g[:, :, :HD]).all() and torch.isnan(gq[:, :, HD:]).all())
    return got


def errors(got, want):
    return [np.abs(x - r).max() / max(np.abs(r).max(), 1e-30) for x, r in zip(got, want)]


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("T", [1, 17, 129, 150])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("d", [1, 5, 64, 128])
def test_against_float64(d, heads, T, mask):
    rng = np.random.default_rng(1000 * d + 10 * T + heads)
    HD = heads * d
    buf, dout = rng.standard_normal((3, T, 3 * HD + 3), np.float32), rng.standard_normal((3, T, HD), np.float32)
    lengths = [T, 2 * T // 3, 0] if heads == 1 else [T, 1, T // 2]
    want = reference(buf[:, :, :HD], buf[:, :, HD:2 * HD], buf[:, :, 2 * HD:3 * HD], dout, heads, lengths, **MASKS[mask])
    got = run(buf, dout, heads, HD, kv_lengths=lengths, **MASKS[mask])
    e = errors(got, want)
    print("attention backward d %d heads %d T %d %s: dq %.3g dk %.3g dv %.3g" % (d, heads, T, mask, *e))
    assert max(e) < TOL
    again = run(buf, dout, heads, HD, kv_lengths=lengths, **MASKS[mask])
    assert all(np.array_equal(x, y) for x, y in zip(got, again))                      # two calls, equal bits


@pytest.mark.parametrize("mask", ["window", "chunked"])
def test_query_window_with_offset_and_poisoned_unseen_rows(mask):
    """Tq != Tk: the inverse visibility range with an offset; dk and dv of keys no query sees are exact zeros; NaN in every K / V row
    that no query sees or that lies beyond kv_lengths, in the Q, out, lse and dout rows of invalid queries and in the padding between
    the strides leaves the bits"""
    B, Tq, Tk, heads, d, off = 3, 40, 150, 2, 20, 100
    HD, lengths, kw = heads * d, [150, 120, 101], dict(MASKS[mask], q_offset=off)
    rng = np.random.default_rng(11)
    clean, dout = rng.standard_normal((B, Tk, 3 * HD + 5), np.float32), rng.standard_normal((B, Tq, HD), np.float32)
    q, k, v = clean[:, off:off + Tq, :HD], clean[:, :, HD:2 * HD], clean[:, :, 2 * HD:3 * HD]
    want = reference(q, k, v, dout, heads, lengths, **kw)
    got = run(clean, dout, heads, HD, Tq=Tq, pad=5, kv_lengths=lengths, **kw)
    assert max(errors(got, want)) < TOL
    vis = [R.visible(Tq, Tk, lengths[b], **kw) for b in range(B)]
    for b in range(B):
        assert not got[1][b, ~vis[b].any(axis=0)].any() and not got[2][b, ~vis[b].any(axis=0)].any() and not got[0][b, ~vis[b].any(axis=1)].any()

    x = torch.from_numpy(clean).cuda()
    qd, kd, vd = x[:, off:off + Tq, :HD], x[:, :, HD:2 * HD], x[:, :, 2 * HD:3 * HD]
    out, lse = NL.attention_device(qd, kd, vd, heads, kv_lengths=lengths, **kw)
    dirty, dd = clean.copy(), torch.from_numpy(dout).cuda()
    dirty[:, :, 3 * HD:] = np.nan
    dirty[:, :off, :HD] = np.nan                                                  # frames of the buffer that are no query of this call
    for b in range(B):
        inv = ~vis[b].any(axis=1)
        dirty[b, ~vis[b].any(axis=0), HD:3 * HD] = np.nan
        dirty[b, off:off + Tq][inv, :HD] = np.nan
        inv = torch.from_numpy(inv).cuda()
        out[b, inv], dd[b, inv], lse[b, :, inv] = np.nan, np.nan, np.nan
    assert np.isnan(dirty[:, :, HD:3 * HD]).any(axis=2).sum() > B * 50 and torch.isnan(out[1]).any()
    x = torch.from_numpy(dirty).cuda()
    poisoned = NL.attention_backward_device(x[:, off:off + Tq, :HD], x[:, :, HD:2 * HD], x[:, :, 2 * HD:3 * HD], out, lse, dd, heads,
                                            kv_lengths=lengths, **kw)
    assert all(np.array_equal(p.cpu().numpy(), g) for p, g in zip(poisoned, got))


def test_large_scores():
    """Scaled scores up to +-1.3e4, exact in f32 (small integers, a power-of-two scale): the range of exp(scale s - lse), and the
    rounding of an f32 lse of 1e4 (an ulp of 9.8e-4), which the kernels take out again by the recomputed row sum: without that the
    queries whose two best keys tie are off by 2.1e-4."""
    rng = np.random.default_rng(5)
    buf = rng.integers(-8, 9, (2, 150, 3 * 128 + 3)).astype(np.float32)
    dout = rng.standard_normal((2, 150, 128), np.float32)
    assert np.abs(16.0 * np.einsum("bid,bjd->bij", buf[:, :, :64], buf[:, :, 128:192])).max() > 1e4
    got = run(buf, dout, 2, 128, scale=16.0, right=0)
    assert all(np.isfinite(t).all() for t in got)
    e = errors(got, reference(buf[:, :, :128], buf[:, :, 128:256], buf[:, :, 256:384], dout, 2, scale=16.0, right=0))
    print("attention backward large scores: dq %.3g dk %.3g dv %.3g" % tuple(e))
    assert max(e) < TOL
