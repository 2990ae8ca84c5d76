"""nntk_attention_device against the float64 definition (tests/attention_reference.py), and the guarantee of its header: poisoned
invisible rows, a stream pushed through a sliding K/V window, two calls, all with equal bits.

Tolerance.  The error of a call is max |x - ref64| / max |ref64|, for out and for lse.  torch's f32 CPU evaluation of the same formula
(matmul, masked_fill, softmax / logsumexp, matmul) on the cases of test_against_float64 reaches 8.8e-7 (out) and 4.7e-7 (lse) at the
most; TOL lies under 8 times the smaller of the two (3.7e-6), which covers another summation order and the device's exp.  The
kernel's own largest errors over these cases: 7.2e-7 (out) and 1.5e-6 (lse; d_head 128 with a single key, where lse is one dot product
of 128 terms summed in index order and the reference value is small).

Block sizes behind the shapes: 128 queries per workgroup; key blocks of 64 for d_head <= 64, of 32 above."""
import itertools

import numpy as np
import pytest
import torch

import attention_reference as R
from nntoolkitcore_amd import layers as NL

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gpu")]

TOL = 3.5e-6
MASKS = {"full": {}, "causal": dict(right=0), "window": dict(left=20, right=3), "chunked": dict(chunk=16, left=2, right=0, pos0=5)}


def fused(rng, B, T, HD, pad=3, ints=False):
    """one [B, T, 3 HD + pad] buffer and its q / k / v views"""
    buf = rng.integers(-8, 9, (B, T, 3 * HD + pad)).astype(np.float32) if ints else rng.standard_normal((B, T, 3 * HD + pad), np.float32)
    return buf, [buf[:, :, i * HD:(i + 1) * HD] for i in range(3)]


def on_device(buf, HD):
    t = torch.from_numpy(buf).cuda()
    return [t[:, :, i * HD:(i + 1) * HD] for i in range(3)]


def run(qkv, heads, **kw):
    """the call on outputs prefilled with NaN -> numpy (out, lse)"""
    q = qkv[0]
    out = torch.full((q.shape[0], q.shape[1], q.shape[2]), float("nan"), device="cuda")
    lse = torch.full((q.shape[0], heads, q.shape[1]), float("nan"), device="cuda")
    NL.attention_device(*qkv, heads, out=out, lse=lse, **kw)
    return out.cpu().numpy(), lse.cpu().numpy()


def errors(got, want):
    (o, l), (ro, rl) = got, want
    assert not np.isnan(o).any() and not np.isnan(l).any(), "an element was not written"
    inv = np.isneginf(rl)
    assert np.array_equal(np.isneginf(l), inv) and not o[np.repeat(inv.transpose(0, 2, 1), o.shape[2] // inv.shape[1], axis=2)].any()
    fin = ~inv
    e_l = np.abs(l[fin] - rl[fin]).max() / np.abs(rl[fin]).max() if fin.any() else 0.0
    return np.abs(o - ro).max() / max(np.abs(ro).max(), 1e-30), e_l


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("T", [1, 17, "BK+1", 129, 150])
@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("d", [1, 5, 64, 128])
def test_against_float64(d, heads, T, mask):
    T = (33 if d > 64 else 65) if T == "BK+1" else T
    rng = np.random.default_rng(1000 * d + 10 * T + heads)
    buf, qkv = fused(rng, 3, T, heads * d)
    lengths = [T, 2 * T // 3, 0] if heads == 1 else [T, 1, T // 2]
    want = R.attention(*qkv, heads, lengths, **MASKS[mask])
    e_o, e_l = errors(run(on_device(buf, heads * d), heads, kv_lengths=lengths, **MASKS[mask]), want)
    print("attention d %d heads %d T %d %s: out %.3g lse %.3g" % (d, heads, T, mask, e_o, e_l))
    assert e_o < TOL and e_l < TOL


def test_large_scores():
    """Scaled scores up to +-1.3e4.  q and k hold small integers and the scale is a power of two, so every score is exact in f32: the
    case is about the range of the softmax, not about the rounding of a score of 1e4 (1e-3 in f32 for any implementation)."""
    rng = np.random.default_rng(5)
    buf, qkv = fused(rng, 2, 150, 2 * 64, ints=True)
    assert np.abs(16.0 * np.einsum("bid,bjd->bij", qkv[0][:, :, :64], qkv[1][:, :, :64])).max() > 1e4
    got = run(on_device(buf, 128), 2, scale=16.0, right=0)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    e_o, e_l = errors(got, R.attention(*qkv, 2, scale=16.0, right=0))
    print("attention large scores: out %.3g lse %.3g" % (e_o, e_l))
    assert e_o < TOL and e_l < TOL


@pytest.mark.parametrize("mask", ["window", "chunked"])
def test_poisoned_invisible_rows_leave_the_bits(mask):
    """NaN in every K / V row that no query sees or that lies beyond kv_lengths, in the Q rows of invalid queries and in the padding
    between the strides"""
    B, Tq, Tk, heads, d, off = 3, 40, 150, 2, 20, 100
    HD, lengths, kw = heads * d, [150, 120, 101], dict(MASKS[mask], q_offset=off)
    rng = np.random.default_rng(11)
    clean, _ = fused(rng, B, Tk, HD, pad=5)
    dirty = clean.copy()
    dirty[:, :, 3 * HD:] = np.nan
    for b in range(B):
        vis = R.visible(Tq, Tk, lengths[b], **kw)
        dirty[b, ~vis.any(axis=0), HD:3 * HD] = np.nan
        dirty[b, off:off + Tq][~vis.any(axis=1), :HD] = np.nan
        dirty[b, :off, :HD] = np.nan                                          # frames of the buffer that are no query of this call
    assert np.isnan(dirty[:, :, HD:3 * HD]).any(axis=2).sum() > B * 50 and np.isnan(dirty[1, off:off + Tq, :HD]).any()
    outs = []
    for x in (clean, dirty):
        q, k, v = on_device(x, HD)
        outs.append(run([q[:, off:off + Tq], k, v], heads, kv_lengths=lengths, **kw))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert errors(outs[1], R.attention(clean[:, off:off + Tq, :HD], clean[:, :, HD:2 * HD], clean[:, :, 2 * HD:3 * HD], heads, lengths, **kw))[0] < TOL


def pushed(q, k, v, heads, sizes, back, ahead, **mask):
    """the stream in pushes of `sizes` frames (cycled) through a K/V window that keeps `back` frames behind the push and `ahead` in
    front of it: the concatenated outputs"""
    T, s, outs, lses = q.shape[1], 0, [], []
    for n in itertools.cycle(sizes):
        n, w0 = min(n, T - s), max(0, s - back)
        w1 = min(T, s + n + ahead)
        o, l = NL.attention_device(q[:, s:s + n], k[:, w0:w1], v[:, w0:w1], heads, q_offset=s - w0, pos0=w0, **mask)
        outs.append(o); lses.append(l)
        s += n
        if s == T:
            return torch.cat(outs, 1).cpu().numpy(), torch.cat(lses, 2).cpu().numpy()


@pytest.fixture(scope="module")
def stream(gpu):
    """one sequence of 150 frames, d_head 20, 2 heads, as rows 0 and 2 of two 3-row batches whose other rows differ"""
    rng = np.random.default_rng(21)
    seq = rng.standard_normal((1, 150, 120), np.float32)
    batches = []
    for pos in (0, 2):
        x = rng.standard_normal((3, 150, 120), np.float32)
        x[pos] = seq[0]
        batches.append((pos, on_device(x, 40)))
    return on_device(seq, 40), batches


@pytest.mark.parametrize("sizes,back,ahead,mask", [((16,), 32, 0, dict(chunk=16, left=2, right=0)), ((1, 7, 40), 20, 3, dict(left=20, right=3))])
def test_pushes_give_the_one_shot_bits(stream, sizes, back, ahead, mask):
    one, batches = stream
    want = run(one, 2, **mask)
    got = pushed(*one, 2, sizes, back, ahead, **mask)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    again = run(one, 2, **mask)
    assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])                 # two calls, equal bits
    if ahead == 0:
        for pos, qkv in batches:
            got = pushed(*qkv, 2, sizes, back, ahead, **mask)
            assert np.array_equal(got[0][pos], want[0][0]) and np.array_equal(got[1][pos], want[1][0])
