"""The definition of the attention core in float64 numpy, straight from the visibility rule (dense scores).  A helper, not a test."""
import numpy as np


def visible(Tq, Tk, kv_len, q_offset=0, pos0=0, chunk=1, left=-1, right=-1):
    """bool [Tq, Tk]: key j valid and visible to query i; an invalid query's row is all False"""
    p = q_offset + np.arange(Tq)[:, None]
    j = np.arange(Tk)[None, :]
    gp, gj = (pos0 + p) // chunk, (pos0 + j) // chunk
    vis = (j < kv_len) & (p < kv_len)
    if left >= 0:
        vis &= gj >= gp - left
    if right >= 0:
        vis &= gj <= gp + right
    return vis


def attention(q, k, v, heads, kv_lengths=None, q_offset=0, pos0=0, chunk=1, left=-1, right=-1, scale=None):
    """q [B, Tq, heads * d], k / v [B, Tk, heads * d] -> (out [B, Tq, heads * d], lse [B, heads, Tq]) in float64"""
    B, Tq, HD = q.shape
    Tk, d = k.shape[1], HD // heads
    scale = d ** -0.5 if scale is None else scale
    out, lse = np.zeros((B, Tq, HD)), np.full((B, heads, Tq), -np.inf)
    for b in range(B):
        vis = visible(Tq, Tk, Tk if kv_lengths is None else int(kv_lengths[b]), q_offset, pos0, chunk, left, right)
        rows = vis.any(axis=1)
        for h in range(heads):
            sl = slice(h * d, (h + 1) * d)
            s = np.where(vis, scale * (np.asarray(q[b, :, sl], np.float64) @ np.asarray(k[b, :, sl], np.float64).T), -np.inf)[rows]
            m = s.max(axis=1, keepdims=True)
            e = np.exp(s - m)
            z = e.sum(axis=1, keepdims=True)
            out[b, rows, sl] = (e / z) @ np.where(vis.any(axis=0)[:, None], np.asarray(v[b, :, sl], np.float64), 0.0)
            lse[b, h, rows] = (m + np.log(z))[:, 0]
    return out, lse
