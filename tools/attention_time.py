#!/usr/bin/env python3
"""What the attention core costs (csrc/hip/attention.hip), next to torch's f32 attention on the same GPU:
python tools/attention_time.py [repeats]      -> one JSON line, also written to profiles/attention_time.json
16 rows x 8 heads x d_head 64 x 1000 frames (Tq = Tk), with the full, the causal and the chunked mask (chunk 16, left 4).  Per mask:
nntk_attention_device; torch.nn.functional.scaled_dot_product_attention in f32 with the same boolean mask; the plain recipe
softmax(scale q k^T masked) v in f32 matmuls.  The parent commit has no attention path, so torch is the baseline.  Reported: the
ratios this / torch, each mask's time over the full mask's and, next to it, the visible share of the Tq x Tk area that it should
approach; the largest difference from the plain recipe as a check that the three compute the same.  Timed by tools/timing.py."""
import sys
import numpy as np
import torch
from timing import emit, open_device, timed
from nntoolkitcore_amd import layers as NL

B, HEADS, D, T = 16, 8, 64, 1000
MASKS = (("full", {}), ("causal", dict(right=0)), ("chunked", dict(chunk=16, left=4, right=0)))
WARMUP, INNER = 3, 40                    # an event pair spans 40 calls: 4 to 50 ms


def bool_mask(chunk=1, left=-1, right=-1):
    g = torch.arange(T, device="cuda") // chunk
    lo = g[:, None] - left if left >= 0 else torch.full((T, 1), -1, device="cuda")
    hi = g[:, None] + right if right >= 0 else torch.full((T, 1), T, device="cuda")
    return (g[None, :] >= lo) & (g[None, :] <= hi)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    L = open_device()
    torch.backends.cuda.matmul.allow_tf32 = False
    g = torch.Generator(device="cuda").manual_seed(B + T)
    qkv = torch.randn((B, T, 3 * HEADS * D), device="cuda", generator=g)             # one fused projection output
    q, k, v = (qkv[:, :, i * HEADS * D:(i + 1) * HEADS * D] for i in range(3))
    qh, kh, vh = (x.reshape(B, T, HEADS, D).transpose(1, 2).contiguous() for x in (q, k, v))      # torch's [B, heads, T, d]
    out, lse = torch.empty((B, T, HEADS * D), device="cuda"), torch.empty((B, HEADS, T), device="cuda")
    scale = D ** -0.5
    res = {"tool": "attention_time", "repeats": repeats, "warmup": WARMUP, "inner": INNER, "source_hash": L.nntk_build_source_hash().decode(),
           "B": B, "heads": HEADS, "d_head": D, "T": T, "masks": []}
    for name, kw in MASKS:
        mask = bool_mask(**kw)
        recipe = lambda: torch.softmax((scale * (qh @ kh.transpose(2, 3))).masked_fill(~mask, float("-inf")), -1) @ vh
        sdpa = lambda: torch.nn.functional.scaled_dot_product_attention(qh, kh, vh, attn_mask=mask)
        t_this = timed(lambda: NL.attention_device(q, k, v, HEADS, out=out, lse=lse, **kw), repeats, WARMUP, INNER)
        t_sdpa, t_recipe = timed(sdpa, repeats, WARMUP, INNER), timed(recipe, repeats, WARMUP, INNER)
        want = recipe().transpose(1, 2).reshape(B, T, HEADS * D)
        row = {"mask": name, "visible_share": float(mask.float().mean()), "this_ms": t_this.dict, "torch_sdpa_ms": t_sdpa.dict,
               "torch_recipe_ms": t_recipe.dict, "this_over_sdpa": t_this.median / t_sdpa.median,
               "this_over_recipe": t_this.median / t_recipe.median, "max_abs_diff_from_recipe": float((out - want).abs().max())}
        res["masks"].append(row)
    full = res["masks"][0]["this_ms"]["median"]
    for row in res["masks"]:
        row["this_over_full"] = row["this_ms"]["median"] / full
    emit(res, "attention_time")


if __name__ == "__main__":
    main()
