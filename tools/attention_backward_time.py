#!/usr/bin/env python3
"""What the attention backward costs (csrc/hip/attention_bwd.hip), next to the backward of torch's f32 attention on the same GPU:
python tools/attention_backward_time.py [repeats]      -> one JSON line, also written to profiles/attention_backward_time.json
16 rows x 8 heads x d_head 64 x 1000 frames (Tq = Tk), with the full, the causal and the chunked mask (chunk 16, left 4).  Per mask:
nntk_attention_backward_device into one fused [B, T, 3 HD] gradient buffer; the backward of
torch.nn.functional.scaled_dot_product_attention in f32 with the same boolean mask (torch.autograd.grad on a graph built once, so only
the backward is timed); nntk_attention_device for the ratio backward / forward.  The parent commit has no backward path, so torch is
the only yardstick.  Reported: the ratios this / torch and backward / forward, each mask's time over the full mask's next to its
visible share, and the largest difference from torch's gradients as a check that the two compute the same.  Timed by tools/timing.py."""
import sys
import torch
from timing import emit, open_device, timed
from attention_time import B, D, HEADS, INNER, MASKS, T, WARMUP, bool_mask
from nntoolkitcore_amd import layers as NL


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    L = open_device()
    torch.backends.cuda.matmul.allow_tf32 = False
    g = torch.Generator(device="cuda").manual_seed(B + T)
    HD = HEADS * D
    qkv = torch.randn((B, T, 3 * HD), device="cuda", generator=g)
    dout = torch.randn((B, T, HD), device="cuda", generator=g)
    q, k, v = (qkv[:, :, i * HD:(i + 1) * HD] for i in range(3))
    heads_first = lambda x: x.reshape(B, T, HEADS, D).transpose(1, 2).contiguous()             # torch's [B, heads, T, d]
    qh, kh, vh = (heads_first(x).requires_grad_() for x in (q, k, v))
    doh = heads_first(dout)
    grad = torch.empty((B, T, 3 * HD), device="cuda")
    dq, dk, dv = (grad[:, :, i * HD:(i + 1) * HD] for i in range(3))
    ws = torch.empty(B * HEADS * T, device="cuda")
    res = {"tool": "attention_backward_time", "repeats": repeats, "warmup": WARMUP, "inner": INNER,
           "source_hash": L.nntk_build_source_hash().decode(), "B": B, "heads": HEADS, "d_head": D, "T": T, "masks": []}
    for name, kw in MASKS:
        mask = bool_mask(**kw)
        out, lse = NL.attention_device(q, k, v, HEADS, **kw)
        oh = torch.nn.functional.scaled_dot_product_attention(qh, kh, vh, attn_mask=mask)
        t_this = timed(lambda: NL.attention_backward_device(q, k, v, out, lse, dout, HEADS, dq=dq, dk=dk, dv=dv, workspace=ws, **kw),
                       repeats, WARMUP, INNER)
        t_fwd = timed(lambda: NL.attention_device(q, k, v, HEADS, out=out, lse=lse, **kw), repeats, WARMUP, INNER)
        t_torch = timed(lambda: torch.autograd.grad(oh, (qh, kh, vh), doh, retain_graph=True), repeats, WARMUP, INNER)
        want = torch.autograd.grad(oh, (qh, kh, vh), doh, retain_graph=True)
        diff = max(float((x - w.transpose(1, 2).reshape(B, T, HD)).abs().max()) for x, w in zip((dq, dk, dv), want))
        res["masks"].append({"mask": name, "visible_share": float(mask.float().mean()), "this_ms": t_this.dict, "forward_ms": t_fwd.dict,
                             "torch_sdpa_backward_ms": t_torch.dict, "this_over_torch": t_this.median / t_torch.median,
                             "backward_over_forward": t_this.median / t_fwd.median, "max_abs_diff_from_torch": diff})
    full = res["masks"][0]["this_ms"]["median"]
    for row in res["masks"]:
        row["this_over_full"] = row["this_ms"]["median"] / full
    emit(res, "attention_backward_time")


if __name__ == "__main__":
    main()
