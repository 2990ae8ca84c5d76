#!/usr/bin/env python3
"""What the CTC calls cost (csrc/hip/ctc.hip), next to torch.nn.functional.ctc_loss on the same GPU and inputs:
python tools/ctc_time.py [repeats]      -> one JSON line (timed by tools/timing.py)
Per shape: the loss alone, loss + gradient, the greedy decode; torch forward and forward + backward (torch is handed the
log-probabilities ready made, [T][B][C] as it wants them); the gradient's bytes over the time the gradient adds to the call, and
the loss-only call's time per timestep (that call is the alpha recursion and nothing else)."""
import sys
import numpy as np
import torch
from timing import emit, open_device, ragged, timed
from nntoolkitcore_amd import layers as NL

SHAPES = ((512, 1000, 1000, 100), (512, 250, 40, 60))
WARMUP = 2


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    L = open_device()
    out = {"tool": "ctc_time", "repeats": repeats, "warmup": WARMUP, "source_hash": L.nntk_build_source_hash().decode(), "shapes": []}
    for B, T, Cc, ML in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(B + T + Cc)
        probs = torch.softmax(4 * torch.rand((B, T, Cc), device="cuda", generator=g) - 2, -1)
        rng = np.random.default_rng(T)
        lab = rng.integers(1, Cc, (B, ML)).astype(np.int32)
        lab[:, 1:] = np.where(lab[:, 1:] == lab[:, :-1], 1 + lab[:, 1:] % (Cc - 1), lab[:, 1:])     # mostly no repeats; feasible anyway: T >= 2 ML
        ll = ragged(rng, ML, B)
        il = rng.integers(max(2 * ML, T // 2), T + 1, B).astype(np.int32); il[0] = T
        ws = torch.empty(L.nntk_ctc_workspace_floats(B, T, ML), device="cuda")
        loss, dprobs = torch.empty(B, device="cuda"), torch.empty_like(probs)
        dec, dn = torch.empty((B, T), dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
        t_loss = timed(lambda: NL.ctc_loss_device(probs, lab, ll, il, 0, want_grad=False, loss=loss, workspace=ws), repeats, WARMUP)
        t_grad = timed(lambda: NL.ctc_loss_device(probs, lab, ll, il, 0, want_grad=True, loss=loss, dprobs=dprobs, workspace=ws), repeats, WARMUP)
        t_dec = timed(lambda: NL.ctc_greedy_decode_device(probs, il, 0, labels_out=dec, out_lengths=dn), repeats, WARMUP)
        ours = loss.clone()
        assert torch.isfinite(ours).all() and torch.isfinite(dprobs).all()
        lp = torch.log(probs).transpose(0, 1).contiguous().requires_grad_(True)
        tl, tll, til = torch.from_numpy(lab.astype(np.int64)).cuda(), torch.from_numpy(ll.astype(np.int64)), torch.from_numpy(il.astype(np.int64))
        keep = {}

        def t_fwd():
            keep["l"] = torch.nn.functional.ctc_loss(lp, tl, til, tll, blank=0, reduction="none")

        def t_fwd_bwd():
            lp.grad = None
            torch.nn.functional.ctc_loss(lp, tl, til, tll, blank=0, reduction="sum").backward()

        tt_f = timed(t_fwd, repeats, WARMUP)
        tt_fb = timed(t_fwd_bwd, repeats, WARMUP)
        rel = float(((keep["l"].detach() - ours).abs() / keep["l"].detach().abs()).max())
        gbytes = 4.0 * B * T * Cc
        out["shapes"].append({
            "B": B, "T": T, "C": Cc, "L": ML,
            "loss_ms": t_loss[0], "loss_ms_min_max": t_loss[1:], "loss_grad_ms": t_grad[0], "loss_grad_ms_min_max": t_grad[1:],
            "decode_ms": t_dec[0], "decode_ms_min_max": t_dec[1:],
            "torch_fwd_ms": tt_f[0], "torch_fwd_bwd_ms": tt_fb[0], "torch_fwd_bwd_ms_min_max": tt_fb[1:],
            "speedup_loss_grad_vs_torch": tt_fb[0] / t_grad[0],
            "recursion_us_per_timestep": 1e3 * t_loss[0] / T,
            "gradient_bytes": gbytes, "gradient_bytes_per_s_over_added_time": gbytes / (1e-3 * max(t_grad[0] - t_loss[0], 1e-6)),
            "gradient_bytes_per_s_over_whole_call": gbytes / (1e-3 * t_grad[0]),
            "decode_read_bytes_per_s": gbytes / (1e-3 * t_dec[0]),
            "max_rel_diff_loss_vs_torch_gpu": rel})
        del lp, probs, dprobs, ws
        torch.cuda.empty_cache()
    emit(out)


if __name__ == "__main__":
    main()
