#!/usr/bin/env python3
"""What RNN-Transducer forced alignment costs (csrc/hip/rnnt_align.hip), next to the loss-only calls at the same shapes in the same run:
python tools/rnnt_align_time.py [repeats]      -> one JSON line, also written to profiles/rnnt_align_time.json
The shapes of tools/rnnt_time.py (batch, T, U = max_label_len, V, J), ragged as there.  nntk_rnnt_loss_device / nntk_rnnt_fused_loss_device
without a gradient write the same emissions and run the same serial chain of T_b + U_b diagonals per row, without the backpointer
stores and the backtrace: the yardsticks of the two forms.  Timed by tools/timing.py."""
import sys
import numpy as np
import torch
from timing import emit, open_device, ragged, timed
from nntoolkitcore_amd import layers as NL

SHAPES = ((16, 200, 40, 512, 512), (4, 100, 20, 1024, 640))
WARMUP = 2


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    L = open_device()
    out = {"tool": "rnnt_align_time", "repeats": repeats, "warmup": WARMUP, "source_hash": L.nntk_build_source_hash().decode(),
           "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "shapes": []}
    for B, T, U, V, J in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(B + T + V)
        logits = 4 * torch.rand((B, T, U + 1, V), device="cuda", generator=g) - 2
        rng = np.random.default_rng(T)
        lab = rng.integers(1, V, (B, U)).astype(np.int32)
        ll = ragged(rng, U, B)
        il = ragged(rng, T, B)
        dev = dict(device="cuda")
        outs = dict(label_frames=torch.empty((B, U), dtype=torch.int32, **dev), frame_labels=torch.empty((B, T), dtype=torch.int32, **dev),
                    label_logp=torch.empty((B, U), **dev), frame_logp=torch.empty((B, T), **dev), scores=torch.empty(B, **dev))
        loss = torch.empty(B, **dev)
        ws_l = torch.empty(L.nntk_rnnt_workspace_floats(B, T, U, 0), **dev)
        ws = torch.empty(L.nntk_rnnt_align_workspace_floats(B, T, U), **dev)
        t_loss = timed(lambda: NL.rnnt_loss_device(logits, lab, ll, il, 0, want_grad=False, loss=loss, workspace=ws_l), repeats, WARMUP)
        t = timed(lambda: NL.rnnt_align_device(logits, lab, ll, il, 0, workspace=ws, **outs), repeats, WARMUP)
        assert torch.isfinite(loss).all() and torch.isfinite(outs["scores"]).all() and (outs["scores"] <= -loss + 1e-2).all()
        enc, pred = torch.rand((B, T, J), generator=g, **dev) - 0.5, torch.rand((B, U + 1, J), generator=g, **dev) - 0.5
        block = (torch.rand(J * V + V, generator=g, **dev) - 0.5) * (4.0 / J ** 0.5)
        ws_fl = torch.empty(L.nntk_rnnt_fused_workspace_floats(B, T, U, J, V, 0), **dev)
        ws_f = torch.empty(L.nntk_rnnt_fused_align_workspace_floats(B, T, U, J, V), **dev)
        t_floss = timed(lambda: NL.rnnt_fused_loss_device(enc, pred, block, lab, ll, il, 0, "tanh", want_grad=False, loss=loss,
                                                          workspace=ws_fl), repeats, WARMUP)
        t_f = timed(lambda: NL.rnnt_fused_align_device(enc, pred, block, lab, ll, il, 0, "tanh", workspace=ws_f, **outs), repeats, WARMUP)
        assert torch.isfinite(loss).all() and torch.isfinite(outs["scores"]).all() and (outs["scores"] <= -loss + 1e-2).all()
        out["shapes"].append({
            "B": B, "T": T, "U": U, "V": V, "J": J,
            "loss_only_ms": t_loss[0], "loss_only_ms_min_max": t_loss[1:], "align_ms": t[0], "align_ms_min_max": t[1:],
            "align_over_loss_only": t[0] / t_loss[0],
            "fused_loss_only_ms": t_floss[0], "fused_loss_only_ms_min_max": t_floss[1:], "fused_align_ms": t_f[0],
            "fused_align_ms_min_max": t_f[1:], "fused_align_over_fused_loss_only": t_f[0] / t_floss[0],
            "workspace_MiB": ws.numel() * 4 / 2 ** 20, "fused_workspace_MiB": ws_f.numel() * 4 / 2 ** 20,
            "logits_MiB": logits.numel() * 4 / 2 ** 20, "frames_per_s": float(il.sum()) / (1e-3 * t[0])})
        del logits, ws, ws_l, ws_f, ws_fl
        torch.cuda.empty_cache()
    emit(out, "rnnt_align_time")


if __name__ == "__main__":
    main()
