#!/usr/bin/env python3
"""What RNN-Transducer forced alignment costs (csrc/hip/rnnt_align.hip), next to the loss-only calls at the same shapes in the same run:
python tools/rnnt_align_time.py [repeats]      -> one JSON line, also written to profiles/rnnt_align_time.json
The shapes of tools/rnnt_time.py (batch, T, U = max_label_len, V, J), ragged as there.  nntk_rnnt_loss_device / nntk_rnnt_fused_loss_device
without a gradient write the same emissions and run the same serial chain of T_b + U_b diagonals per row, without the backpointer
stores and the backtrace: the yardsticks of the two forms.  HIP events around the whole device call, warm-up, median of the repeats."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from nntoolkitcore_amd import capi, layers as NL

SHAPES = ((16, 200, 40, 512, 512), (4, 100, 20, 1024, 640))
WARMUP = 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn, repeats):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    assert torch.cuda.is_available(), "needs the GPU"
    torch.cuda.set_device(0); L = capi.load(); NL.use_torch_stream()
    out = {"tool": "rnnt_align_time", "repeats": repeats, "warmup": WARMUP, "source_hash": L.nntk_build_source_hash().decode(),
           "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "shapes": []}
    for B, T, U, V, J in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(B + T + V)
        logits = 4 * torch.rand((B, T, U + 1, V), device="cuda", generator=g) - 2
        rng = np.random.default_rng(T)
        lab = rng.integers(1, V, (B, U)).astype(np.int32)
        ll = rng.integers(U // 2, U + 1, B).astype(np.int32); ll[0] = U
        il = rng.integers(T // 2, T + 1, B).astype(np.int32); il[0] = T
        dev = dict(device="cuda")
        outs = dict(label_frames=torch.empty((B, U), dtype=torch.int32, **dev), frame_labels=torch.empty((B, T), dtype=torch.int32, **dev),
                    label_logp=torch.empty((B, U), **dev), frame_logp=torch.empty((B, T), **dev), scores=torch.empty(B, **dev))
        loss = torch.empty(B, **dev)
        ws_l = torch.empty(L.nntk_rnnt_workspace_floats(B, T, U, 0), **dev)
        ws = torch.empty(L.nntk_rnnt_align_workspace_floats(B, T, U), **dev)
        t_loss = timed(lambda: NL.rnnt_loss_device(logits, lab, ll, il, 0, want_grad=False, loss=loss, workspace=ws_l), repeats)
        t = timed(lambda: NL.rnnt_align_device(logits, lab, ll, il, 0, workspace=ws, **outs), repeats)
        assert torch.isfinite(loss).all() and torch.isfinite(outs["scores"]).all() and (outs["scores"] <= -loss + 1e-2).all()
        enc, pred = torch.rand((B, T, J), generator=g, **dev) - 0.5, torch.rand((B, U + 1, J), generator=g, **dev) - 0.5
        block = (torch.rand(J * V + V, generator=g, **dev) - 0.5) * (4.0 / J ** 0.5)
        ws_fl = torch.empty(L.nntk_rnnt_fused_workspace_floats(B, T, U, J, V, 0), **dev)
        ws_f = torch.empty(L.nntk_rnnt_fused_align_workspace_floats(B, T, U, J, V), **dev)
        t_floss = timed(lambda: NL.rnnt_fused_loss_device(enc, pred, block, lab, ll, il, 0, "tanh", want_grad=False, loss=loss,
                                                          workspace=ws_fl), repeats)
        t_f = timed(lambda: NL.rnnt_fused_align_device(enc, pred, block, lab, ll, il, 0, "tanh", workspace=ws_f, **outs), repeats)
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
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "rnnt_align_time.json"), "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
