#!/usr/bin/env python3
"""What the RNN-Transducer calls cost (csrc/hip/rnnt.hip):
python tools/rnnt_time.py [repeats]      -> one JSON line (HIP events, warm-up, median of the repeats)
Per shape (batch, T, U = max_label_len, V, J): the loss alone, loss + gradient, the joiner and its backward, each with the bytes it
cannot avoid moving and the bytes per second that makes of the measured time.  Minimum traffic: the loss reads the score tensor once;
loss + gradient reads it once and writes the gradient once (the call reads it twice: 3 tensor passes against 2); the joiner writes its
output once (its inputs are smaller by a factor U1 or T); the backward reads dout and, for tanh, out, once."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from nntoolkitcore_amd import capi, layers as NL

SHAPES = ((16, 200, 40, 512, 512), (4, 100, 20, 1024, 640))
WARMUP = 2


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
    out = {"tool": "rnnt_time", "repeats": repeats, "warmup": WARMUP, "source_hash": L.nntk_build_source_hash().decode(), "shapes": []}
    for B, T, U, V, J in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(B + T + V)
        logits = 4 * torch.rand((B, T, U + 1, V), device="cuda", generator=g) - 2
        rng = np.random.default_rng(T)
        lab = rng.integers(1, V, (B, U)).astype(np.int32)
        ll = rng.integers(U // 2, U + 1, B).astype(np.int32); ll[0] = U
        il = rng.integers(T // 2, T + 1, B).astype(np.int32); il[0] = T
        ws = torch.empty(L.nntk_rnnt_workspace_floats(B, T, U, 1), device="cuda")
        loss, dlogits = torch.empty(B, device="cuda"), torch.empty_like(logits)
        t_loss = timed(lambda: NL.rnnt_loss_device(logits, lab, ll, il, 0, want_grad=False, loss=loss, workspace=ws), repeats)
        t_grad = timed(lambda: NL.rnnt_loss_device(logits, lab, ll, il, 0, want_grad=True, loss=loss, dlogits=dlogits, workspace=ws), repeats)
        assert torch.isfinite(loss).all() and torch.isfinite(dlogits).all()
        enc, pred = torch.rand((B, T, J), device="cuda", generator=g) - 0.5, torch.rand((B, U + 1, J), device="cuda", generator=g) - 0.5
        joint, denc, dpred = torch.empty((B, T, U + 1, J), device="cuda"), torch.empty_like(enc), torch.empty_like(pred)
        dout = torch.rand((B, T, U + 1, J), device="cuda", generator=g) - 0.5
        t_j = timed(lambda: NL.rnnt_joint_device(enc, pred, "tanh", out=joint), repeats)
        t_jb = timed(lambda: NL.rnnt_joint_backward_device(joint, dout, "tanh", denc=denc, dpred=dpred), repeats)
        tensor = 4.0 * B * T * (U + 1) * V
        jt = 4.0 * B * T * (U + 1) * J
        out["shapes"].append({
            "B": B, "T": T, "U": U, "V": V, "J": J,
            "loss_ms": t_loss[0], "loss_ms_min_max": t_loss[1:], "loss_grad_ms": t_grad[0], "loss_grad_ms_min_max": t_grad[1:],
            "loss_min_bytes": tensor, "loss_bytes_per_s": tensor / (1e-3 * t_loss[0]),
            "loss_grad_min_bytes": 2 * tensor, "loss_grad_moved_bytes": 3 * tensor,
            "loss_grad_min_bytes_per_s": 2 * tensor / (1e-3 * t_grad[0]), "loss_grad_moved_bytes_per_s": 3 * tensor / (1e-3 * t_grad[0]),
            "joint_ms": t_j[0], "joint_ms_min_max": t_j[1:], "joint_min_bytes": jt, "joint_bytes_per_s": jt / (1e-3 * t_j[0]),
            "joint_backward_ms": t_jb[0], "joint_backward_ms_min_max": t_jb[1:], "joint_backward_min_bytes": 2 * jt,
            "joint_backward_moved_bytes": 4 * jt, "joint_backward_min_bytes_per_s": 2 * jt / (1e-3 * t_jb[0]),
            "joint_backward_moved_bytes_per_s": 4 * jt / (1e-3 * t_jb[0])})
        del logits, dlogits, ws, joint, dout
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
