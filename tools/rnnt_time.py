#!/usr/bin/env python3
"""What the RNN-Transducer calls cost (csrc/hip/rnnt.hip):
python tools/rnnt_time.py [repeats]      -> one JSON line (timed by tools/timing.py)
Per shape (batch, T, U = max_label_len, V, J): the loss alone, loss + gradient, the joiner and its backward, each with the bytes it
cannot avoid moving and the bytes per second that makes of the measured time.  Minimum traffic: the loss reads the score tensor once;
loss + gradient reads it once and writes the gradient once (the call reads it twice: 3 tensor passes against 2); the joiner writes its
output once (its inputs are smaller by a factor U1 or T); the backward reads dout and, for tanh, out, once."""
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
    out = {"tool": "rnnt_time", "repeats": repeats, "warmup": WARMUP, "source_hash": L.nntk_build_source_hash().decode(), "shapes": []}
    for B, T, U, V, J in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(B + T + V)
        logits = 4 * torch.rand((B, T, U + 1, V), device="cuda", generator=g) - 2
        rng = np.random.default_rng(T)
        lab = rng.integers(1, V, (B, U)).astype(np.int32)
        ll = ragged(rng, U, B)
        il = ragged(rng, T, B)
        ws = torch.empty(L.nntk_rnnt_workspace_floats(B, T, U, 1), device="cuda")
        loss, dlogits = torch.empty(B, device="cuda"), torch.empty_like(logits)
        t_loss = timed(lambda: NL.rnnt_loss_device(logits, lab, ll, il, 0, want_grad=False, loss=loss, workspace=ws), repeats, WARMUP)
        t_grad = timed(lambda: NL.rnnt_loss_device(logits, lab, ll, il, 0, want_grad=True, loss=loss, dlogits=dlogits, workspace=ws), repeats, WARMUP)
        assert torch.isfinite(loss).all() and torch.isfinite(dlogits).all()
        enc, pred = torch.rand((B, T, J), device="cuda", generator=g) - 0.5, torch.rand((B, U + 1, J), device="cuda", generator=g) - 0.5
        joint, denc, dpred = torch.empty((B, T, U + 1, J), device="cuda"), torch.empty_like(enc), torch.empty_like(pred)
        dout = torch.rand((B, T, U + 1, J), device="cuda", generator=g) - 0.5
        t_j = timed(lambda: NL.rnnt_joint_device(enc, pred, "tanh", out=joint), repeats, WARMUP)
        t_jb = timed(lambda: NL.rnnt_joint_backward_device(joint, dout, "tanh", denc=denc, dpred=dpred), repeats, WARMUP)
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
    emit(out)


if __name__ == "__main__":
    main()
