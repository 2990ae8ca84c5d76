#!/usr/bin/env python3
"""What one training step of the pruned transducer loss costs (csrc/hip/rnnt_pruned.hip) against the two routes that make the whole lattice:
python tools/rnnt_pruned_time.py [repeats] > profiles/rnnt_pruned_time.json    (timed by tools/timing.py)
Per shape (batch, T, U = max_label_len, V, J) and S, in one process:
  pruned: simple loss with its gradients and the occupancies (on given am [B][T][V] and lm [B][U1][V]), prune ranges, banded joiner, the
    training Dense forward on batch T S rows, banded loss and gradient, the Dense gradient, banded joiner backward -- the whole step and
    each part on its own;
  composed: nntk_rnnt_joint_device, the training Dense on batch T U1 rows, nntk_rnnt_loss_device, the Dense gradient,
    nntk_rnnt_joint_backward_device;
  fused: nntk_rnnt_fused_loss_device with the gradients;
and the device bytes each route allocates for its intermediates.  Lengths ragged as in tools/rnnt_fused_time.py."""
import ctypes as C
import sys
import numpy as np
import torch
from timing import emit, open_device, ragged, timed
from nntoolkitcore_amd import capi, layers as NL

SHAPES = ((16, 200, 40, 512, 512), (4, 100, 20, 4096, 512))
S = 5
WARMUP = 2


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    L = open_device()
    dp = lambda t: C.c_void_p(t.data_ptr())
    out = {"tool": "rnnt_pruned_time", "repeats": repeats, "warmup": WARMUP, "S": S, "source_hash": L.nntk_build_source_hash().decode(),
           "shapes": []}
    for B, T, U, V, J in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(B + T + V)
        rng = np.random.default_rng(T)
        lab = rng.integers(1, V, (B, U)).astype(np.int32)
        ll = ragged(rng, U, B)
        il = ragged(rng, T, B)
        U1 = U + 1
        rnd = lambda *s: torch.rand(s, device="cuda", generator=g) - 0.5
        enc, pred, am, lm = rnd(B, T, J), rnd(B, U1, J), 4 * rnd(B, T, V), 4 * rnd(B, U1, V)
        w = rnd(J * V + V) * (4.0 / np.sqrt(J))
        loss, denc, dpred, dw = torch.empty(B, device="cuda"), torch.empty_like(enc), torch.empty_like(pred), torch.empty_like(w)
        # ---- pruned ----
        dense = L.DenseCreateForTraining(L.DenseConfigCreate(J, V, None), capi.ConvTrainingConfig(B * T * S))
        assert dense, capi.last_error()
        assert L.DenseLoadWeightsDevice(dense, dp(w)) == 0, capi.last_error()
        sloss, dam, dlm, occ = torch.empty(B, device="cuda"), torch.empty_like(am), torch.empty_like(lm), torch.empty((B, T, U1), device="cuda")
        ranges = torch.empty((B, T), dtype=torch.int32, device="cuda")
        joint, logits = torch.empty((B, T, S, J), device="cuda"), torch.empty((B, T, S, V), device="cuda")
        dlogits, djoint = torch.empty_like(logits), torch.empty_like(joint)
        ws_s = torch.empty(L.nntk_rnnt_simple_workspace_floats(B, T, U, 1), device="cuda")
        ws_r = torch.empty(L.nntk_rnnt_prune_workspace_floats(B), device="cuda")
        ws_p = torch.empty(L.nntk_rnnt_pruned_workspace_floats(B, T, U, 1), device="cuda")
        parts = {
            "simple_loss_grad_occ": lambda: NL.rnnt_simple_loss_device(am, lm, lab, ll, il, 0, loss=sloss, dam=dam, dlm=dlm, occ=occ, workspace=ws_s),
            "prune_ranges": lambda: NL.rnnt_prune_ranges_device(occ, ll, S, il, ranges=ranges, workspace=ws_r),
            "banded_joint": lambda: NL.rnnt_pruned_joint_device(enc, pred, ranges, S, "tanh", out=joint),
            "dense_forward": lambda: L.DenseApplyTrainingBatchDevice(dense, dp(joint), dp(logits)),
            "banded_loss_grad": lambda: NL.rnnt_pruned_loss_device(logits, ranges, lab, U, ll, il, 0, loss=loss, dlogits=dlogits, workspace=ws_p),
            "dense_gradient": lambda: (dw.zero_(), L.DenseCalculateGradientDevice(dense, dp(dw), dp(djoint), dp(dlogits))),
            "banded_joint_backward": lambda: NL.rnnt_pruned_joint_backward_device(joint, djoint, ranges, U1, "tanh", denc=denc, dpred=dpred)}

        def step():
            for fn in parts.values():
                fn()

        t_step = timed(step, repeats, WARMUP)
        t_parts = {k: timed(fn, repeats, WARMUP)[0] for k, fn in parts.items()}
        assert torch.isfinite(loss).all() and torch.isfinite(sloss).all() and torch.isfinite(denc).all() and torch.isfinite(dw).all()
        pruned_loss, simple_loss = loss.clone(), sloss.clone()
        pruned_bytes = 4 * sum(t.numel() for t in (dam, dlm, occ, ranges, joint, logits, dlogits, djoint, ws_s, ws_r, ws_p))
        L.DenseDestroy(dense)
        del joint, logits, dlogits, djoint, ws_s, ws_r, ws_p, dam, dlm, occ
        torch.cuda.empty_cache()
        # ---- fused ----
        ws1 = torch.empty(L.nntk_rnnt_fused_workspace_floats(B, T, U, J, V, 1), device="cuda")
        t_f = timed(lambda: NL.rnnt_fused_loss_device(enc, pred, w, lab, ll, il, 0, "tanh", loss=loss, denc=denc, dpred=dpred, dout=dw,
                                                      workspace=ws1), repeats, WARMUP)
        fused_bytes = 4 * ws1.numel()
        full_loss = loss.clone()
        del ws1
        torch.cuda.empty_cache()
        # ---- composed: five calls, the tensors of [B][T][U1][J] and [B][T][U1][V] all stored ----
        rows = B * T * U1
        dense = L.DenseCreateForTraining(L.DenseConfigCreate(J, V, None), capi.ConvTrainingConfig(rows))
        assert dense, capi.last_error()
        assert L.DenseLoadWeightsDevice(dense, dp(w)) == 0, capi.last_error()
        joint, logits = torch.empty((B, T, U1, J), device="cuda"), torch.empty((B, T, U1, V), device="cuda")
        dlogits, djoint = torch.empty_like(logits), torch.empty_like(joint)
        wsl = torch.empty(L.nntk_rnnt_workspace_floats(B, T, U, 1), device="cuda")

        def composed():
            NL.rnnt_joint_device(enc, pred, "tanh", out=joint)
            assert L.DenseApplyTrainingBatchDevice(dense, dp(joint), dp(logits)) == 0, capi.last_error()
            NL.rnnt_loss_device(logits, lab, ll, il, 0, loss=loss, dlogits=dlogits, workspace=wsl)
            dw.zero_()
            assert L.DenseCalculateGradientDevice(dense, dp(dw), dp(djoint), dp(dlogits)) == 0, capi.last_error()
            NL.rnnt_joint_backward_device(joint, djoint, "tanh", denc=denc, dpred=dpred)

        t_c = timed(composed, repeats, WARMUP)
        composed_bytes = 4 * (joint.numel() + logits.numel() + dlogits.numel() + djoint.numel() + wsl.numel())
        L.DenseDestroy(dense)
        out["shapes"].append({
            "B": B, "T": T, "U": U, "V": V, "J": J, "S": S, "lattice_cells": rows, "band_cells": B * T * S,
            "pruned_step_ms": t_step[0], "pruned_step_ms_min_max": t_step[1:], "pruned_parts_ms": t_parts,
            "composed_loss_grad_ms": t_c[0], "composed_loss_grad_ms_min_max": t_c[1:],
            "fused_loss_grad_ms": t_f[0], "fused_loss_grad_ms_min_max": t_f[1:],
            "pruned_intermediate_bytes": pruned_bytes, "composed_intermediate_bytes": composed_bytes, "fused_workspace_bytes": fused_bytes,
            "dense_layer_buffers": "not counted in either Dense route (owned by the training Dense)",
            "am_lm_projections": "not timed: am and lm are given tensors",
            "mean_simple_loss": float(simple_loss.mean()), "mean_pruned_loss": float(pruned_loss.mean()), "mean_full_loss": float(full_loss.mean()),
            "pruned_loss_not_below_full_loss": bool((pruned_loss >= full_loss * (1 - 1e-5)).all())})
        del joint, logits, dlogits, djoint, wsl
        torch.cuda.empty_cache()
    emit(out)


if __name__ == "__main__":
    main()
