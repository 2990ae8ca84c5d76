#!/usr/bin/env python3
"""What the fused token-and-duration training loss costs (csrc/hip/rnnt_tdt_fused.hip) against the composed five-call route it replaces:
python tools/rnnt_tdt_fused_time.py [repeats] > profiles/rnnt_tdt_fused_time.json      (timed by tools/timing.py)
Per shape (batch, T, U = max_label_len, V, J) with durations 0 .. 4, in one process: the fused call, loss only and with the gradients;
the composed route on device pointers (nntk_rnnt_joint_device, the training Dense of width V + D, nntk_rnnt_tdt_loss_device, the Dense
gradient, nntk_rnnt_joint_backward_device), forward only and with the gradients; and the device bytes each route allocates for its
intermediates."""
import ctypes as C
import sys
import numpy as np
import torch
from timing import emit, open_device, ragged, timed
from nntoolkitcore_amd import capi, layers as NL

SHAPES = ((16, 200, 40, 1024, 640), (4, 100, 20, 1024, 640))        # the grids of tools/rnnt_tdt_time.py, V + D = 1029
DURATIONS = [0, 1, 2, 3, 4]
WARMUP = 2


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    L = open_device()
    dp = lambda t: C.c_void_p(t.data_ptr())
    D = len(DURATIONS)
    out = {"tool": "rnnt_tdt_fused_time", "repeats": repeats, "warmup": WARMUP, "source_hash": L.nntk_build_source_hash().decode(),
           "durations": DURATIONS, "shapes": []}
    for B, T, U, V, J in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(B + T + V)
        rng = np.random.default_rng(T)
        lab = rng.integers(1, V, (B, U)).astype(np.int32)
        ll, il = ragged(rng, U, B), ragged(rng, T, B)
        U1, VD, rows = U + 1, V + D, B * T * (U + 1)
        enc, pred = torch.rand((B, T, J), device="cuda", generator=g) - 0.5, torch.rand((B, U1, J), device="cuda", generator=g) - 0.5
        w = (torch.rand(J * VD + VD, device="cuda", generator=g) - 0.5) * (4.0 / np.sqrt(J))
        loss, denc, dpred, dw = torch.empty(B, device="cuda"), torch.empty_like(enc), torch.empty_like(pred), torch.empty_like(w)
        # ---- fused ----
        ws0 = torch.empty(L.nntk_rnnt_tdt_fused_workspace_floats(B, T, U, J, V, D, 0), device="cuda")
        ws1 = torch.empty(L.nntk_rnnt_tdt_fused_workspace_floats(B, T, U, J, V, D, 1), device="cuda")
        fused = lambda grad, ws: NL.rnnt_tdt_fused_loss_device(enc, pred, w, lab, DURATIONS, ll, il, 0, 0.0, "tanh", want_grad=grad, loss=loss,
                                                               denc=denc, dpred=dpred, dout=dw, workspace=ws)
        t_f0 = timed(lambda: fused(False, ws0), repeats, WARMUP)
        t_f1 = timed(lambda: fused(True, ws1), repeats, WARMUP)
        fused_loss = loss.clone()
        assert torch.isfinite(loss).all() and torch.isfinite(denc).all() and torch.isfinite(dpred).all() and torch.isfinite(dw).all()
        fused_bytes = (4 * ws0.numel(), 4 * ws1.numel())
        del ws0, ws1
        torch.cuda.empty_cache()
        # ---- composed: five calls, the tensors of [B][T][U1][J] and [B][T][U1][V + D] all stored ----
        dense = L.DenseCreateForTraining(L.DenseConfigCreate(J, VD, None), capi.ConvTrainingConfig(rows))
        assert dense, capi.last_error()
        assert L.DenseLoadWeightsDevice(dense, dp(w)) == 0, capi.last_error()
        joint, logits = torch.empty((B, T, U1, J), device="cuda"), torch.empty((B, T, U1, VD), device="cuda")
        dlogits, djoint = torch.empty_like(logits), torch.empty_like(joint)
        wsl = torch.empty(L.nntk_rnnt_tdt_workspace_floats(B, T, U, D, 1), device="cuda")

        def forward(want_grad):
            NL.rnnt_joint_device(enc, pred, "tanh", out=joint)
            assert L.DenseApplyTrainingBatchDevice(dense, dp(joint), dp(logits)) == 0, capi.last_error()
            NL.rnnt_tdt_loss_device(logits, lab, DURATIONS, ll, il, 0, want_grad=want_grad, loss=loss, dlogits=dlogits if want_grad else None,
                                    workspace=wsl)

        def both():
            forward(True)
            dw.zero_()
            assert L.DenseCalculateGradientDevice(dense, dp(dw), dp(djoint), dp(dlogits)) == 0, capi.last_error()
            NL.rnnt_joint_backward_device(joint, djoint, "tanh", denc=denc, dpred=dpred)

        t_c0 = timed(lambda: forward(False), repeats, WARMUP)
        t_c1 = timed(both, repeats, WARMUP)
        rel = float(((loss - fused_loss).abs() / fused_loss.abs()).max())
        composed_bytes = (4 * (joint.numel() + logits.numel() + wsl.numel()),
                          4 * (joint.numel() + logits.numel() + dlogits.numel() + djoint.numel() + wsl.numel()))
        L.DenseDestroy(dense)
        out["shapes"].append({
            "B": B, "T": T, "U": U, "V": V, "D": D, "J": J, "cells": rows,
            "fused_loss_ms": t_f0[0], "fused_loss_ms_min_max": t_f0[1:], "fused_loss_grad_ms": t_f1[0], "fused_loss_grad_ms_min_max": t_f1[1:],
            "composed_loss_ms": t_c0[0], "composed_loss_ms_min_max": t_c0[1:], "composed_loss_grad_ms": t_c1[0],
            "composed_loss_grad_ms_min_max": t_c1[1:],
            "fused_workspace_bytes_loss": fused_bytes[0], "fused_workspace_bytes_loss_grad": fused_bytes[1],
            "composed_intermediate_bytes_loss": composed_bytes[0], "composed_intermediate_bytes_loss_grad": composed_bytes[1],
            "composed_dense_layer_buffers": "not counted (owned by the training Dense: at least one more [rows][J] and [rows][V + D])",
            "loss_rows_max_relative_difference_fused_vs_composed": rel})
        del joint, logits, dlogits, djoint, wsl
        torch.cuda.empty_cache()
    emit(out)


if __name__ == "__main__":
    main()
