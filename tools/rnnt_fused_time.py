#!/usr/bin/env python3
"""What the fused transducer training loss costs (csrc/hip/rnnt_fused.hip) against the composed five-call route it replaces:
python tools/rnnt_fused_time.py [repeats] > profiles/rnnt_fused_time.json      (timed by tools/timing.py)
Per shape (batch, T, U = max_label_len, V, J), in one process: the fused call, loss only and with the gradients; the composed route
(nntk_rnnt_joint_device, the training Dense, nntk_rnnt_loss_device, the Dense gradient, nntk_rnnt_joint_backward_device), forward only and
with the gradients; the device bytes each route allocates for its intermediates; and the fraction of the exact-f32 MFMA peak the fused
call reaches, counting 2 J V flops per live cell and product (1 product forward; 5 with the gradients: the forward's, its recomputation
twice, d z and d W)."""
import ctypes as C
import sys
import numpy as np
import torch
from timing import emit, open_device, ragged, timed
from nntoolkitcore_amd import capi, layers as NL

SHAPES = ((16, 200, 40, 512, 512), (4, 100, 20, 1024, 640), (4, 100, 20, 4096, 512))
WARMUP = 2
PEAK_F32_MFMA = 157.3e12                                  # MI355X, dense f32 matrix


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    L = open_device()
    dp = lambda t: C.c_void_p(t.data_ptr())
    out = {"tool": "rnnt_fused_time", "repeats": repeats, "warmup": WARMUP, "source_hash": L.nntk_build_source_hash().decode(),
           "peak_f32_mfma_flops": PEAK_F32_MFMA, "shapes": []}
    for B, T, U, V, J in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(B + T + V)
        rng = np.random.default_rng(T)
        lab = rng.integers(1, V, (B, U)).astype(np.int32)
        ll = ragged(rng, U, B)
        il = ragged(rng, T, B)
        live = int((il.astype(np.int64) * (ll + 1)).sum())
        U1, rows = U + 1, B * T * (U + 1)
        enc, pred = torch.rand((B, T, J), device="cuda", generator=g) - 0.5, torch.rand((B, U1, J), device="cuda", generator=g) - 0.5
        w = (torch.rand(J * V + V, device="cuda", generator=g) - 0.5) * (4.0 / np.sqrt(J))
        loss, denc, dpred, dw = torch.empty(B, device="cuda"), torch.empty_like(enc), torch.empty_like(pred), torch.empty_like(w)
        # ---- fused ----
        ws0 = torch.empty(L.nntk_rnnt_fused_workspace_floats(B, T, U, J, V, 0), device="cuda")
        ws1 = torch.empty(L.nntk_rnnt_fused_workspace_floats(B, T, U, J, V, 1), device="cuda")
        t_f0 = timed(lambda: NL.rnnt_fused_loss_device(enc, pred, w, lab, ll, il, 0, "tanh", want_grad=False, loss=loss, workspace=ws0), repeats, WARMUP)
        t_f1 = timed(lambda: NL.rnnt_fused_loss_device(enc, pred, w, lab, ll, il, 0, "tanh", loss=loss, denc=denc, dpred=dpred, dout=dw,
                                                       workspace=ws1), repeats, WARMUP)
        fused_loss = loss.clone()
        assert torch.isfinite(loss).all() and torch.isfinite(denc).all() and torch.isfinite(dpred).all() and torch.isfinite(dw).all()
        fused_bytes = (4 * ws0.numel(), 4 * ws1.numel())
        del ws0, ws1
        torch.cuda.empty_cache()
        # ---- composed: five calls, the tensors of [B][T][U1][J] and [B][T][U1][V] all stored ----
        dense = L.DenseCreateForTraining(L.DenseConfigCreate(J, V, None), capi.ConvTrainingConfig(rows))
        assert dense, capi.last_error()
        assert L.DenseLoadWeightsDevice(dense, dp(w)) == 0, capi.last_error()
        joint, logits = torch.empty((B, T, U1, J), device="cuda"), torch.empty((B, T, U1, V), device="cuda")
        dlogits, djoint = torch.empty_like(logits), torch.empty_like(joint)
        wsl = torch.empty(L.nntk_rnnt_workspace_floats(B, T, U, 1), device="cuda")

        def forward(want_grad):
            NL.rnnt_joint_device(enc, pred, "tanh", out=joint)
            assert L.DenseApplyTrainingBatchDevice(dense, dp(joint), dp(logits)) == 0, capi.last_error()
            NL.rnnt_loss_device(logits, lab, ll, il, 0, want_grad=want_grad, loss=loss, dlogits=dlogits if want_grad else None, workspace=wsl)

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
        flop = 2.0 * live * J * V
        out["shapes"].append({
            "B": B, "T": T, "U": U, "V": V, "J": J, "cells": rows, "live_cells": live,
            "fused_loss_ms": t_f0[0], "fused_loss_ms_min_max": t_f0[1:], "fused_loss_grad_ms": t_f1[0], "fused_loss_grad_ms_min_max": t_f1[1:],
            "composed_loss_ms": t_c0[0], "composed_loss_ms_min_max": t_c0[1:], "composed_loss_grad_ms": t_c1[0],
            "composed_loss_grad_ms_min_max": t_c1[1:],
            "fused_workspace_bytes_loss": fused_bytes[0], "fused_workspace_bytes_loss_grad": fused_bytes[1],
            "composed_intermediate_bytes_loss": composed_bytes[0], "composed_intermediate_bytes_loss_grad": composed_bytes[1],
            "composed_dense_layer_buffers": "not counted (owned by the training Dense: at least one more [rows][J] and [rows][V])",
            "fused_loss_fraction_of_f32_mfma_peak": flop / (1e-3 * t_f0[0]) / PEAK_F32_MFMA,
            "fused_loss_grad_fraction_of_f32_mfma_peak": 5 * flop / (1e-3 * t_f1[0]) / PEAK_F32_MFMA,
            "loss_rows_max_relative_difference_fused_vs_composed": rel})
        del joint, logits, dlogits, djoint, wsl
        torch.cuda.empty_cache()
    emit(out)


if __name__ == "__main__":
    main()
