#!/usr/bin/env python3
"""What CTC forced alignment costs (csrc/hip/ctc_align.hip), next to the loss-only CTC call at the same shapes in the same run:
python tools/ctc_align_time.py [repeats]      -> one JSON line, also written to profiles/ctc_align_time.json
B = 512, T = 1000, ragged input lengths as in tools/ctc_beam_time.py; label lengths around 100 (the one-state-per-lane kernel) and one
line at 600 (any-S kernel).  nntk_ctc_loss_device without a gradient runs the same serial chain of T steps per row without the
backpointer stores and the backtrace: the yardstick.  Timed by tools/timing.py."""
import sys
import numpy as np
import torch
from timing import emit, open_device, ragged, timed
from nntoolkitcore_amd import layers as NL

SHAPES = ((512, 1000, 40, 100), (512, 1000, 40, 600))         # B, T, C, max_label_len
WARMUP = 2


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    L = open_device()
    out = {"tool": "ctc_align_time", "repeats": repeats, "warmup": WARMUP, "source_hash": L.nntk_build_source_hash().decode(),
           "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "shapes": []}
    for B, T, Cc, maxL in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(B + T + Cc)
        probs = torch.softmax(4 * torch.rand((B, T, Cc), device="cuda", generator=g) - 2, -1)
        rng = np.random.default_rng(T + maxL)
        il = ragged(rng, T, B)
        ll = rng.integers(maxL - maxL // 5, maxL + 1, B).astype(np.int32); ll[0] = maxL
        ll = np.minimum(ll, il // 2).astype(np.int32)                             # every row has an alignment, repeats included
        lab = rng.integers(1, Cc, (B, maxL)).astype(np.int32)
        loss = torch.empty(B, device="cuda")
        ws_l = torch.empty(L.nntk_ctc_workspace_floats(B, 0, maxL), device="cuda")
        t_loss = timed(lambda: NL.ctc_loss_device(probs, lab, ll, il, 0, want_grad=False, loss=loss, workspace=ws_l), repeats, WARMUP)
        ws = torch.empty(L.nntk_ctc_align_workspace_floats(B, T, maxL), device="cuda")
        st = torch.empty((B, T), dtype=torch.int32, device="cuda")
        sp = torch.empty((B, maxL, 2), dtype=torch.int32, device="cuda")
        sc = torch.empty(B, device="cuda")
        t = timed(lambda: NL.ctc_align_device(probs, lab, ll, il, 0, states=st, spans=sp, scores=sc, workspace=ws), repeats, WARMUP)
        assert torch.isfinite(sc).all() and torch.isfinite(loss).all() and (sc <= -loss + 1e-2).all()
        out["shapes"].append({"B": B, "T": T, "C": Cc, "max_label_len": maxL, "loss_only_ms": t_loss[0], "loss_only_ms_min_max": t_loss[1:],
                              "align_ms": t[0], "align_ms_min_max": t[1:], "align_over_loss_only": t[0] / t_loss[0],
                              "workspace_MiB": ws.numel() * 4 / 2 ** 20, "frames_per_s": float(il.sum()) / (1e-3 * t[0])})
        del ws, probs
        torch.cuda.empty_cache()
    emit(out, "ctc_align_time")


if __name__ == "__main__":
    main()
