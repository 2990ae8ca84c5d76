#!/usr/bin/env python3
"""What token-and-duration forced alignment costs (csrc/hip/rnnt_tdt_align.hip):
python tools/rnnt_tdt_align_time.py [repeats]      -> one JSON line, also written to profiles/rnnt_tdt_align_time.json
Per shape (batch, T, U = max_label_len, V) of tools/rnnt_tdt_time.py and durations 0 .. 4: the alignment call with all seven outputs
and with the score alone (no backtrack launch), the loss-only TDT call of the same library on the same grid, and the classic
rnnt_align_device on the token columns.  The expectation to confirm or refute: the alignment costs about the loss-only call -- the same
emit pass, a max-walk in place of a sum-walk -- plus a backtrack that is small next to it.  Each timing is median [min, max] over
`repeats` event pairs: the spread is in the line."""
import sys
import numpy as np
import torch
from timing import emit, open_device, ragged, timed
from nntoolkitcore_amd import layers as NL

SHAPES = ((16, 200, 40, 512), (4, 100, 20, 1024))
DURATIONS = [0, 1, 2, 3, 4]
WARMUP = 2


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    L = open_device()
    out = {"tool": "rnnt_tdt_align_time", "repeats": repeats, "warmup": WARMUP, "source_hash": L.nntk_build_source_hash().decode(),
           "durations": DURATIONS, "shapes": []}
    D = len(DURATIONS)
    for B, T, U, V in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(B + T + V)
        x = 4 * torch.rand((B, T, U + 1, V + D), device="cuda", generator=g) - 2
        classic = x[..., :V].contiguous()
        rng = np.random.default_rng(T)
        lab = rng.integers(1, V, (B, U)).astype(np.int32)
        ll, il = ragged(rng, U, B), ragged(rng, T, B)
        ws = torch.empty(max(L.nntk_rnnt_tdt_align_workspace_floats(B, T, U, D), L.nntk_rnnt_align_workspace_floats(B, T, U)), device="cuda")
        tdt = NL.rnnt_tdt_align_device(x, lab, DURATIONS, ll, il, 0, workspace=ws)
        cls = NL.rnnt_align_device(classic, lab, ll, il, 0, workspace=ws)
        loss = torch.empty(B, device="cuda")
        assert torch.isfinite(tdt[6]).all() and torch.isfinite(cls[4]).all()
        names = ("label_frames", "label_durations", "frame_labels", "frame_durations", "label_logp", "frame_logp", "scores")
        only = dict(zip(names, [False] * 6 + [tdt[6]]))
        calls = {"tdt_align": lambda: NL.rnnt_tdt_align_device(x, lab, DURATIONS, ll, il, 0, workspace=ws, **dict(zip(names, tdt))),
                 "tdt_align_score_only": lambda: NL.rnnt_tdt_align_device(x, lab, DURATIONS, ll, il, 0, workspace=ws, **only),
                 "tdt_loss_only": lambda: NL.rnnt_tdt_loss_device(x, lab, DURATIONS, ll, il, 0, want_grad=False, loss=loss, workspace=ws),
                 "classic_align": lambda: NL.rnnt_align_device(classic, lab, ll, il, 0, workspace=ws, label_frames=cls[0], frame_labels=cls[1],
                                                               label_logp=cls[2], frame_logp=cls[3], scores=cls[4])}
        row = {"B": B, "T": T, "U": U, "V": V, "D": D}
        for key, fn in calls.items():
            t = timed(fn, repeats, WARMUP)
            row.update({key + "_ms": t[0], key + "_ms_min_max": t[1:]})
        assert (tdt[6] <= -loss).all()
        row.update(align_over_loss=row["tdt_align_ms"] / row["tdt_loss_only_ms"], align_over_classic=row["tdt_align_ms"] / row["classic_align_ms"],
                   backtrack_share=1.0 - row["tdt_align_score_only_ms"] / row["tdt_align_ms"])
        out["shapes"].append(row)
        del x, classic, ws, tdt, cls
        torch.cuda.empty_cache()
    emit(out, "rnnt_tdt_align_time")


if __name__ == "__main__":
    main()
