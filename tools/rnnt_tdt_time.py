#!/usr/bin/env python3
"""What the token-and-duration transducer loss costs (csrc/hip/rnnt_tdt.hip) next to the classic loss (csrc/hip/rnnt.hip):
python tools/rnnt_tdt_time.py [repeats]      -> one JSON line (timed by tools/timing.py)
Per shape (batch, T, U = max_label_len, V) and durations 0 .. 4: loss + gradient and the loss alone of both calls on the same
[B][T][U1] grid, the TDT call on V + D columns against V, and the ratio of the two."""
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
    out = {"tool": "rnnt_tdt_time", "repeats": repeats, "warmup": WARMUP, "source_hash": L.nntk_build_source_hash().decode(),
           "durations": DURATIONS, "shapes": []}
    D = len(DURATIONS)
    for B, T, U, V in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(B + T + V)
        x = 4 * torch.rand((B, T, U + 1, V + D), device="cuda", generator=g) - 2
        classic = x[..., :V].contiguous()
        rng = np.random.default_rng(T)
        lab = rng.integers(1, V, (B, U)).astype(np.int32)
        ll, il = ragged(rng, U, B), ragged(rng, T, B)
        ws = torch.empty(L.nntk_rnnt_tdt_workspace_floats(B, T, U, D, 1), device="cuda")
        loss, dx, dc = torch.empty(B, device="cuda"), torch.empty_like(x), torch.empty_like(classic)
        row = {"B": B, "T": T, "U": U, "V": V, "D": D}
        for key, grad in (("loss", False), ("loss_grad", True)):
            t_tdt = timed(lambda: NL.rnnt_tdt_loss_device(x, lab, DURATIONS, ll, il, 0, want_grad=grad, loss=loss, dlogits=dx, workspace=ws),
                          repeats, WARMUP)
            assert torch.isfinite(loss).all()
            t_cls = timed(lambda: NL.rnnt_loss_device(classic, lab, ll, il, 0, want_grad=grad, loss=loss, dlogits=dc, workspace=ws), repeats, WARMUP)
            row.update({"tdt_%s_ms" % key: t_tdt[0], "tdt_%s_ms_min_max" % key: t_tdt[1:], "classic_%s_ms" % key: t_cls[0],
                        "classic_%s_ms_min_max" % key: t_cls[1:], "%s_ratio" % key: t_tdt[0] / t_cls[0]})
        assert torch.isfinite(dx).all()
        out["shapes"].append(row)
        del x, classic, dx, dc, ws
        torch.cuda.empty_cache()
    emit(out)


if __name__ == "__main__":
    main()
