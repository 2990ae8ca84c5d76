#!/usr/bin/env python3
"""What the CTC prefix beam search costs (csrc/hip/ctc_beam.hip), next to the greedy decoder in the same run:
python tools/ctc_beam_time.py [repeats]      -> one JSON line, also written to profiles/ctc_beam_time.json
Shapes and inputs are those of tools/ctc_time.py; beam_width 1, 16 and 64, nbest = min(beam_width, 4).  Where beam_width * C passes
the 16384 candidate cells of a frame the class cut is set to 40 (and recorded).  Timed by tools/timing.py.  The
serial chain of a row is its T frames: us_per_frame = the call's time / (T * waves of rows), waves = ceil(B / CUs) since the beam
kernel's LDS lets one row live on a CU at a time once the cells pass half of it -- an upper bound of a frame's time."""
import sys
import numpy as np
import torch
from timing import emit, open_device, ragged, timed
from nntoolkitcore_amd import layers as NL

SHAPES = ((512, 1000, 1000), (512, 250, 40))
WIDTHS = (1, 16, 64)
WARMUP = 2


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    L = open_device()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = {"tool": "ctc_beam_time", "repeats": repeats, "warmup": WARMUP, "source_hash": L.nntk_build_source_hash().decode(),
           "compute_units": cus, "shapes": []}
    for B, T, Cc in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(B + T + Cc)
        probs = torch.softmax(4 * torch.rand((B, T, Cc), device="cuda", generator=g) - 2, -1)
        rng = np.random.default_rng(T)
        il = ragged(rng, T, B)
        dec, dn = torch.empty((B, T), dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
        t_dec = timed(lambda: NL.ctc_greedy_decode_device(probs, il, 0, labels_out=dec, out_lengths=dn), repeats, WARMUP)
        row = {"B": B, "T": T, "C": Cc, "greedy_ms": t_dec[0], "greedy_ms_min_max": t_dec[1:], "beam": []}
        waves = -(-B // cus)
        for W in WIDTHS:
            cut = 0 if W * Cc <= 16384 else 40
            nbest = min(W, 4)
            ws = torch.empty(L.nntk_ctc_beam_workspace_floats(B, T, Cc, W, cut), device="cuda")
            lab = torch.empty((B, nbest, T), dtype=torch.int32, device="cuda")
            n = torch.empty((B, nbest), dtype=torch.int32, device="cuda")
            sc = torch.empty((B, nbest), device="cuda")
            t = timed(lambda: NL.ctc_beam_decode_device(probs, il, 0, W, cut, nbest, labels_out=lab, out_lengths=n, scores=sc, workspace=ws),
                      repeats, WARMUP)
            assert torch.isfinite(sc[:, 0]).all() and (n[:, 0] >= 0).all()
            row["beam"].append({"beam_width": W, "cutoff_top_n": cut, "nbest": nbest, "ms": t[0], "ms_min_max": t[1:],
                                "over_greedy": t[0] / t_dec[0], "row_waves": waves, "us_per_frame": 1e3 * t[0] / (T * waves),
                                "frames_per_s": float(il.sum()) / (1e-3 * t[0])})
            del ws
        out["shapes"].append(row)
        del probs
        torch.cuda.empty_cache()
    emit(out, "ctc_beam_time")


if __name__ == "__main__":
    main()
