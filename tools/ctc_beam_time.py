#!/usr/bin/env python3
"""What the CTC prefix beam search costs (csrc/hip/ctc_beam.hip), next to the greedy decoder in the same run:
python tools/ctc_beam_time.py [repeats]      -> one JSON line, also written to profiles/ctc_beam_time.json
Shapes and inputs are those of tools/ctc_time.py; beam_width 1, 16 and 64, nbest = min(beam_width, 4).  Where beam_width * C passes
the 16384 candidate cells of a frame the class cut is set to 40 (and recorded).  HIP events, warm-up, median of the repeats.  The
serial chain of a row is its T frames: us_per_frame = the call's time / (T * waves of rows), waves = ceil(B / CUs) since the beam
kernel's LDS lets one row live on a CU at a time once the cells pass half of it -- an upper bound of a frame's time."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from nntoolkitcore_amd import capi, layers as NL

SHAPES = ((512, 1000, 1000), (512, 250, 40))
WIDTHS = (1, 16, 64)
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
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    assert torch.cuda.is_available(), "needs the GPU"
    torch.cuda.set_device(0); L = capi.load(); NL.use_torch_stream()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = {"tool": "ctc_beam_time", "repeats": repeats, "warmup": WARMUP, "source_hash": L.nntk_build_source_hash().decode(),
           "compute_units": cus, "shapes": []}
    for B, T, Cc in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(B + T + Cc)
        probs = torch.softmax(4 * torch.rand((B, T, Cc), device="cuda", generator=g) - 2, -1)
        rng = np.random.default_rng(T)
        il = rng.integers(T // 2, T + 1, B).astype(np.int32); il[0] = T
        dec, dn = torch.empty((B, T), dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
        t_dec = timed(lambda: NL.ctc_greedy_decode_device(probs, il, 0, labels_out=dec, out_lengths=dn), repeats)
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
                      repeats)
            assert torch.isfinite(sc[:, 0]).all() and (n[:, 0] >= 0).all()
            row["beam"].append({"beam_width": W, "cutoff_top_n": cut, "nbest": nbest, "ms": t[0], "ms_min_max": t[1:],
                                "over_greedy": t[0] / t_dec[0], "row_waves": waves, "us_per_frame": 1e3 * t[0] / (T * waves),
                                "frames_per_s": float(il.sum()) / (1e-3 * t[0])})
            del ws
        out["shapes"].append(row)
        del probs
        torch.cuda.empty_cache()
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "ctc_beam_time.json"), "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
