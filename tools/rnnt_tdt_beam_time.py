#!/usr/bin/env python3
"""What token-and-duration beam search costs (csrc/hip/rnnt_tdt_beam.hip) next to the classic beam search at the same H, J, V, W and batch:
python tools/rnnt_tdt_beam_time.py [repeats]      -> profiles/rnnt_tdt_beam_time.json and the same JSON line on stdout
The model of tools/rnnt_beam_time.py (E = H = J = 512, V = 1024, T = 100, tanh joiner, with the projection, max_symbols_per_frame 3); the
TDT model is that model with five duration columns (durations 0 .. 4) behind the same token columns.  Per beam_width (4, 8), batch (1,
16) and call: the milliseconds of one call (tools/timing.py), and for the TDT call what its kernel counted: the frames it joined over the
frames available, and its LSTM steps (the classic search joins every frame and steps W cells a depth).  The classic call is timed twice:
the spread of its two medians is the margin for `tdt_over_classic`.  The weights are random, so the durations the search takes are
arbitrary: the ratio says what the machinery costs at this many joined frames, not what a trained model gains.  Reported as measured."""
import sys
import numpy as np
import torch
from timing import emit, open_device, timed
from nntoolkitcore_amd import layers as NL
from rnnt_tdt_decode_time import BLANK, DURATIONS, E, H, J, MAX_SYMBOLS, V, model

T = 100
WIDTHS, BATCHES = (4, 8), (1, 16)
WARMUP = 1


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    L = open_device()
    rng = np.random.default_rng(2024)
    m = model(rng)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    blocks = (d(m["embed"]), d(np.concatenate([m["W"].ravel(), m["U"].ravel(), m["b_i"], m["b_h"]])), d(np.concatenate([m["Wp"].ravel(), m["bp"]])))
    kw = dict(blank=BLANK, joint_activation="tanh", max_symbols_per_frame=MAX_SYMBOLS)
    classic = NL.RnntDecoder(*blocks, d(np.concatenate([m["Wo"].ravel(), m["bo"]])), **kw)
    tdt = NL.RnntDecoder(*blocks, d(np.concatenate([np.concatenate([m["Wo"], m["Wd"]], 1).ravel(), m["bo"], m["bd"]])), durations=DURATIONS, **kw)
    out = {"tool": "rnnt_tdt_beam_time", "repeats": repeats, "warmup": WARMUP, "source_hash": L.nntk_build_source_hash().decode(),
           "model": {"E": E, "H": H, "J": J, "V": V, "T": T, "max_symbols_per_frame": MAX_SYMBOLS, "durations": list(DURATIONS)}, "runs": []}
    ML = MAX_SYMBOLS * T
    for B in BATCHES:
        enc = d(rng.uniform(-1.5, 1.5, (B, T, J)).astype(np.float32))
        for W in WIDTHS:
            c_outs, c_ws = classic._beam_outputs(enc.device, B, W, ML), classic._beam_workspace(enc.device, B, W, ML)
            run_classic = lambda: classic._beam(None, enc, None, W, W, ML, c_outs, c_ws)
            _, ws = tdt._tdt_beam(enc, None, W, W, ML)
            a = timed(run_classic, repeats, WARMUP)
            t = timed(lambda: tdt._tdt_beam(enc, None, W, W, ML, ws), repeats, WARMUP)
            again = timed(run_classic, repeats, WARMUP)
            stat = ws[(B + 3) // 4 * 4:(B + 3) // 4 * 4 + 2 * B].view(torch.int32).cpu().numpy().reshape(B, 2)      # frames joined | LSTM steps
            out["runs"].append({"batch": B, "beam_width": W, "classic_ms": a.median, "classic_ms_min_max": [a.min, a.max],
                                "classic_again_ms": again.median, "classic_spread": abs(a.median - again.median) / (0.5 * (a.median + again.median)),
                                "tdt_ms": t.median, "tdt_ms_min_max": [t.min, t.max], "tdt_over_classic": t.median / a.median,
                                "tdt_frames_joined": int(stat[:, 0].sum()), "frames_available": B * T,
                                "tdt_frames_joined_longest_row": int(stat[:, 0].max()), "tdt_lstm_steps": int(stat[:, 1].sum()),
                                "hypotheses_per_pass": int(L.nntk_shim_rnnt_tdt_beam_group(W, H, J, V, len(DURATIONS))),
                                "tdt_workspace_mib": float(ws.numel() * 4 / 2 ** 20)})
    emit(out, "rnnt_tdt_beam_time")


if __name__ == "__main__":
    main()
