#!/usr/bin/env python3
"""What transducer beam search costs (csrc/hip/rnnt_beam.hip), next to greedy decoding of the same model and frames:
python tools/rnnt_beam_time.py [repeats]      -> profiles/rnnt_beam_time.json and the same JSON line on stdout
Model E = H = J = 512, V = 1024, T = 100, tanh joiner, with the projection, max_symbols_per_frame 3; batch 16.  `beam_ms`: one
nntk_rnnt_beam_decode_device call at beam_width 1, 4 and 8 (nbest = beam_width; timed by tools/timing.py);
`greedy_ms`: one nntk_rnnt_greedy_decode_device call, measured the same way; `ratio_to_greedy` their quotient.  All numbers are
reported as measured; nothing is asserted."""
import sys
import numpy as np
import torch
from timing import emit, open_device, timed
from nntoolkitcore_amd import layers as NL

E = H = J = 512
V, T, BLANK, MAX_SYMBOLS, BATCH = 1024, 100, 0, 3, 16
WIDTHS = (1, 4, 8)
WARMUP = 1


def model(rng):
    u = lambda sc, *s: rng.uniform(-sc, sc, s).astype(np.float32)
    G = 4 * H
    bias = u(0.1, V)
    bias[1:] -= np.float32(3.0)                      # about one label in four decisions
    return dict(embed=u(1.0, V, E), W=u(2.0 * E ** -0.5, E, G), U=u(2.0 * H ** -0.5, H, G), b_i=u(0.1, G), b_h=u(0.1, G),
                Wp=u(2.0 * H ** -0.5, H, J), bp=u(0.1, J), Wo=u(3.0 * J ** -0.5, J, V), bo=bias)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    L = open_device()
    rng = np.random.default_rng(2024)
    m = model(rng)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dec = NL.RnntDecoder(d(m["embed"]), d(np.concatenate([m["W"].ravel(), m["U"].ravel(), m["b_i"], m["b_h"]])),
                         d(np.concatenate([m["Wp"].ravel(), m["bp"]])), d(np.concatenate([m["Wo"].ravel(), m["bo"]])), blank=BLANK,
                         joint_activation="tanh", max_symbols_per_frame=MAX_SYMBOLS)
    enc = d(rng.uniform(-1.5, 1.5, (BATCH, T, J)).astype(np.float32))
    ML = MAX_SYMBOLS * T
    g_outs = dec._outputs(enc.device, BATCH, ML)
    greedy_ms, greedy_mm = timed(lambda: dec._decode(None, enc, None, ML, g_outs), repeats, WARMUP).pair
    g_len, g_lab, g_sc = g_outs[2].cpu().numpy(), g_outs[0].cpu().numpy(), g_outs[3].cpu().numpy()
    out = {"tool": "rnnt_beam_time", "repeats": repeats, "warmup": WARMUP, "source_hash": L.nntk_build_source_hash().decode(),
           "model": {"E": E, "H": H, "J": J, "V": V, "T": T, "batch": BATCH, "max_symbols_per_frame": MAX_SYMBOLS},
           "greedy_ms": greedy_ms, "greedy_ms_min_max": greedy_mm, "greedy_labels_total": int(g_len.sum()), "widths": []}
    for W in WIDTHS:
        outs = dec._beam_outputs(enc.device, BATCH, W, ML)
        ws = dec._beam_workspace(enc.device, BATCH, W, ML)
        ms, mm = timed(lambda: dec._beam(None, enc, None, W, W, ML, outs, ws), repeats, WARMUP).pair
        lab, ln, sc = (o.cpu().numpy() for o in outs)
        same = sum(lab[b, 0, :ln[b, 0]].tolist() == g_lab[b, :g_len[b]].tolist() for b in range(BATCH))
        out["widths"].append({"beam_width": W, "beam_ms": ms, "beam_ms_min_max": mm, "ratio_to_greedy": ms / greedy_ms,
                              "hypotheses_per_pass": int(L.nntk_shim_rnnt_beam_group(W, H, J, V)),
                              "workspace_mib": float(ws.numel() * 4 / 2 ** 20), "rows_whose_best_is_the_greedy_labels": int(same),
                              "rows_whose_best_score_is_at_least_greedy": int((sc[:, 0] >= g_sc - 1e-3).sum())})
    emit(out, "rnnt_beam_time")


if __name__ == "__main__":
    main()
