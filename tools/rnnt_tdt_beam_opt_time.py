#!/usr/bin/env python3
"""What the options of the token-and-duration beam search cost (csrc/hip/rnnt_tdt_beam.hip, the LM and DETAIL instantiations) over the
plain call, measured in the same run on the same build:
python tools/rnnt_tdt_beam_opt_time.py [repeats]      -> profiles/rnnt_tdt_beam_opt_time.json and the same JSON line on stdout
The model, frames, widths and batches of tools/rnnt_tdt_beam_time.py and the sparse trigram of tools/rnnt_beam_lm_time.py (about 20 V
arcs).  Per beam_width and batch, the milliseconds of one call (tools/timing.py, HIP events): plain, with the trigram at alpha = beta = 0
and no final term (`lm_unit`: the plain search step for step, so the ratio is the cost of the machinery: filling lnF [W][V] each depth,
the selection reading it, the next states), with detail, with both, and with the trigram at alpha 0.5, beta 0.25 (`lm`: another search,
for information).  The plain call is timed twice: the spread of its two medians is the margin for every ratio.  Reported as measured."""
import sys
import numpy as np
import torch
from timing import emit, open_device, timed
from nntoolkitcore_amd import layers as NL
from rnnt_beam_lm_time import trigram
from rnnt_tdt_beam_time import BATCHES, T, WARMUP, WIDTHS
from rnnt_tdt_decode_time import BLANK, DURATIONS, E, H, J, MAX_SYMBOLS, V, model


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    L = open_device()
    rng = np.random.default_rng(2024)
    m = model(rng)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dec = NL.RnntDecoder(d(m["embed"]), d(np.concatenate([m["W"].ravel(), m["U"].ravel(), m["b_i"], m["b_h"]])),
                         d(np.concatenate([m["Wp"].ravel(), m["bp"]])),
                         d(np.concatenate([np.concatenate([m["Wo"], m["Wd"]], 1).ravel(), m["bo"], m["bd"]])), blank=BLANK,
                         joint_activation="tanh", max_symbols_per_frame=MAX_SYMBOLS, durations=DURATIONS)
    tri = trigram(np.random.default_rng(7))
    unit, lm = NL.NgramLm.from_arrays(alpha=0.0, beta=0.0, **dict(tri, final_logp=None)), NL.NgramLm.from_arrays(alpha=0.5, beta=0.25, **tri)
    modes = {"lm_unit": dict(lm=unit), "detail": dict(detail=True), "lm_unit_detail": dict(lm=unit, detail=True), "lm": dict(lm=lm),
             "lm_detail": dict(lm=lm, detail=True)}
    out = {"tool": "rnnt_tdt_beam_opt_time", "repeats": repeats, "warmup": WARMUP, "source_hash": L.nntk_build_source_hash().decode(),
           "model": {"E": E, "H": H, "J": J, "V": V, "T": T, "max_symbols_per_frame": MAX_SYMBOLS, "durations": list(DURATIONS)},
           "trigram": {"states": len(tri["backoff_state"]), "arcs": len(tri["arc_label"])}, "runs": []}
    ML = MAX_SYMBOLS * T
    same = lambda x, y: bool(all(np.array_equal(p.cpu().numpy().view(np.int32), q.cpu().numpy().view(np.int32)) for p, q in zip(x, y)))
    for B in BATCHES:
        enc = d(rng.uniform(-1.5, 1.5, (B, T, J)).astype(np.float32))
        for W in WIDTHS:
            plain, ws = dec._tdt_beam(enc, None, W, W, ML)
            run_plain = lambda: dec._tdt_beam(enc, None, W, W, ML, ws)
            a = timed(run_plain, repeats, WARMUP)
            row = {"batch": B, "beam_width": W, "plain_ms": a.median, "plain_ms_min_max": [a.min, a.max],
                   "plain_workspace_mib": float(ws.numel() * 4 / 2 ** 20)}
            for name, kw in modes.items():
                outs, mws = dec._tdt_beam(enc, None, W, W, ML, **kw)
                t = timed(lambda: dec._tdt_beam(enc, None, W, W, ML, mws, **kw), repeats, WARMUP)
                row.update({name + "_ms": t.median, name + "_ms_min_max": [t.min, t.max], name + "_over_plain": t.median / a.median,
                            name + "_workspace_mib": float(mws.numel() * 4 / 2 ** 20)})
                if "unit" in name or name == "detail":     # these must leave the plain call's three outputs
                    row[name + "_bits_equal_plain"] = same(outs[:3], plain)
            again = timed(run_plain, repeats, WARMUP)
            row.update({"plain_again_ms": again.median, "plain_spread": abs(a.median - again.median) / (0.5 * (a.median + again.median))})
            out["runs"].append(row)
    emit(out, "rnnt_tdt_beam_opt_time")


if __name__ == "__main__":
    main()
