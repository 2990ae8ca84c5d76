#!/usr/bin/env python3
"""What n-gram fusion costs in transducer beam search (csrc/hip/rnnt_beam.hip, the LM instantiations), next to the acoustic call:
python tools/rnnt_beam_lm_time.py [repeats] [--acoustic-json OUT] [--parent FILE]... [--same FILE]...
    -> profiles/rnnt_beam_lm_time.json and the same JSON line on stdout
The model, frames and batch of tools/rnnt_beam_time.py (E = H = J = 512, V = 1024, T = 100, tanh joiner, projection,
max_symbols_per_frame 3, batch 16) at beam_width 4 and 8 (nbest = beam_width), timed by tools/timing.py.  Per width:
  acoustic_ms           nntk_rnnt_beam_decode_device
  fused_no_arcs_ms      nntk_rnnt_beam_decode_lm_device with a one-state table without arcs, alpha = beta = 0, unk_logp 0: every term is
                        +0.0, so the search is the acoustic one step for step; what it costs beyond it is marking and filling lmterm
                        [W][V] and the selection reading it
  fused_unit_trigram_ms the sparse trigram below with alpha = beta = 0: still the acoustic search step for step, now scattering the
                        real backoff chains and looking up the next states
  fused_trigram_ms      the same trigram at alpha 0.5, beta 0.25: another search (the model changes the hypotheses), for information
The trigram: every label in state 0, ten arcs from each one-label context, nine from each of 1024 two-label contexts: about 20 V arcs.
--acoustic-json OUT measures the acoustic call only and writes it to OUT: this is how another build of the library (NNTK_LIB, e.g. the
parent commit's) is measured with the same code.  --parent FILE / --same FILE take such files -- of the parent's library, and of
earlier runs of this one -- into the result: per width the parent's figures, and `spread`, the largest relative difference between
two runs of one library in this session, which is the yardstick for `acoustic_vs_parent`.  Nothing is asserted."""
import json, sys
import numpy as np
import torch
from timing import emit, open_device, timed
from nntoolkitcore_amd import capi, layers as NL
from rnnt_beam_time import BATCH, BLANK, E, H, J, MAX_SYMBOLS, T, V, WARMUP, model

WIDTHS = (4, 8)


def trigram(rng):
    labels = np.arange(1, V)
    arcs = {(): labels.tolist()}
    for a in labels:
        arcs[(int(a),)] = sorted(rng.choice(labels, 10, replace=False).tolist())
    pairs = [(a, b) for (a,), bs in list(arcs.items())[1:] for b in bs]
    for q in rng.choice(len(pairs), 1024, replace=False):
        arcs[pairs[q]] = sorted(rng.choice(labels, 9, replace=False).tolist())
    ctx = sorted(arcs, key=lambda c: (len(c), c))
    sid = {c: i for i, c in enumerate(ctx)}

    def state_of(hist):
        hist = hist[-2:]
        while hist not in sid:
            hist = hist[1:]
        return sid[hist]
    t = dict(n_classes=V, blank=BLANK, arc_begin=[0], arc_label=[], arc_logp=[], arc_next=[], backoff_state=[], backoff_logw=[],
             start_state=0, unk_logp=float(np.log(0.01)))
    for c in ctx:
        for a in arcs[c]:
            t["arc_label"].append(a); t["arc_logp"].append(float(np.log(rng.uniform(0.02, 0.9)))); t["arc_next"].append(state_of(c + (a,)))
        t["arc_begin"].append(len(t["arc_label"]))
        t["backoff_state"].append(-1 if not c else state_of(c[1:]))
        t["backoff_logw"].append(0.0 if not c else float(np.log(rng.uniform(0.2, 0.9))))
    t["final_logp"] = np.log(rng.uniform(0.05, 0.9, len(ctx))).tolist()
    return t


def vs_parent(i, ms, parent_runs, same_runs):
    """width i of --parent / --same files next to this run's acoustic_ms: not the protocol of tools/timing.py, whose children this tool
    does not start -- the files come from whole earlier runs, any number of them, so the spread is (max - min) / min over a library's
    runs and the ratio is median over median"""
    row = {"parent_acoustic_ms": [r["widths"][i]["acoustic_ms"] for r in parent_runs], "parent_source_hash": parent_runs[0]["source_hash"],
           "acoustic_ms_earlier_runs": [r["widths"][i]["acoustic_ms"] for r in same_runs]}
    rel = lambda v: (max(v) - min(v)) / min(v) if len(v) > 1 else None
    mine = row["acoustic_ms_earlier_runs"] + [ms]
    row["spread"] = {"parent_runs": rel(row["parent_acoustic_ms"]), "this_commit_runs": rel(mine)}
    row["acoustic_vs_parent"] = float(np.median(mine) / np.median(row["parent_acoustic_ms"]))
    return row


def main():
    args = sys.argv[1:]
    take = lambda flag: [args[i + 1] for i, a in enumerate(args) if a == flag]
    acoustic_json, parents, sames = take("--acoustic-json"), take("--parent"), take("--same")
    rest = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or not args[i - 1].startswith("--"))]
    repeats = int(rest[0]) if rest else 5
    if acoustic_json:                                # an older build of the library lacks the newest entry points: bind what it exports
        import ctypes
        older = ctypes.CDLL(capi.LIB_PATH)
        for name in [n for n in capi.SIGNATURES if not hasattr(older, n)]:
            del capi.SIGNATURES[name]
    L = open_device()
    rng = np.random.default_rng(2024)
    m = model(rng)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dec = NL.RnntDecoder(d(m["embed"]), d(np.concatenate([m["W"].ravel(), m["U"].ravel(), m["b_i"], m["b_h"]])),
                         d(np.concatenate([m["Wp"].ravel(), m["bp"]])), d(np.concatenate([m["Wo"].ravel(), m["bo"]])), blank=BLANK,
                         joint_activation="tanh", max_symbols_per_frame=MAX_SYMBOLS)
    enc = d(rng.uniform(-1.5, 1.5, (BATCH, T, J)).astype(np.float32))
    ML = MAX_SYMBOLS * T
    out = {"tool": "rnnt_beam_lm_time", "repeats": repeats, "source_hash": L.nntk_build_source_hash().decode(),
           "model": {"E": E, "H": H, "J": J, "V": V, "T": T, "batch": BATCH, "max_symbols_per_frame": MAX_SYMBOLS}, "widths": []}

    def acoustic(W):
        outs, ws = dec._beam_outputs(enc.device, BATCH, W, ML), dec._beam_workspace(enc.device, BATCH, W, ML)
        ms, mm = timed(lambda: L.nntk_rnnt_beam_decode_device(dec.h, None, NL._dp(enc), BATCH, T, None, W, W, ML, NL._ipv(outs[0]),
                                                              NL._ipv(outs[1]), NL._dp(outs[2]), NL._dp(ws)), repeats, WARMUP).pair
        return ms, mm, [o.cpu().numpy() for o in outs]

    if acoustic_json:
        for W in WIDTHS:
            ms, mm, _ = acoustic(W)
            out["widths"].append({"beam_width": W, "acoustic_ms": ms, "acoustic_ms_min_max": mm})
        with open(acoustic_json[0], "w") as fh:
            fh.write(json.dumps(out) + "\n")
        print(json.dumps(out))
        return

    tri = trigram(np.random.default_rng(7))
    empty = dict(n_classes=V, blank=BLANK, arc_begin=[0, 0], arc_label=[], arc_logp=[], arc_next=[], backoff_state=[-1], backoff_logw=[0.0],
                 unk_logp=0.0)
    lms = {"fused_no_arcs": NL.NgramLm.from_arrays(alpha=0.0, beta=0.0, **empty),
           "fused_unit_trigram": NL.NgramLm.from_arrays(alpha=0.0, beta=0.0, **dict(tri, final_logp=None)),
           "fused_trigram": NL.NgramLm.from_arrays(alpha=0.5, beta=0.25, **tri)}
    out["trigram"] = {"states": len(tri["backoff_state"]), "arcs": len(tri["arc_label"]), "arcs_per_class": len(tri["arc_label"]) / V,
                      "lookup_table_bytes": lms["fused_trigram"].device_bytes(), "double_table_bytes": lms["fused_trigram"].rnnt_device_bytes()}
    load = lambda files: [json.load(open(f)) for f in files]
    parent_runs, same_runs = load(parents), load(sames)
    for i, W in enumerate(WIDTHS):
        ms, mm, plain = acoustic(W)
        row = {"beam_width": W, "acoustic_ms": ms, "acoustic_ms_min_max": mm,
               "lm_workspace_mib": float(L.nntk_rnnt_beam_lm_workspace_floats(dec.h, BATCH, W, ML) * 4 / 2 ** 20),
               "acoustic_workspace_mib": float(L.nntk_rnnt_beam_workspace_floats(dec.h, BATCH, W, ML) * 4 / 2 ** 20),
               "lmterm_bytes_per_depth_written_and_read": 8 * W * V}
        for name, lm in lms.items():
            outs, ws = dec._beam_outputs(enc.device, BATCH, W, ML), dec._beam_workspace(enc.device, BATCH, W, ML, lm)
            fms, fmm = timed(lambda: dec._beam(None, enc, None, W, W, ML, outs, ws, lm), repeats, WARMUP).pair
            row[name + "_ms"], row[name + "_ms_min_max"], row[name + "_over_acoustic"] = fms, fmm, fms / ms
            if name != "fused_trigram":             # the unit models must leave the acoustic call's bits
                got = [o.cpu().numpy() for o in outs]
                row[name + "_bits_equal_acoustic"] = bool(all(np.array_equal(g.view(np.int32), p.view(np.int32)) for g, p in zip(got, plain)))
        if parent_runs:
            row.update(vs_parent(i, ms, parent_runs, same_runs))
        out["widths"].append(row)
    emit(out, "rnnt_beam_lm_time")


if __name__ == "__main__":
    main()
