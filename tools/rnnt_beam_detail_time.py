#!/usr/bin/env python3
"""What label timestamps and confidences cost in transducer beam search (csrc/hip/rnnt_beam.hip, the DETAIL instantiations), next to
the plain call:
python tools/rnnt_beam_detail_time.py [repeats] [--acoustic-json OUT] [--parent FILE]... [--same FILE]...
    -> profiles/rnnt_beam_detail_time.json and the same JSON line on stdout
The model, frames and batch of tools/rnnt_beam_lm_time.py (E = H = J = 512, V = 1024, T = 100, tanh joiner, projection,
max_symbols_per_frame 3, batch 16) at beam_width 4 and 8 (nbest = beam_width), timed by tools/timing.py.  Per width:
  acoustic_ms        nntk_rnnt_beam_decode_device
  detail_ms          nntk_rnnt_beam_decode_opt_device with label_frames and label_logps; its labels, lengths and score bits must be the
                     plain call's (detail_bits_equal_acoustic)
  detail_norm_ms     ... with length_norm = 1 as well (only the report differs)
  lm_ms              nntk_rnnt_beam_decode_lm_device with the sparse trigram of tools/rnnt_beam_lm_time.py at alpha 0.5, beta 0.25
  detail_lm_ms       the options call with that model, label_frames and label_logps; bits as lm_ms's (detail_lm_bits_equal_lm)
--acoustic-json OUT measures the plain call only and writes it to OUT: this is how another build of the library (NNTK_LIB, e.g. the
parent commit's) is measured with the same code.  --parent FILE / --same FILE take such files -- of the parent's library, and of
earlier runs of this one -- into the result: per width the parent's figures, and `spread`, the largest relative difference between
two runs of one library in this session, which is the yardstick for `acoustic_vs_parent`.  Nothing but the bits is asserted."""
import json, sys
import numpy as np
import torch
from timing import emit, open_device, timed
from nntoolkitcore_amd import capi, layers as NL
from rnnt_beam_lm_time import WIDTHS, trigram, vs_parent
from rnnt_beam_time import BATCH, BLANK, E, H, J, MAX_SYMBOLS, T, V, WARMUP, model


def main():
    args = sys.argv[1:]
    take = lambda flag: [args[i + 1] for i, a in enumerate(args) if a == flag]
    acoustic_json, parents, sames = take("--acoustic-json"), take("--parent"), take("--same")
    rest = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or not args[i - 1].startswith("--"))]
    repeats = int(rest[0]) if rest else 7
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
    out = {"tool": "rnnt_beam_detail_time", "repeats": repeats, "source_hash": L.nntk_build_source_hash().decode(),
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

    lm = NL.NgramLm.from_arrays(alpha=0.5, beta=0.25, **trigram(np.random.default_rng(7)))
    same = lambda got, want: bool(all(np.array_equal(g.view(np.int32), p.view(np.int32)) for g, p in zip(got, want)))

    def run(W, model_, detail, norm):
        outs = dec._beam_outputs(enc.device, BATCH, W, ML) + (dec._beam_detail_outputs(enc.device, BATCH, W, ML) if detail else ())
        ws = dec._beam_workspace(enc.device, BATCH, W, ML, model_, detail, norm)
        ms, mm = timed(lambda: dec._beam(None, enc, None, W, W, ML, outs, ws, model_, norm), repeats, WARMUP).pair
        return ms, mm, [o.cpu().numpy() for o in outs], ws.numel() * 4 / 2 ** 20

    load = lambda files: [json.load(open(f)) for f in files]
    parent_runs, same_runs = load(parents), load(sames)
    for i, W in enumerate(WIDTHS):
        ms, mm, plain = acoustic(W)
        row = {"beam_width": W, "acoustic_ms": ms, "acoustic_ms_min_max": mm,
               "acoustic_workspace_mib": float(L.nntk_rnnt_beam_workspace_floats(dec.h, BATCH, W, ML) * 4 / 2 ** 20),
               "detail_bytes_per_copied_hypothesis": 8 * ML, "state_bytes_per_copied_hypothesis": 4 * (2 * H + J)}
        dms, dmm, got, mib = run(W, None, True, False)
        row.update(detail_ms=dms, detail_ms_min_max=dmm, detail_over_acoustic=dms / ms, detail_workspace_mib=mib,
                   detail_bits_equal_acoustic=same(got[:3], plain))
        assert row["detail_bits_equal_acoustic"], W
        labelled = int((got[1] > 0).sum())
        row["hypotheses_with_labels"], row["mean_labels"] = labelled, float(got[1][got[1] >= 0].mean())
        nms, nmm, _, _ = run(W, None, True, True)
        row.update(detail_norm_ms=nms, detail_norm_ms_min_max=nmm, detail_norm_over_acoustic=nms / ms)
        lms, lmm, lm_plain, _ = run(W, lm, False, False)
        row.update(lm_ms=lms, lm_ms_min_max=lmm)
        xms, xmm, got, mib = run(W, lm, True, False)
        row.update(detail_lm_ms=xms, detail_lm_ms_min_max=xmm, detail_lm_over_lm=xms / lms, detail_lm_workspace_mib=mib,
                   detail_lm_bits_equal_lm=same(got[:3], lm_plain))
        assert row["detail_lm_bits_equal_lm"], W
        if parent_runs:
            row.update(vs_parent(i, ms, parent_runs, same_runs))
        out["widths"].append(row)
    emit(out, "rnnt_beam_detail_time")


if __name__ == "__main__":
    main()
