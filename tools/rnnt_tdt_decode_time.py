#!/usr/bin/env python3
"""What token-and-duration greedy decoding costs (csrc/hip/rnnt_tdt_decode.hip) next to the classic greedy call it was modelled on:
python tools/rnnt_tdt_decode_time.py [repeats]      -> profiles/rnnt_tdt_decode_time.json and the same JSON line on stdout
The model of tools/rnnt_decode_time.py (E = H = J = 512, V = 1024, T = 200, tanh joiner, with the projection; batch 1, 16 and 256); the
TDT model is that model with five duration columns (durations 0 .. 4) behind the same token columns.  Per batch and call: the
milliseconds of one call (tools/timing.py), the decisions made, and the microseconds per decision.  A workgroup owns a row and the rows
run side by side, so the call lasts as long as its longest row: `us_per_decision` divides by the decisions of the row with the most,
`decisions_total` is there to see the work saved.  The decisions are counted by a float32 numpy restatement of the recursion, the batch
in lockstep; `rows_with_identical_labels` says how many rows it decoded as the device did.  The classic call is timed twice: the spread
of its two medians is the margin for `tdt_over_classic_us_per_decision`.  Everything is reported as measured."""
import sys
import numpy as np
import torch
from timing import emit, open_device, timed
from nntoolkitcore_amd import layers as NL

E = H = J = 512
V, T, BLANK, MAX_SYMBOLS = 1024, 200, 0, 3
DURATIONS = (0, 1, 2, 3, 4)
BATCHES = (1, 16, 256)
WARMUP = 1


def model(rng):
    u = lambda sc, *s: rng.uniform(-sc, sc, s).astype(np.float32)
    G, D = 4 * H, len(DURATIONS)
    bias = u(0.1, V)
    bias[1:] -= np.float32(3.0)                      # about one label in four decisions
    return dict(embed=u(1.0, V, E), W=u(2.0 * E ** -0.5, E, G), U=u(2.0 * H ** -0.5, H, G), b_i=u(0.1, G), b_h=u(0.1, G),
                Wp=u(2.0 * H ** -0.5, H, J), bp=u(0.1, J), Wo=u(3.0 * J ** -0.5, J, V), bo=bias, Wd=u(3.0 * J ** -0.5, J, D), bd=u(0.1, D))


def restated(m, enc, durations):
    """the recursion in float32 numpy, the batch in lockstep; durations None: the classic rule (a blank moves one frame, a label none)
    -> (labels per row, decisions per row)"""
    B = enc.shape[0]
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    Wo, bo = (m["Wo"], m["bo"]) if durations is None else (np.concatenate([m["Wo"], m["Wd"]], 1), np.concatenate([m["bo"], m["bd"]]))
    dur = np.asarray(durations if durations is not None else (0, 1))
    pos = np.flatnonzero(dur > 0)
    h, c, g = np.zeros((B, H), np.float32), np.zeros((B, H), np.float32), np.zeros((B, J), np.float32)
    t, s, decisions = np.zeros(B, int), np.zeros(B, int), np.zeros(B, int)
    emitted = np.full(B, BLANK)
    labels = [[] for _ in range(B)]
    while True:
        r = np.flatnonzero(emitted >= 0)
        if r.size:
            z = (m["embed"][emitted[r]] @ m["W"] + m["b_i"]) + h[r] @ m["U"] + m["b_h"]
            c[r] = sig(z[:, H:2 * H]) * c[r] + sig(z[:, :H]) * np.tanh(z[:, 2 * H:3 * H])
            h[r] = sig(z[:, 3 * H:]) * np.tanh(c[r])
            g[r] = h[r] @ m["Wp"] + m["bp"]
        live = np.flatnonzero(t < T)
        if not live.size:
            return labels, decisions
        x = np.tanh(enc[live, t[live]] + g[live]) @ Wo + bo
        k = x[:, :V].argmax(1)
        if durations is None:
            d = (k == BLANK).astype(int)
        else:
            d = dur[np.where(k == BLANK, pos[x[:, V:][:, pos].argmax(1)], x[:, V:].argmax(1))]
        decisions[live] += 1
        emitted[:] = -1
        for b, kb, db in zip(live, k, d):
            if kb != BLANK:
                labels[b].append(int(kb)); emitted[b] = kb
            if kb == BLANK or db > 0:
                t[b] += db; s[b] = 0
            else:
                s[b] += 1
                if s[b] == MAX_SYMBOLS:
                    t[b] += 1; s[b] = 0


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
    out = {"tool": "rnnt_tdt_decode_time", "repeats": repeats, "warmup": WARMUP, "source_hash": L.nntk_build_source_hash().decode(),
           "model": {"E": E, "H": H, "J": J, "V": V, "T": T, "max_symbols_per_frame": MAX_SYMBOLS, "durations": list(DURATIONS)}, "batches": []}
    ML = MAX_SYMBOLS * T
    for B in BATCHES:
        enc_h = rng.uniform(-1.5, 1.5, (B, T, J)).astype(np.float32)
        enc = d(enc_h)
        row = {"batch": B}
        runs = {}
        for name, dec, durs in (("classic", classic, None), ("tdt", tdt, DURATIONS), ("classic_again", classic, None)):
            outs = dec._outputs(enc.device, B, ML)
            runs[name] = timed(lambda: dec._decode(None, enc, None, ML, outs), repeats, WARMUP)
            if name == "classic_again":
                continue
            labels, lengths = outs[0].cpu().numpy(), outs[-2].cpu().numpy()
            ref_labels, decisions = restated(m, enc_h, durs)
            same = sum(labels[b, :lengths[b]].tolist() == ref_labels[b] for b in range(B))
            row[name] = {"ms": runs[name].median, "ms_min_max": [runs[name].min, runs[name].max], "decisions_longest_row": int(decisions.max()),
                         "decisions_total": int(decisions.sum()), "labels_total": int(lengths.sum()), "rows_with_identical_labels": int(same),
                         "us_per_decision": 1e3 * runs[name].median / int(decisions.max())}
        a, b = runs["classic"].median, runs["classic_again"].median
        row["classic_again_ms"] = b
        row["classic_spread"] = abs(a - b) / (0.5 * (a + b))
        row["tdt_over_classic_us_per_decision"] = row["tdt"]["us_per_decision"] / row["classic"]["us_per_decision"]
        row["rows_per_workgroup"] = int(L.nntk_shim_rnnt_tdt_dec_rows_per_group(B, H, J, V, len(DURATIONS)))
        out["batches"].append(row)
    emit(out, "rnnt_tdt_decode_time")


if __name__ == "__main__":
    main()
