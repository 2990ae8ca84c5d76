"""Token-and-duration beam search with its options as include/nntoolkitcore_hip.h states them under "RNN-Transducer: token-and-duration
beam search" (language-model fusion, label frames, durations and confidences, length normalisation), in numpy: the float64 reference the
device tests compare with, and the float32 restatement of the same search (sequential sums, float32 scores, the model's terms rounded
to float32 as they are added) that serves only as the yardstick of what float32 arithmetic costs.  The network, the heads and the
n-gram walk are those of the existing references.  A helper, no test."""
import numpy as np

from rnnt_decode_reference import _act, _matvec
from rnnt_tdt_beam_reference import _log_softmax, _network

COUNTS = ("merges", "lead_switches", "twins", "twins_clamped", "clamped_labels", "backoffs", "dead_arcs", "cuts")


def tdt_beam_decode(embed, lstm_block, pred_proj, out, enc, durations, n_frames=None, blank=0, activation="tanh", max_symbols_per_frame=10,
                    beam_width=8, nbest=1, max_labels=None, lm=None, length_norm=False, dtype=np.float64):
    """lm: an rnnt_beam_reference.Lm or None.  -> dict(labels, scores, frames, durs, lps: per row the first nbest of the report; final:
    the whole report as (labels, score, frames, durs, lps); per row the COUNTS -- merges, lead_switches (merges that took the candidate's
    arrays), twins (selected cells sharing (i, v) with an earlier one), twins_clamped (those where both land in bucket[n]),
    clamped_labels (label moves beyond n), backoffs (walks that took one), dead_arcs (terms of -inf), cuts -- and the gaps: cut_gap (the
    smallest at any top-W cut), order_gap (the smallest among the first nbest + 1 of the report, in the key it is ranked by), lead_gap
    (the smallest |cand.score - lead| over the merges whose two sides' arrays differ))"""
    seq = dtype == np.float32
    dur = [int(d) for d in durations]
    D, S, BW = len(dur), max_symbols_per_frame, beam_width
    enc = np.asarray(enc, dtype=dtype)
    B, T, J = enc.shape
    V = np.asarray(embed).shape[0]
    step, H, Wo, bo = _network(embed, lstm_block, pred_proj, out, J, V + D, dtype)
    cap = max(1, S * T) if max_labels is None else max_labels
    pos = np.array([d > 0 for d in dur])
    ninf = dtype(-np.inf)
    res = dict(labels=[], scores=[], frames=[], durs=[], lps=[], final=[], cut_gap=np.full(B, np.inf), order_gap=np.full(B, np.inf),
               lead_gap=np.full(B, np.inf), **{k: np.zeros(B, int) for k in COUNTS})
    for b in range(B):
        n = T if n_frames is None else int(n_frames[b])
        met = (lm.backoffs, lm.dead) if lm is not None else (0, 0)
        buckets = [[] for _ in range(n + 1)]                     # entries [y, score, state, q, lead, (frames, durs, lps)], insertion order
        def put(t, d, y, s, state, q, arr):
            if s == ninf:
                return
            for e in buckets[min(t + d, n)]:
                if e[0] == y:
                    res["merges"][b] += 1
                    if e[5] != arr:
                        res["lead_gap"][b] = min(res["lead_gap"][b], abs(float(s) - float(e[4])))
                    if s > e[4]:
                        res["lead_switches"][b] += e[5] != arr
                        e[4], e[5] = s, arr
                    e[1] = np.logaddexp(e[1], s)
                    return
            buckets[min(t + d, n)].append([y, s, state, q, s, arr])
        def best(scores):
            order = np.argsort(-np.asarray(scores, dtype=dtype), kind="stable")
            if len(order) > BW:
                res["cuts"][b] += 1
                res["cut_gap"][b] = min(res["cut_gap"][b], float(scores[order[BW - 1]]) - float(scores[order[BW]]))
            return order[:BW]
        buckets[0].append([(), dtype(0), step(blank, np.zeros(H, dtype), np.zeros(H, dtype)), lm.start if lm is not None else 0, dtype(0),
                           ((), (), ())])
        for t in range(n):
            if not buckets[t]:
                continue
            C = [buckets[t][j] for j in best([e[1] for e in buckets[t]])]
            for depth in range(S + 1):
                heads = []
                for hyp in C:
                    x = _matvec(_act(activation, enc[b, t] + hyp[2][2]), Wo, seq) + bo
                    heads.append((_log_softmax(x[:V], seq), _log_softmax(x[V:], seq)))
                for hyp, (lt, ld) in zip(C, heads):
                    for k in np.flatnonzero(pos):
                        put(t, dur[k], hyp[0], hyp[1] + (lt[blank] + ld[k]), hyp[2], hyp[3], hyp[5])
                ok = pos if depth == S else np.ones(D, bool)
                scores, idx, nxq = [], [], {}
                for i, (hyp, (lt, ld)) in enumerate(zip(C, heads)):
                    if len(hyp[0]) >= cap:
                        continue
                    c = hyp[1] + (lt[:, None] + ld[None, :])     # [V][D]
                    if lm is not None:
                        walks = [(0.0, 0) if v == blank else lm.walk(hyp[3], v) for v in range(V)]
                        c = c + np.array([dtype(w[0]) for w in walks], dtype=dtype)[:, None]
                        nxq[i] = [w[1] for w in walks]
                    keep = (c > ninf) & ok[None, :] & (np.arange(V) != blank)[:, None]
                    scores.append(c[keep])
                    idx.append(((i * V + np.arange(V))[:, None] * D + np.arange(D)[None, :])[keep])
                if not scores:
                    break
                scores, idx = np.concatenate(scores), np.concatenate(idx)
                nxt, stepped = [], {}
                for j in best(scores):
                    i, v, k = int(idx[j]) // D // V, int(idx[j]) // D % V, int(idx[j]) % D
                    lands_n = dur[k] > 0 and t + dur[k] >= n
                    if (i, v) not in stepped:
                        stepped[(i, v)] = (step(v, C[i][2][0], C[i][2][1]), [])
                    else:
                        res["twins"][b] += 1
                        res["twins_clamped"][b] += lands_n and any(stepped[(i, v)][1])
                    stepped[(i, v)][1].append(lands_n)
                    fr, du, lp = C[i][5]
                    hyp = [C[i][0] + (v,), scores[j], stepped[(i, v)][0], nxq[i][v] if lm is not None else 0, scores[j],
                           (fr + (t,), du + (dur[k],), lp + (heads[i][0][v],))]
                    if dur[k] == 0:
                        nxt.append(hyp)
                    else:
                        res["clamped_labels"][b] += t + dur[k] > n
                        put(t, dur[k], hyp[0], hyp[1], hyp[2], hyp[3], hyp[5])
                C = nxt
                if depth == S or not C:
                    break
        last = buckets[n]
        rep = [last[j] for j in best([e[1] for e in last])]
        rep = [(list(e[0]), e[1] + dtype(lm.final_ln[e[3]]) if lm is not None else e[1]) + tuple(list(a) for a in e[5]) for e in rep]
        rep = [r for r in rep if r[1] > ninf]
        keys = np.array([r[1] / dtype(len(r[0]) + 1) if length_norm else r[1] for r in rep], dtype=dtype)
        rank = np.argsort(-keys, kind="stable")
        rep = [rep[j] for j in rank]
        top = [float(keys[j]) for j in rank[:nbest + 1]]
        if len(top) > 1:
            res["order_gap"][b] = min(x - y for x, y in zip(top, top[1:]))
        res["final"].append(rep)
        for at, key in enumerate(("labels", "scores", "frames", "durs", "lps")):
            res[key].append([r[at] for r in rep[:nbest]])
        if lm is not None:
            res["backoffs"][b], res["dead_arcs"][b] = lm.backoffs - met[0], lm.dead - met[1]
    return res
