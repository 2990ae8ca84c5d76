"""Token-and-duration beam search as include/nntoolkitcore_hip.h "RNN-Transducer: token-and-duration beam search" states it, in numpy:
the float64 reference the device tests compare with, the float32 restatement of the same search (sequential sums, float32 scores) that
serves only as the yardstick of what float32 arithmetic costs, and tdt_path_mass, a forward recursion over (t, u) that knows nothing of
the search and checks it.  A helper, no test."""
import numpy as np

from rnnt_decode_reference import _act, _matvec, _sum
from rnnt_tdt_decode_reference import _network


def _log_softmax(v, seq=False):
    return (v - v.max()) - np.log(_sum(np.exp(v - v.max()), seq))


def tdt_beam_decode(embed, lstm_block, pred_proj, out, enc, durations, n_frames=None, blank=0, activation="tanh", max_symbols_per_frame=10,
                    beam_width=8, nbest=1, max_labels=None, dtype=np.float64):
    """-> dict(labels, scores: per row the first nbest of the W best of bucket[n]; final: all of them as (labels, score); cut_gap [B]: the
    smallest gap at any top-W cut of a bucket or of the cells; order_gap [B]: the smallest gap among the first nbest + 1 results; counts
    [B]: merges, cuts, at_max (hypotheses that could not be extended), clamped (moves beyond n), skipped_frames; skipped: those frames)"""
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
    res = dict(labels=[], scores=[], final=[], skipped=[], cut_gap=np.full(B, np.inf), order_gap=np.full(B, np.inf),
               **{k: np.zeros(B, int) for k in ("merges", "cuts", "at_max", "clamped", "skipped_frames")})
    for b in range(B):
        n = T if n_frames is None else int(n_frames[b])
        buckets = [[] for _ in range(n + 1)]                     # entries [y, score, (h, c, g)] in insertion order
        def put(t, d, y, s, state):
            res["clamped"][b] += t + d > n
            if s == ninf:
                return
            for e in buckets[min(t + d, n)]:
                if e[0] == y:
                    e[1] = np.logaddexp(e[1], s)
                    res["merges"][b] += 1
                    return
            buckets[min(t + d, n)].append([y, s, state])
        def best(scores):
            order = np.argsort(-np.asarray(scores, dtype=dtype), kind="stable")
            if len(order) > BW:
                res["cuts"][b] += 1
                res["cut_gap"][b] = min(res["cut_gap"][b], float(scores[order[BW - 1]]) - float(scores[order[BW]]))
            return order[:BW]
        buckets[0].append([(), dtype(0), step(blank, np.zeros(H, dtype), np.zeros(H, dtype))])
        skipped = []
        for t in range(n):
            if not buckets[t]:
                skipped.append(t)
                continue
            C = [buckets[t][j] for j in best([e[1] for e in buckets[t]])]
            for depth in range(S + 1):
                heads = []
                for y, s, st in C:
                    x = _matvec(_act(activation, enc[b, t] + st[2]), Wo, seq) + bo
                    heads.append((_log_softmax(x[:V], seq), _log_softmax(x[V:], seq)))
                for (y, s, st), (lt, ld) in zip(C, heads):
                    for k in np.flatnonzero(pos):
                        put(t, dur[k], y, s + (lt[blank] + ld[k]), st)
                ok = pos if depth == S else np.ones(D, bool)
                scores, idx = [], []
                for i, ((y, s, st), (lt, ld)) in enumerate(zip(C, heads)):
                    if len(y) >= cap:
                        res["at_max"][b] += 1
                        continue
                    c = s + (lt[:, None] + ld[None, :])          # [V][D]
                    keep = (c > ninf) & ok[None, :] & (np.arange(V) != blank)[:, None]
                    scores.append(c[keep])
                    idx.append(((i * V + np.arange(V))[:, None] * D + np.arange(D)[None, :])[keep])
                if not scores:
                    break
                scores, idx = np.concatenate(scores), np.concatenate(idx)
                nxt, stepped = [], {}
                for j in best(scores):
                    i, v, k = int(idx[j]) // D // V, int(idx[j]) // D % V, int(idx[j]) % D
                    if (i, v) not in stepped:
                        stepped[(i, v)] = step(v, C[i][2][0], C[i][2][1])
                    if dur[k] == 0:
                        nxt.append([C[i][0] + (v,), scores[j], stepped[(i, v)]])
                    else:
                        put(t, dur[k], C[i][0] + (v,), scores[j], stepped[(i, v)])
                C = nxt
                if depth == S or not C:
                    break
        last = buckets[n]
        rep = [(list(last[j][0]), last[j][1]) for j in best([e[1] for e in last])]
        top = [float(r[1]) for r in rep[:nbest + 1]]
        if len(top) > 1:
            res["order_gap"][b] = min(x - y for x, y in zip(top, top[1:]))
        for key, v in (("final", rep), ("labels", [r[0] for r in rep[:nbest]]), ("scores", [r[1] for r in rep[:nbest]]), ("skipped", skipped)):
            res[key].append(v)
        res["skipped_frames"][b] = len(skipped)
    return res


def tdt_path_mass(logits, y, durations, blank=0):
    """float64: ln of the mass of the paths that emit y on logits [n][len(y) + 1][V + D], a move from t < n landing on min(t + d, n), a
    blank never taking duration 0: alpha(n, U) of a forward recursion over (t, u)"""
    x = np.asarray(logits, np.float64)
    n, U, D = x.shape[0], len(y), len(durations)
    V = x.shape[2] - D
    alpha = np.full((n + 1, U + 1), -np.inf)
    alpha[0, 0] = 0.0
    for t in range(n):
        for u in range(U + 1):                                   # a label with duration 0 feeds (t, u + 1): u ascending
            if alpha[t, u] == -np.inf:
                continue
            lt, ld = _log_softmax(x[t, u, :V]), _log_softmax(x[t, u, V:])
            for k, d in enumerate(durations):
                f = min(t + d, n)
                if d > 0:
                    alpha[f, u] = np.logaddexp(alpha[f, u], alpha[t, u] + (lt[blank] + ld[k]))
                if u < U:
                    alpha[f, u + 1] = np.logaddexp(alpha[f, u + 1], alpha[t, u] + (lt[y[u]] + ld[k]))
    return float(alpha[n, U])
