"""RNN-Transducer beam search as include/nntoolkitcore_hip.h "RNN-Transducer: beam search" states it, on the library's weight blocks,
in numpy: the float64 reference the device tests compare with, and a float32 restatement of the same search (sequential sums, numpy's
float32 exp / tanh / log, float32 scores) that serves only as the yardstick of what float32 arithmetic costs on the same inputs.
A helper, no test."""
import numpy as np

from rnnt_decode_reference import _act, _matvec, _sum, split_dense, split_lstm


def lattice_logits(embed, lstm_block, pred_proj, out, enc_row, labels, blank=0, activation="tanh"):
    """float64: the unnormalised scores [T][len(labels) + 1][V] of one row's lattice for one label sequence, as the training path builds
    them: the prediction network on blank, y_1 .. y_U, the joiner against every frame, the vocabulary Dense"""
    f = lambda a: np.asarray(a, dtype=np.float64)
    embed, enc_row = f(embed), f(enc_row)
    V, E = embed.shape
    J = enc_row.shape[1]
    H = int(round((-(E + 2) + ((E + 2) ** 2 + np.asarray(lstm_block).size) ** 0.5) / 2))
    W, U, b_i, b_h = (f(a) for a in split_lstm(lstm_block, E, H))
    Wo, bo = (f(a) for a in split_dense(out, J, V))
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    h, c, gs = np.zeros(H), np.zeros(H), []
    for k in [blank] + list(labels):
        z = embed[k] @ W + b_i + h @ U + b_h
        c = sig(z[H:2 * H]) * c + sig(z[:H]) * np.tanh(z[2 * H:3 * H])
        h = sig(z[3 * H:]) * np.tanh(c)
        gs.append(h if pred_proj is None else h @ f(split_dense(pred_proj, H, J)[0]) + f(split_dense(pred_proj, H, J)[1]))
    return _act(activation, enc_row[:, None, :] + np.array(gs)[None, :, :]) @ Wo + bo


def beam_decode(embed, lstm_block, pred_proj, out, enc, n_frames=None, blank=0, activation="tanh", max_symbols_per_frame=10,
                beam_width=8, nbest=1, max_labels=None, dtype=np.float64):
    """-> dict(labels: per row the label lists of the first nbest final hypotheses; scores: per row their scores; final: per row every
    final hypothesis as (labels, score); cut_gap [B]: the smallest difference, over every top-W cut of C and of B, between the last kept
    and the best dropped score (inf where nothing was dropped); order_gap [B]: the smallest difference between consecutive scores among
    the first nbest + 1 final hypotheses (inf for fewer than two); merges [B]: candidates that met their label sequence in B; cuts [B]:
    cuts that dropped something; at_max [B]: hypotheses that could not be extended because they held max_labels labels; max_b [B]: the
    largest number of entries B held at the end of any frame, before its cut).
    dtype float32: the sequential restatement."""
    seq = dtype == np.float32
    f = lambda a: np.asarray(a, dtype=dtype)
    embed, enc = f(embed), f(enc)
    V, E = embed.shape
    B, T, J = enc.shape
    H = int(round((-(E + 2) + ((E + 2) ** 2 + np.asarray(lstm_block).size) ** 0.5) / 2))
    W, U, b_i, b_h = (f(a) for a in split_lstm(lstm_block, E, H))
    Wp, bp = (f(a) for a in split_dense(pred_proj, H, J)) if pred_proj is not None else (None, None)
    Wo, bo = (f(a) for a in split_dense(out, J, V))
    one = dtype(1)
    sig = lambda x: one / (one + np.exp(-x))
    S, BW = max_symbols_per_frame, beam_width
    cap = max(1, S * T) if max_labels is None else max_labels
    ninf = dtype(-np.inf)

    def step(k, h, c):
        z = ((_matvec(embed[k], W, seq) + b_i) + _matvec(h, U, seq)) + b_h
        i, fg, g, o = sig(z[:H]), sig(z[H:2 * H]), np.tanh(z[2 * H:3 * H]), sig(z[3 * H:])
        c = fg * c + i * g
        h = o * np.tanh(c)
        return h, c, (_matvec(h, Wp, seq) + bp if Wp is not None else h)

    def logp(e, g):
        logits = _matvec(_act(activation, e + g), Wo, seq) + bo
        m = logits.max()
        return (logits - m) - np.log(_sum(np.exp(logits - m), seq))

    res = dict(labels=[], scores=[], final=[], cut_gap=np.full(B, np.inf), order_gap=np.full(B, np.inf), merges=np.zeros(B, int),
               cuts=np.zeros(B, int), at_max=np.zeros(B, int), max_b=np.zeros(B, int))

    def cut(b, scores):
        """scores: descending; the gap between the last kept and the best dropped"""
        if len(scores) > BW:
            res["cuts"][b] += 1
            res["cut_gap"][b] = min(res["cut_gap"][b], float(scores[BW - 1]) - float(scores[BW]))

    for b in range(B):
        n = T if n_frames is None else int(n_frames[b])
        A = [((), dtype(0)) + step(blank, np.zeros(H, dtype), np.zeros(H, dtype))]          # (labels, score, h, c, g)
        for t in range(n):
            Bl, where = [], {}
            C = A
            for depth in range(S + 1):
                lps = [logp(enc[b, t], hyp[4]) for hyp in C]
                for hyp, lp in zip(C, lps):
                    s = hyp[1] + lp[blank]
                    if s == ninf:
                        continue
                    if hyp[0] in where:
                        e = Bl[where[hyp[0]]]
                        e[1] = np.logaddexp(e[1], s)
                        res["merges"][b] += 1
                    else:
                        where[hyp[0]] = len(Bl)
                        Bl.append([hyp[0], s, hyp[2], hyp[3], hyp[4]])
                if depth == S:
                    break
                cells = []                                                                 # (score, i * V + v), ascending in i * V + v
                for i, (hyp, lp) in enumerate(zip(C, lps)):
                    if len(hyp[0]) >= cap:
                        res["at_max"][b] += 1
                        continue
                    if not hyp[1] > ninf:
                        continue
                    cells += [(hyp[1] + lp[v], i * V + v) for v in range(V) if v != blank]
                order = np.argsort(-np.array([c[0] for c in cells], dtype=dtype), kind="stable") if cells else []
                cut(b, [cells[j][0] for j in order])
                nxt = []
                for j in order[:BW]:
                    s, idx = cells[j]
                    src, v = C[idx // V], idx % V
                    nxt.append((src[0] + (v,), s) + step(v, src[2], src[3]))
                C = nxt
                if not C:
                    break
            res["max_b"][b] = max(res["max_b"][b], len(Bl))
            order = np.argsort(-np.array([e[1] for e in Bl], dtype=dtype), kind="stable") if Bl else []
            cut(b, [Bl[j][1] for j in order])
            A = [tuple(Bl[j]) for j in order[:BW]]
        res["final"].append([(list(h[0]), h[1]) for h in A])
        res["labels"].append([list(h[0]) for h in A[:nbest]])
        res["scores"].append([h[1] for h in A[:nbest]])
        top = [float(h[1]) for h in A[:nbest + 1]]
        if len(top) > 1:
            res["order_gap"][b] = min(x - y for x, y in zip(top, top[1:]))
    return res
