"""RNN-Transducer beam search as include/nntoolkitcore_hip.h "RNN-Transducer: beam search" states it, on the library's weight blocks,
in numpy, once: with or without an n-gram language model ("Language-model fusion": every hypothesis carries a state of the backoff
automaton, a label cell adds lnF(state, label), the report adds the end-of-sentence term) and always with the detail ("Label
timestamps": every hypothesis carries the frame and the acoustic log-probability of each of its labels, an entry of B remembers its
largest single contribution, ``lead``, and reports that contributor's arrays; the report may be ordered by score / (length + 1)).
float64 is the reference the device tests compare with; float32 is a restatement of the same search (sequential sums, numpy's float32
exp / tanh / log, float32 scores, the model's terms rounded to float32 as they are added) that serves only as the yardstick of what
float32 arithmetic costs on the same inputs.  A helper, no test."""
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


class Lm:
    """The automaton of NgramLm.from_arrays' keyword arguments ``t`` with alpha and beta: float64 terms from the table's float32 inputs,
    exactly what csrc/host/ngram_lm.c keeps (alpha a power of two makes alpha * v + beta one rounding).  Counts what a search met:
    ``backoffs`` (walks that took at least one), ``unk`` (walks that ended without an arc in state 0), ``dead`` (terms of -inf)."""

    def __init__(self, t, alpha=1.0, beta=0.0):
        self.t, self.a, self.b = t, float(np.float32(alpha)), float(np.float32(beta))
        f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
        sc = lambda v, beta: np.full(len(v), beta) if self.a == 0.0 else self.a * v + beta
        with np.errstate(invalid="ignore"):
            self.arc_ln = sc(f32(t["arc_logp"]), self.b)
            self.backoff_ln = sc(f32(t["backoff_logw"]), 0.0)
            self.final_ln = np.zeros(len(t["backoff_state"])) if t.get("final_logp") is None else sc(f32(t["final_logp"]), 0.0)
            self.unk_ln = float(sc(f32([t["unk_logp"]]), self.b)[0])
        self.lab = np.asarray(t["arc_label"], np.int64)
        self.start = int(t.get("start_state", 0))
        self.backoffs = self.unk = self.dead = 0

    def walk(self, s, v):
        """-> lnF(s, v) = ((0 + b_0) + b_1 ...) + g in float64, next(s, v)"""
        t, acc, took = self.t, 0.0, False
        while True:
            lo, hi = t["arc_begin"][s], t["arc_begin"][s + 1]
            q = lo + int(np.searchsorted(self.lab[lo:hi], v))
            if q < hi and self.lab[q] == v:
                ln, nx = acc + self.arc_ln[q], int(t["arc_next"][q])
                break
            if s == 0:
                ln, nx = acc + self.unk_ln, 0
                self.unk += 1
                break
            acc += self.backoff_ln[s]
            s = int(t["backoff_state"][s])
            took = True
        self.backoffs += took
        self.dead += ln == -np.inf
        return float(ln), nx

    def score(self, labels, with_final=True):
        """the sum nntk_ngram_lm_score forms"""
        s, total = self.start, 0.0
        for v in labels:
            ln, s = self.walk(s, int(v))
            total += ln
        return total + (float(self.final_ln[s]) if with_final else 0.0)


def beam_decode(embed, lstm_block, pred_proj, out, enc, n_frames=None, blank=0, activation="tanh", max_symbols_per_frame=10,
                beam_width=8, nbest=1, max_labels=None, lm=None, length_norm=False, t0=None, dtype=np.float64):
    """-> dict.  The report is the final A in order; with lm (an Lm): + ln E, the -inf entries dropped, ordered descending; with
    length_norm: ordered by key = score / (length + 1), ties to the lower rank in A.  Its first nbest per row as labels, scores, frames,
    lps; ``final``: every reported hypothesis as (labels, score, frames, lps) in report order; ``carried``: the final A itself as
    (labels, score, lm state); ``plain_labels``: the first nbest of the report without length_norm.
    cut_gap [B]: the smallest difference, over every top-W cut of C and of B, between the last kept and the best dropped score (inf
    where nothing was dropped); order_gap [B]: the smallest difference between consecutive scores among the first nbest + 1 of the plain
    report (inf for fewer than two); merges [B]: candidates that met their label sequence in B; cuts [B]: cuts that dropped something;
    at_max [B]: hypotheses that could not be extended because they held max_labels labels; max_b [B]: the largest number of entries B
    held at the end of any frame, before its cut; lead_gap [B]: the smallest |cand.score - lead| over the merges whose two sides'
    frames differ (inf: none); lead_gap_nonzero [B]: the same over those that are no exact tie; lead_ties [B]: the exact ties among
    them; lead_switches [B]: the merges that changed the arrays; key_gap [B]: the smallest gap between consecutive keys among the first
    nbest + 1 of the ranked report (inf without length_norm or for fewer than two); reordered [B]: the ranked nbest differs from the
    plain one.  t0: per row, the frames its stream consumed before (None: 0).  dtype float32: the sequential restatement."""
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

    inf = lambda: np.full(B, np.inf)
    zero = lambda: np.zeros(B, int)
    res = dict(labels=[], scores=[], frames=[], lps=[], final=[], carried=[], plain_labels=[], cut_gap=inf(), order_gap=inf(), lead_gap=inf(),
               lead_gap_nonzero=inf(), key_gap=inf(), merges=zero(), cuts=zero(), at_max=zero(), max_b=zero(), lead_switches=zero(),
               lead_ties=zero(), reordered=np.zeros(B, bool))

    def cut(b, scores):
        if len(scores) > BW:
            res["cuts"][b] += 1
            res["cut_gap"][b] = min(res["cut_gap"][b], float(scores[BW - 1]) - float(scores[BW]))

    for b in range(B):
        n = T if n_frames is None else int(n_frames[b])
        base = 0 if t0 is None else int(t0[b])
        # a hypothesis: [labels, score, h, c, g, q, frames, lps]; an entry of B: the same with lead behind
        A = [[(), dtype(0)] + list(step(blank, np.zeros(H, dtype), np.zeros(H, dtype))) + [lm.start if lm is not None else 0, (), ()]]
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
                        assert e[5] == hyp[5]
                        res["merges"][b] += 1
                        if e[6] != hyp[6]:
                            gap = abs(float(s) - float(e[8]))
                            res["lead_gap"][b] = min(res["lead_gap"][b], gap)
                            if gap == 0.0:
                                res["lead_ties"][b] += 1
                            else:
                                res["lead_gap_nonzero"][b] = min(res["lead_gap_nonzero"][b], gap)
                        if s > e[8]:
                            res["lead_switches"][b] += e[6] != hyp[6]
                            e[8], e[6], e[7] = s, hyp[6], hyp[7]
                        e[1] = np.logaddexp(e[1], s)
                    else:
                        where[hyp[0]] = len(Bl)
                        Bl.append([hyp[0], s, hyp[2], hyp[3], hyp[4], hyp[5], hyp[6], hyp[7], s])
                if depth == S:
                    break
                cells = []                                                                  # (score, i * V + v, next state)
                for i, (hyp, lp) in enumerate(zip(C, lps)):
                    if len(hyp[0]) >= cap:
                        res["at_max"][b] += 1
                        continue
                    if not hyp[1] > ninf:
                        continue
                    for v in range(V):
                        if v == blank:
                            continue
                        if lm is None:
                            cells.append((hyp[1] + lp[v], i * V + v, 0))
                        else:
                            ln, nx = lm.walk(hyp[5], v)
                            s = (hyp[1] + lp[v]) + dtype(ln)
                            if s > ninf:
                                cells.append((s, i * V + v, nx))
                order = np.argsort(-np.array([c[0] for c in cells], dtype=dtype), kind="stable") if cells else []
                cut(b, [cells[j][0] for j in order])
                nxt = []
                for j in order[:BW]:
                    s, idx, nx = cells[j]
                    src, v = C[idx // V], idx % V
                    nxt.append([src[0] + (v,), s] + list(step(v, src[2], src[3])) + [nx, src[6] + (base + t,), src[7] + (lps[idx // V][v],)])
                C = nxt
                if not C:
                    break
            res["max_b"][b] = max(res["max_b"][b], len(Bl))
            order = np.argsort(-np.array([e[1] for e in Bl], dtype=dtype), kind="stable") if Bl else []
            cut(b, [Bl[j][1] for j in order])
            A = [Bl[j][:8] for j in order[:BW]]
        res["carried"].append([(list(h[0]), h[1], h[5]) for h in A])
        rep = [(list(h[0]), h[1], list(h[6]), [float(x) for x in h[7]]) for h in A]         # without a model: A in order, nothing added
        if lm is not None:
            rep = [(r[0], r[1] + dtype(lm.final_ln[h[5]])) + r[2:] for r, h in zip(rep, A)]
            rep = [r for r in rep if r[1] > ninf]
            rep = [rep[j] for j in np.argsort(-np.array([r[1] for r in rep], dtype=dtype), kind="stable")] if rep else []
        top = [float(r[1]) for r in rep[:nbest + 1]]
        if len(top) > 1:
            res["order_gap"][b] = min(x - y for x, y in zip(top, top[1:]))
        res["plain_labels"].append([r[0] for r in rep[:nbest]])
        if length_norm and rep:
            keys = np.array([r[1] / dtype(len(r[0]) + 1) for r in rep], dtype=dtype)
            rank = np.argsort(-keys, kind="stable")
            rep = [rep[j] for j in rank]
            top = [float(keys[j]) for j in rank[:nbest + 1]]
            if len(top) > 1:
                res["key_gap"][b] = min(x - y for x, y in zip(top, top[1:]))
        res["final"].append(rep)
        for key, at in (("labels", 0), ("scores", 1), ("frames", 2), ("lps", 3)):
            res[key].append([r[at] for r in rep[:nbest]])
        res["reordered"][b] = res["labels"][b] != res["plain_labels"][b]
    return res
