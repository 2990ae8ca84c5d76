"""RNN-Transducer beam search fused with an n-gram language model as include/nntoolkitcore_hip.h "RNN-Transducer: beam search",
Language-model fusion, states it, in numpy: the search of rnnt_beam_reference.beam_decode in which every hypothesis also carries a state
of the backoff automaton, a label cell adds lnF(state, label), and the report adds the end-of-sentence term.  float64 is the reference
the device tests compare with; float32 is the sequential restatement (rnnt_decode_reference's sums, float32 scores, the model's terms
rounded to float32 as they are added) that serves only as the yardstick of what float32 arithmetic costs.  A helper, no test."""
import numpy as np

from rnnt_beam_reference import lattice_logits  # noqa: F401  (the tests take it from here)
from rnnt_decode_reference import _act, _matvec, _sum, split_dense, split_lstm


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


def beam_decode(embed, lstm_block, pred_proj, out, enc, lm, n_frames=None, blank=0, activation="tanh", max_symbols_per_frame=10,
                beam_width=8, nbest=1, max_labels=None, dtype=np.float64):
    """rnnt_beam_reference.beam_decode with the model ``lm`` (an Lm).  The same dict: labels / scores are the report (the final A with the
    end-of-sentence term, -inf dropped, ordered descending, ties to the lower rank in A; the first nbest), ``final`` every reported
    hypothesis as (labels, score), ``carried`` the final A itself as (labels, score, lm state); cut_gap, order_gap (over the report),
    merges, cuts, at_max, max_b as there.  dtype float32: the sequential restatement."""
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

    res = dict(labels=[], scores=[], final=[], carried=[], cut_gap=np.full(B, np.inf), order_gap=np.full(B, np.inf),
               merges=np.zeros(B, int), cuts=np.zeros(B, int), at_max=np.zeros(B, int), max_b=np.zeros(B, int))

    def cut(b, scores):
        if len(scores) > BW:
            res["cuts"][b] += 1
            res["cut_gap"][b] = min(res["cut_gap"][b], float(scores[BW - 1]) - float(scores[BW]))

    for b in range(B):
        n = T if n_frames is None else int(n_frames[b])
        A = [((), dtype(0)) + step(blank, np.zeros(H, dtype), np.zeros(H, dtype)) + (lm.start,)]      # (labels, score, h, c, g, q)
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
                        assert e[5] == hyp[5]                                               # the automaton is deterministic
                        e[1] = np.logaddexp(e[1], s)
                        res["merges"][b] += 1
                    else:
                        where[hyp[0]] = len(Bl)
                        Bl.append([hyp[0], s, hyp[2], hyp[3], hyp[4], hyp[5]])
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
                    nxt.append((src[0] + (v,), s) + step(v, src[2], src[3]) + (nx,))
                C = nxt
                if not C:
                    break
            res["max_b"][b] = max(res["max_b"][b], len(Bl))
            order = np.argsort(-np.array([e[1] for e in Bl], dtype=dtype), kind="stable") if Bl else []
            cut(b, [Bl[j][1] for j in order])
            A = [tuple(Bl[j]) for j in order[:BW]]
        rep = [(list(h[0]), h[1] + dtype(lm.final_ln[h[5]])) for h in A]
        rep = [r for r in rep if r[1] > ninf]
        rep = [rep[j] for j in np.argsort(-np.array([r[1] for r in rep], dtype=dtype), kind="stable")] if rep else []
        res["carried"].append([(list(h[0]), h[1], h[5]) for h in A])
        res["final"].append(rep)
        res["labels"].append([r[0] for r in rep[:nbest]])
        res["scores"].append([r[1] for r in rep[:nbest]])
        top = [float(r[1]) for r in rep[:nbest + 1]]
        if len(top) > 1:
            res["order_gap"][b] = min(x - y for x, y in zip(top, top[1:]))
    return res
