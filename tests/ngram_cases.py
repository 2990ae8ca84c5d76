"""The n-gram tables that the tests of the fused searches share (CTC: test_gpu_ctc_beam_lm.py, ctc_long_cases.py,
ctc_beam_detail_reference.py; transducer: rnnt_beam_lm_cases.py) and ``Walk``, the float64 restatement of a table's F, next state and
end-of-sentence factor.  The tables' float32 inputs are taken as they are; everything else is float64."""
import numpy as np


def table(n_classes, blank, arcs, rng, unk, final):
    """arcs: {context tuple: sorted labels}, closed under dropping the oldest label -> NgramLm.from_arrays' keyword arguments"""
    ctx = sorted(arcs, key=lambda c: (len(c), c))
    sid = {c: i for i, c in enumerate(ctx)}
    depth = max(len(c) for c in ctx)

    def state_of(hist):
        hist = hist[len(hist) - depth:] if len(hist) > depth else hist
        while hist not in sid:
            hist = hist[1:]
        return sid[hist]
    t = dict(n_classes=n_classes, blank=blank, arc_begin=[0], arc_label=[], arc_logp=[], arc_next=[], backoff_state=[], backoff_logw=[],
             start_state=0, unk_logp=unk)
    for c in ctx:
        for a in arcs[c]:
            t["arc_label"].append(a); t["arc_logp"].append(float(np.log(rng.uniform(0.02, 0.9)))); t["arc_next"].append(state_of(c + (a,)))
        t["arc_begin"].append(len(t["arc_label"]))
        t["backoff_state"].append(-1 if not c else state_of(c[1:]))
        t["backoff_logw"].append(0.0 if not c else float(np.log(rng.uniform(0.2, 0.9))))
    t["final_logp"] = np.log(rng.uniform(0.05, 0.9, len(ctx))).tolist() if final else None
    return t


def dense_bigram(seed, n_classes, blank, final=False):
    rng = np.random.default_rng(seed)
    labels = [c for c in range(n_classes) if c != blank]
    return table(n_classes, blank, {c: labels for c in [()] + [(a,) for a in labels]}, rng, float(np.log(0.01)), final)


def sparse_trigram(seed, n_classes, blank, n_bi, n_tri, arcs0, unk=float(np.log(0.01)), final=False):
    """state 0 with arcs0 arcs (those to the n_bi one-label contexts among them), up to n_tri two-label contexts (x, a) that the state
    (x) reaches, each backing off to (a) where that is a state, else to state 0"""
    rng = np.random.default_rng(seed)
    labels = [c for c in range(n_classes) if c != blank]
    uni = sorted(rng.choice(labels, n_bi, replace=False).tolist())
    pick = lambda k, must=(): sorted(set(must) | set(rng.choice(labels, k, replace=False).tolist()))
    arcs = {(): pick(arcs0, uni)}
    for x in uni:
        arcs[(x,)] = pick(int(rng.integers(2, max(3, min(len(labels), 40) // 3))))
    pairs = [(x, a) for x in uni for a in arcs[(x,)]]
    for q in sorted(rng.choice(len(pairs), min(n_tri, len(pairs)), replace=False).tolist()):
        arcs[pairs[q]] = pick(int(rng.integers(1, max(2, min(len(labels), 40) // 3))))
    return table(n_classes, blank, arcs, rng, unk, final)


class Walk:
    """float64 F, next state, backoffs taken and the unknown-label flag of (state, class), cached; counts what the search met"""

    def __init__(self, t, alpha, beta):
        self.t, self.a, self.b, self.cache = t, float(np.float32(alpha)), float(np.float32(beta)), {}
        self.depths, self.unk, self.dead = set(), False, 0
        f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
        self.logp, self.bow, self.unk_logp = f32(t["arc_logp"]), f32(t["backoff_logw"]), float(np.float32(t["unk_logp"]))
        self.fin = None if t["final_logp"] is None else f32(t["final_logp"])
        self.lab = np.asarray(t["arc_label"], np.int64)

    def _ln(self, v, beta):
        return beta if self.a == 0.0 else self.a * v + beta

    def __call__(self, s, c):
        key = (s, c)
        if key not in self.cache:
            t, ln, d, st = self.t, 0.0, 0, s
            while True:
                lo, hi = t["arc_begin"][st], t["arc_begin"][st + 1]
                q = lo + int(np.searchsorted(self.lab[lo:hi], c))
                if q < hi and self.lab[q] == c:
                    self.cache[key] = (float(np.exp(ln + self._ln(self.logp[q], self.b))), t["arc_next"][q], d, False)
                    break
                if st == 0:
                    self.cache[key] = (float(np.exp(ln + self._ln(self.unk_logp, self.b))), 0, d, True)
                    break
                ln += self._ln(self.bow[st], 0.0)
                st = t["backoff_state"][st]
                d += 1
        f, nx, d, u = self.cache[key]
        self.depths.add(d)
        self.unk |= u
        self.dead += f == 0.0
        return f, nx

    def final(self, s):
        return 1.0 if self.fin is None else float(np.exp(self._ln(self.fin[s], 0.0)))
