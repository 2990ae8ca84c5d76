"""The cases of the fused transducer beam search tests (tests/test_gpu_rnnt_beam_lm.py) and their premises, which
tests/test_rnnt_beam_lm_host.py checks without a device: the acoustic models and frames of tests/rnnt_beam_cases.py, the n-gram tables of
tests/ngram_cases.py's recipe, the float64 reference (tests/rnnt_beam_reference.py with a model) and its float32 restatement.
A helper, no test.

alpha is a power of two in every case, so that alpha * v + beta is one rounding whatever the host compiler contracts, and beta is a
float32.  The table seeds were searched on the CPU so that the reference's smallest gap at a cut and in the reported order is at least
GAP and its float32 restatement returns the same labels; nothing about them comes from a device."""
import functools

import numpy as np

import rnnt_beam_reference as RB
from rnnt_beam_cases import case as acoustic_case, model as _model, search_kw  # noqa: F401  (search_kw: the host tests take it from here)
from ngram_cases import table as _table, dense_bigram, sparse_trigram

GAP = 1e-3

# name: (the acoustic case, the table, alpha, beta)
LM_SEEDS = {"awkward": 0, "awkward_w3": 1, "big_v": 5, "wide_identity": 1, "stream": 0, "decides": 0, "exhaustive3": 0, "exhaustive4": 0}
PARITY = ("awkward", "awkward_w3", "big_v", "wide_identity")
SPARSE = ("big_v", "wide_identity", "stream")       # a dense bigram takes no backoff and meets no unknown label, by construction
GAP_CASES = PARITY + ("stream", "decides", "zero_arc", "final_drop")
ALL_CASES = GAP_CASES + ("final_tie", "exhaustive3", "exhaustive4")


def table(name):
    """-> (NgramLm.from_arrays' keyword arguments, alpha, beta)"""
    seed = LM_SEEDS.get(name, 0)
    if name in ("awkward", "awkward_w3"):           # V 5, blank 0: every context holds every label
        return dense_bigram(seed, 5, 0, final=True), 0.5, 0.25
    if name == "big_v":                             # state 0 holds 1027 of the 1029 labels: more arcs than lanes, two unknown labels
        return sparse_trigram(seed, 1030, 1029, 24, 40, 1027, final=True), 0.5, -0.125
    if name == "wide_identity":
        return sparse_trigram(seed, 70, 69, 12, 30, 40, final=False), 1.0, 0.5
    if name == "stream":
        return sparse_trigram(seed, 6, 2, 3, 5, 4, final=True), 1.0, 0.25
    if name == "decides":                           # a model strong enough to change the best hypothesis
        return dense_bigram(seed, 5, 0, final=True), 2.0, 0.0
    if name == "zero_arc":                          # the awkward table with the arcs of row 0's best hypothesis at zero mass
        t, a, b = table("awkward")
        t = dict(t, arc_logp=list(t["arc_logp"]))
        for q in zero_arcs():
            t["arc_logp"][q] = -np.inf
        return t, a, b
    if name == "final_drop":                        # ... with no end of sentence from the state of row 0's best hypothesis
        t, a, b = table("awkward")
        t = dict(t, final_logp=list(t["final_logp"]))
        t["final_logp"][drop_state()] = -np.inf
        return t, a, b
    if name == "final_tie":                         # labels 1 and 3 alike in every context; the empty context ends a sentence best
        t = dense_bigram(0, 5, 0, final=True)
        lp = {1: 0.0, 2: np.log(0.125), 3: 0.0, 4: np.log(0.0625)}       # 1 and 3 keep their acoustic tie
        t["arc_logp"] = [float(np.float32(lp[v])) for v in t["arc_label"]]
        t["final_logp"] = [0.0] + [float(np.float32(np.log(1.0 / 64)))] * 4
        return t, 1.0, 0.0
    if name in ("exhaustive3", "exhaustive4"):
        arcs = {(): [0], (0,): [2], (0, 2): [0]} if name == "exhaustive3" else {(): [0, 2], (0,): [2], (2,): [3], (0, 2): [0, 3]}
        return _table(int(name[-1]), 1, arcs, np.random.default_rng(seed), float(np.log(0.01)), True), 0.5, 0.25
    raise KeyError(name)


def case(name):
    """dict(m, enc, n, act, ms, W, nbest, max_labels) of the acoustic search that the case's table is fused into"""
    if name in ("awkward", "awkward_w3", "big_v", "wide_identity", "stream", "tie"):
        return acoustic_case(name)
    if name in ("zero_arc", "final_drop"):
        return acoustic_case("awkward")
    if name == "decides":
        return acoustic_case("awkward_w3")
    if name == "final_tie":
        return acoustic_case("tie")
    if name in ("exhaustive3", "exhaustive4"):      # T 3, at most 2 labels, S 2: 1 + (V - 1) + (V - 1)^2 sequences, all inside W
        V = int(name[-1])
        m = _model(7 + V, V, 7, 13, 22, True, blank=1)
        return dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, (2, 3, 22)).astype(np.float32), n=[3, 2], act="tanh", ms=2, W=16, nbest=16,
                    max_labels=2)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (float64 result, float32 restatement, the float64 run's Lm with its counts)"""
    c = case(name)
    m = c["m"]
    t, alpha, beta = table(name)
    lm64, lm32 = RB.Lm(t, alpha, beta), RB.Lm(t, alpha, beta)
    r64 = RB.beam_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], lm=lm64, **search_kw(c))
    r32 = RB.beam_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], lm=lm32, dtype=np.float32, **search_kw(c))
    return r64, r32, lm64


@functools.lru_cache(maxsize=None)
def acoustic_reference(name):
    c = case(name)
    m = c["m"]
    return RB.beam_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], **search_kw(c))


def _state_after(t, labels):
    lm = RB.Lm(t)
    s = lm.start
    for v in labels:
        s = lm.walk(s, v)[1]
    return s


@functools.lru_cache(maxsize=None)
def zero_arcs():
    """the arcs (indices) that row 0's best hypothesis of the awkward case takes, after its first label"""
    t = table("awkward")[0]
    y = reference("awkward")[0]["labels"][0][0]
    assert len(y) >= 2, y
    arcs, s = [], 0
    for v in y:
        lo, hi = t["arc_begin"][s], t["arc_begin"][s + 1]
        q = lo + t["arc_label"][lo:hi].index(v)     # dense: every state holds every label
        arcs.append(q)
        s = t["arc_next"][q]
    return tuple(arcs[1:])


@functools.lru_cache(maxsize=None)
def drop_state():
    return _state_after(table("awkward")[0], reference("awkward")[0]["labels"][0][0])


def f32_error(name):
    r64, r32, _ = reference(name)
    return max([abs(float(x) - float(y)) for a, b in zip(r32["scores"], r64["scores"]) for x, y in zip(a, b)] + [0.0])


@functools.lru_cache(maxsize=None)
def score_tol():
    """4 x the largest |float32 restatement - float64| reported score over the cases (4: the device's summation order differs)"""
    err = max(f32_error(nm) for nm in ALL_CASES)
    print("largest float32-restatement score error over the cases: %.3e -> tolerance %.3e" % (err, 4 * err))
    assert err > 0
    return 4 * err


def assert_premise(name):
    r64, r32, lm = reference(name)
    c = case(name)
    live = [b for b, n in enumerate(c["n"]) if n > 0]
    cg, og = min(r64["cut_gap"][b] for b in live), min(r64["order_gap"][b] for b in live)
    print("%s: cut gap %.3e, order gap %.3e, backoffs %d, unknown %d, -inf terms %d; labels %s" % (name, cg, og, lm.backoffs, lm.unk, lm.dead,
                                                                                                 r64["labels"]))
    assert cg >= GAP and og >= GAP, (name, cg, og)
    assert r32["labels"] == r64["labels"], name
    assert any(len(y) > 0 for b in live for y in r64["labels"][b]), (name, "needs a label")
    if name in SPARSE:
        assert lm.backoffs > 0 and lm.unk > 0, (name, lm.backoffs, lm.unk)
