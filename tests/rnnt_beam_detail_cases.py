"""The cases of the transducer beam search's label timestamps, confidences and length normalisation (tests/test_gpu_rnnt_beam_detail.py)
and their premises, which tests/test_rnnt_beam_detail_host.py checks without a device: the geometries of tests/rnnt_beam_cases.py,
tests/rnnt_wide_cases.py (b4) and tests/rnnt_beam_lm_cases.py, the float64 reference (tests/rnnt_beam_reference.py) and its float32
restatement.  A helper, no test.

Where a geometry's existing seed does not give the premises (a gap below GAP at a merge's lead or between the keys, no switch, no
reordering), the case takes the same geometry with another seed, searched on the CPU alone; nothing about a seed comes from a device."""
import functools

import numpy as np

import rnnt_beam_lm_cases as LC
import rnnt_beam_reference as RB
import rnnt_wide_cases as WC
from rnnt_beam_cases import case as acoustic_case, model as _model, search_kw

GAP = 1e-3

# name: (where the acoustic case comes from, its name there, the table's name in rnnt_beam_lm_cases or None, length_norm)
CASES = {
    "awkward": ("beam", "awkward", None, False),
    "big_v": ("beam", "big_v", None, False),
    "wide_identity": ("beam", "wide_identity", None, False),
    "b4": ("wide", "b4", None, False),
    "pruned": ("beam", "pruned", None, False),
    "stream": ("beam", "stream", None, False),
    "exhaustive": ("own", "exhaustive", None, False),
    "tie": ("beam", "tie", None, False),
    "lm_stream": ("lm", "stream", "stream", False),
    "lm_wide_identity": ("lm", "wide_identity", "wide_identity", False),
    "norm": ("own", "norm", None, True),
    "lm_norm": ("own", "lm_norm", "stream", True),
    "lm_norm_drop": ("own", "lm_norm_drop", "final_drop", True),
}
GAP_CASES = tuple(nm for nm in CASES if nm != "tie")
ALL_CASES = tuple(CASES)
NORM_CASES = tuple(nm for nm, v in CASES.items() if v[3])
STREAM_CASES = ("stream", "lm_stream", "norm", "lm_norm")
SEEDS = {"norm": 2, "lm_norm": 0}       # norm: the stream case of rnnt_beam_cases.py itself


def case(name):
    """dict(m, enc, n, act, ms, W, nbest, max_labels) of the acoustic search"""
    src, nm = CASES[name][:2]
    if src == "beam":
        return acoustic_case(nm)
    if src == "wide":
        return WC.beam_case(nm)
    if src == "lm":
        return LC.case(nm)
    if name == "exhaustive":                        # V 3, at most 2 labels, S 2, W = nbest = 8: nothing is pruned
        m = _model(3, 3, 7, 13, 22, True, blank=0)
        return dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, (3, 4, 22)).astype(np.float32), n=[4, 2, 3], act="tanh", ms=2, W=8, nbest=8,
                    max_labels=2)
    if name in ("norm", "lm_norm"):                 # the stream geometry: T 12, rows [12, 12, 7]
        m = _model(SEEDS[name], 6, 5, 16, 16, False, blank=2, label_bias=-1.0)
        return dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, (3, 12, 16)).astype(np.float32), n=[12, 12, 7], act="tanh", ms=3, W=5, nbest=3,
                    max_labels=12)
    if name == "lm_norm_drop":
        return LC.case("final_drop")
    raise KeyError(name)


def lm_table(name):
    """-> (NgramLm.from_arrays' keyword arguments, alpha, beta) or None"""
    return LC.table(CASES[name][2]) if CASES[name][2] else None


def length_norm(name):
    return CASES[name][3]


def run(name, dtype=np.float64, **over):
    c = case(name)
    m = c["m"]
    t = lm_table(name)
    kw = dict(search_kw(c), length_norm=length_norm(name), dtype=dtype)
    kw.update(over)
    return RB.beam_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], lm=RB.Lm(*t) if t else None, **kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (float64 result, float32 restatement); computed once, shared by every test, never changed"""
    return run(name), run(name, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def unranked_labels(name):
    return run(name, length_norm=False)["labels"]


def lps_f32_error(name):
    r64, r32 = reference(name)
    worst = 0.0
    for a, b in zip(r32["lps"], r64["lps"]):
        for x, y in zip(a, b):
            if len(x) == len(y):
                worst = max([worst] + [abs(p - q) for p, q in zip(x, y)])
    return worst


@functools.lru_cache(maxsize=None)
def lps_tol():
    """4 x the largest |float32 restatement - float64| over the lps of all cases (4: the device's summation order differs)"""
    err = max(lps_f32_error(nm) for nm in ALL_CASES)
    print("largest float32-restatement error of a label's log-probability over the cases: %.3e -> tolerance %.3e" % (err, 4 * err))
    assert err > 0
    return 4 * err


def scores_f32_error(name):
    r64, r32 = reference(name)
    return max([abs(float(x) - float(y)) for a, b in zip(r32["scores"], r64["scores"]) for x, y in zip(a, b)] + [0.0])


@functools.lru_cache(maxsize=None)
def score_tol():
    """4 x the largest |float32 restatement - float64| reported score over the cases, as the existing beam tests form it"""
    err = max(scores_f32_error(nm) for nm in ALL_CASES)
    print("largest float32-restatement score error over the cases: %.3e -> tolerance %.3e" % (err, 4 * err))
    assert err > 0
    return 4 * err


def assert_premise(name):
    r64, r32 = reference(name)
    c = case(name)
    live = [b for b, n in enumerate(c["n"]) if n > 0]
    mn = lambda key: min(r64[key][b] for b in live)
    print("%s: cut gap %.3e, order gap %.3e, lead gap %.3e, key gap %.3e; merges %s, switches %s, reordered %s; labels %s frames %s" % (
        name, mn("cut_gap"), mn("order_gap"), mn("lead_gap"), mn("key_gap"), r64["merges"], r64["lead_switches"], r64["reordered"],
        r64["labels"], r64["frames"]))
    if length_norm(name):                           # the ranking alone differs: the same search without it reports plain_labels
        assert r64["plain_labels"] == unranked_labels(name), name
    if name == "tie":                               # exact ties by construction; whatever is no exact tie keeps its distance
        assert r64["lead_ties"].sum() > 0 and mn("lead_gap_nonzero") >= GAP, (name, r64["lead_ties"], mn("lead_gap_nonzero"))
    else:
        assert mn("cut_gap") >= GAP and mn("order_gap") >= GAP and mn("lead_gap") >= GAP, (name, mn("cut_gap"), mn("order_gap"), mn("lead_gap"))
        if length_norm(name):
            assert mn("key_gap") >= GAP, (name, mn("key_gap"))
    assert r32["labels"] == r64["labels"] and r32["frames"] == r64["frames"], name
    assert any(len(y) > 0 for b in live for y in r64["labels"][b]), (name, "needs a label")
    return r64
