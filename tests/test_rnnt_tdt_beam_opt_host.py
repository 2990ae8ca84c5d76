"""The ground the device tests of the token-and-duration beam search's options stand on (tests/test_gpu_rnnt_tdt_beam_opt.py imports the
cases from here): the premises of every case, on the CPU.  The shapes are those of test_rnnt_tdt_beam_host's awkward and awkward_w3; the
model seed, the label bias and the table's seed were searched here so that the premises hold with and without the model and with and
without length normalisation.  Nothing about them comes from a device.  No GPU."""
import functools

import numpy as np
import pytest

import rnnt_beam_reference as RB
import rnnt_tdt_beam_opt_reference as R
import rnnt_tdt_beam_reference as PLAIN
import test_rnnt_tdt_beam_host as H
from ngram_cases import sparse_trigram

GAP = H.GAP
ALPHA, BETA = 0.5, 0.25                              # alpha a power of two: alpha * v + beta is one rounding
VARIANT = {"awkward": (1, -0.5, 0), "awkward_w3": (0, -1.0, 1)}          # name: (model seed, label bias, table seed)
MODES = [(lm, ln) for lm in (False, True) for ln in (False, True)]


def case(name):
    _, V, E, Hh, J, proj, durs, blank, _, shape, n, act, ms, W, nbest, _ = H.CASES[name]
    seed, bias, _ = VARIANT[name]
    m = H.model(seed, V, E, Hh, J, proj, durs, blank, bias)
    return dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, shape + (J,)).astype(np.float32), n=n, act=act, ms=ms, W=W, nbest=nbest,
                max_labels=ms * shape[1])


def table(name):
    """a sparse trigram over V 5, blank 0 (backoffs, unknown labels) with one arc of the empty context at zero mass"""
    t = sparse_trigram(VARIANT[name][2], 5, 0, 2, 3, 3, final=True)
    t["arc_logp"] = list(t["arc_logp"])
    t["arc_logp"][1] = -np.inf
    return t


def search(c, lm=None, length_norm=False, dtype=np.float64, **kw):
    m = c["m"]
    return R.tdt_beam_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], m["durs"], n_frames=c["n"], blank=m["blank"],
                             activation=c["act"], max_symbols_per_frame=c["ms"], beam_width=kw.get("W", c["W"]),
                             nbest=kw.get("nbest", c["nbest"]), max_labels=c["max_labels"], lm=lm, length_norm=length_norm, dtype=dtype)


@functools.lru_cache(maxsize=None)
def reference(name, lm, length_norm):
    """-> the float64 result and the float32 restatement"""
    mk = lambda: RB.Lm(table(name), ALPHA, BETA) if lm else None
    return search(case(name), mk(), length_norm), search(case(name), mk(), length_norm, np.float32)


@functools.lru_cache(maxsize=None)
def score_tol():
    """4 x the largest |float32 restatement - float64| over the cases, scores and logps alike (4: the device's summation order differs)"""
    err = max(abs(float(x) - float(y)) for name in VARIANT for mode in MODES for key in ("scores", "lps")
              for a, b in zip(*(r[key] for r in reference(name, *mode))) for p, q in zip(a, b) for x, y in zip(np.ravel(p), np.ravel(q)))
    print("largest float32-restatement error over the cases, scores and logps: %.3e -> tolerance %.3e" % (err, 4 * err))
    assert err > 0
    return 4 * err


@pytest.mark.parametrize("lm,length_norm", MODES)
@pytest.mark.parametrize("name", list(VARIANT))
def test_cases_meet_their_premises(name, lm, length_norm):
    r64, r32 = reference(name, lm, length_norm)
    live = [b for b, n in enumerate(case(name)["n"]) if n > 0]
    gaps = {k: r64[k][live].min() for k in ("cut_gap", "order_gap", "lead_gap")}
    print(name, gaps, {k: int(r64[k].sum()) for k in R.COUNTS}, r64["labels"], "tolerance %.3e" % score_tol())
    assert min(gaps.values()) >= GAP, gaps
    assert all(r32[k] == r64[k] for k in ("labels", "frames", "durs"))
    assert r64["lead_switches"].sum() > 0 and r64["twins_clamped"].sum() > 0 and r64["clamped_labels"].sum() > 0
    assert not lm or (r64["backoffs"].sum() > 0 and r64["dead_arcs"].sum() > 0)
    for y, _, fr, du, lp in (h for b in live for h in r64["final"][b]):       # the arrays describe one path to bucket[n]
        assert len(fr) == len(du) == len(lp) == len(y) and all(t + d <= u for t, d, u in zip(fr, du, fr[1:])), (y, fr, du)


@pytest.mark.parametrize("name", list(H.CASES) + ["tie"])
def test_with_everything_off_it_is_the_plain_reference(name):
    c = H.case(name)
    for dtype, plain in zip((np.float64, np.float32), H.reference(name)):
        r = search(c, dtype=dtype)
        assert r["labels"] == plain["labels"] and r["scores"] == plain["scores"] and (r["cut_gap"] == plain["cut_gap"]).all()
        assert [[(h[0], h[1]) for h in f] for f in r["final"]] == plain["final"] and (r["merges"] == plain["merges"]).all()
    assert PLAIN.tdt_beam_decode is not R.tdt_beam_decode
