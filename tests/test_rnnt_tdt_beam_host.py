"""The ground the device tests of the token-and-duration beam search stand on (tests/test_gpu_rnnt_tdt_beam.py imports the cases from
here): the float64 reference (tests/rnnt_tdt_beam_reference.py) against tdt_path_mass, a forward recursion that knows nothing of the
search, and the premises of every named case.  The seeds were chosen here on the CPU; nothing about them comes from a device.  No GPU."""
import functools

import numpy as np
import pytest

import rnnt_beam_reference as RB
import rnnt_tdt_beam_reference as R

GAP = 1e-3


def model(seed, V, E, H, J, proj, durs, blank=0, label_bias=0.0):
    rng = np.random.default_rng(seed)
    u = lambda sc, *s: rng.uniform(-sc, sc, s).astype(np.float32)
    G, D = 4 * H, len(durs)
    bias = u(0.1, V + D)
    bias[:V][np.arange(V) != blank] += np.float32(label_bias)
    return dict(V=V, E=E, H=H, J=J, blank=blank, durs=durs, embed=u(1.0, V, E),
                lstm=np.concatenate([u(2.0 * E ** -0.5, E * G), u(2.0 * H ** -0.5, H * G), u(0.1, G), u(0.1, G)]),
                proj=np.concatenate([u(2.0 * H ** -0.5, H * J), u(0.1, J)]) if proj else None,
                out=np.concatenate([u(3.0 * J ** -0.5, J * (V + D)), bias]), rng=rng)


# name: (seed, V, E, H, J, projection, durations, blank, label bias, (batch, T), n_frames, activation, S, W, nbest, max_labels)
# awkward*: E, H, J no multiples of 4, V % 64 != 0, a row without frames; big_v: V + D > 1024; skip: odd frames are never landed on;
# clamp: jumps overshoot n; pruned: merges, cuts and a hypothesis at max_labels; ring: the ring (17 frames) is longer than the row
CASES = {"awkward": (0, 5, 7, 13, 22, True, (0, 1, 2, 3), 0, -1.0, (3, 10), [10, 4, 0], "tanh", 3, 8, 3, None),
         "awkward_w3": (0, 5, 7, 13, 22, True, (0, 1, 2, 3), 0, -1.0, (3, 10), [10, 4, 0], "tanh", 1, 3, 2, None),
         "awkward_w1": (0, 5, 7, 13, 22, True, (0, 1, 2, 3), 0, -1.0, (3, 10), [10, 4, 0], "tanh", 3, 1, 1, None),
         "big_v": (0, 1030, 5, 16, 16, False, (1, 2), 1029, -1.0, (2, 4), [4, 3], "relu", 1, 3, 2, None),
         "skip": (0, 6, 5, 16, 16, False, (0, 2, 4), 2, -1.0, (2, 11), [11, 8], "tanh", 2, 4, 2, None),
         "clamp": (0, 6, 5, 16, 16, False, (2, 3), 2, -1.0, (2, 9), [9, 4], "identity", 2, 4, 2, None),
         "pruned": (0, 5, 7, 13, 22, True, (0, 1, 2), 0, 0.5, (2, 9), [9, 5], "tanh", 3, 3, 3, 3),
         "ring": (1, 5, 7, 13, 22, True, (0, 1, 16), 0, -1.0, (2, 9), [9, 6], "tanh", 2, 4, 2, None)}
NEEDS = {"skip": ("skipped_frames",), "clamp": ("clamped",), "pruned": ("merges", "cuts", "at_max"), "ring": ("clamped",)}


def case(name):
    """dict(m = the model, enc, n, act, ms = max_symbols_per_frame, W, nbest, max_labels)"""
    if name == "tie":                                # W_out = 0: the scores are the bias; labels 1 and 3 share it, and so do both durations
        m = model(5, 5, 7, 13, 22, True, (1, 2))
        m["out"][:22 * 7] = 0.0
        m["out"][22 * 7:] = np.float32([0.5, 0.25, -1.0, 0.25, -2.0, 0.125, 0.125])
        return dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, (2, 4, 22)).astype(np.float32), n=[4, 2], act="tanh", ms=2, W=5, nbest=3, max_labels=8)
    seed, V, E, H, J, proj, durs, blank, lb, shape, n, act, ms, W, nbest, ml = CASES[name]
    m = model(seed, V, E, H, J, proj, durs, blank, lb)
    return dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, shape + (J,)).astype(np.float32), n=n, act=act, ms=ms, W=W, nbest=nbest,
                max_labels=ml if ml is not None else ms * shape[1])


def exhaustive_case(durs, blank):
    """V 3, at most 2 labels, S 2, nbest 8; W 32, not 8: the 3 hypotheses that can be extended have 3 * 2 * D cells, which 8 would cut"""
    m = model(3 + blank, 3, 7, 13, 22, True, durs, blank)
    return dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, (3, 5, 22)).astype(np.float32), n=[5, 2, 3], act="tanh", ms=2, W=32, nbest=8, max_labels=2)


def search(c, dtype=np.float64):
    m = c["m"]
    return R.tdt_beam_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], m["durs"], n_frames=c["n"], blank=m["blank"],
                             activation=c["act"], max_symbols_per_frame=c["ms"], beam_width=c["W"], nbest=c["nbest"],
                             max_labels=c["max_labels"], dtype=dtype)


def path_mass(c, b, y):
    """tdt_path_mass of row b's sequence y on float64 logits"""
    m = c["m"]
    wide = np.concatenate([m["embed"], np.zeros((len(m["durs"]), m["E"]), np.float32)])         # V + D rows: the block is that wide
    x = RB.lattice_logits(wide, m["lstm"], m["proj"], m["out"], c["enc"][b, :c["n"][b]], y, m["blank"], c["act"])
    return R.tdt_path_mass(x, y, m["durs"], m["blank"])


@functools.lru_cache(maxsize=None)
def reference(name):
    return search(case(name)), search(case(name), np.float32)


@functools.lru_cache(maxsize=None)
def score_tol():
    err = max(abs(float(x) - float(y)) for nm in list(CASES) + ["tie"] for a, b in zip(*(r["scores"] for r in reference(nm)))
              for x, y in zip(a, b))
    print("largest float32-restatement score error over the cases: %.3e -> tolerance %.3e" % (err, 4 * err))
    assert err > 0
    return 4 * err


EXHAUSTIVE = [(d, b) for d in ((0, 1), (1, 2), (0, 1, 2, 4)) for b in (0, 2)]


@pytest.mark.parametrize("durs,blank", EXHAUSTIVE)
def test_unpruned_scores_are_the_path_masses(durs, blank):
    c = exhaustive_case(durs, blank)
    r = search(c)
    assert r["cuts"].sum() == 0
    for b in range(3):
        assert len(r["final"][b]) == 7 and all(abs(s - path_mass(c, b, y)) <= 1e-10 for y, s in r["final"][b]), (b, r["final"][b])

    if durs == (0, 1):                               # S large: the masses of all sequences of up to 3 labels sum to at most 1
        r = search(dict(c, ms=9, max_labels=3, nbest=32))
        assert all(len(f) == 15 and 0.0 < np.exp([s for _, s in f]).sum() <= 1.0 + 1e-12 for f in r["final"]) and r["cuts"].sum() == 0


@pytest.mark.parametrize("name", list(CASES) + ["tie"])
def test_named_cases_meet_their_premises(name):
    r64, r32 = reference(name)
    if name == "tie":                                # exact ties at a cut and in the final order, by construction
        assert r64["cut_gap"][0] == 0.0 and r64["order_gap"][0] == 0.0 and r64["labels"][0][:2] == [[1], [3]]
        return
    live = [b for b, n in enumerate(case(name)["n"]) if n > 0]
    print("%s: cut gap %.3e, order gap %.3e; labels %s" % (name, r64["cut_gap"][live].min(), r64["order_gap"][live].min(), r64["labels"]))
    assert r64["cut_gap"][live].min() >= GAP and r64["order_gap"][live].min() >= GAP
    assert r32["labels"] == r64["labels"] and any(len(y) > 0 for b in live for y in r64["labels"][b])
    assert all(r64[k].sum() > 0 for k in NEEDS.get(name, ())), {k: r64[k] for k in NEEDS.get(name, ())}
    if name == "pruned":
        assert any(len(y) == 3 for y in r64["labels"][0])
