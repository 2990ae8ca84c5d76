"""The acoustic cases of the transducer beam search tests (tests/test_gpu_rnnt_beam.py; tests/rnnt_beam_lm_cases.py and
tests/rnnt_beam_detail_cases.py build on them) and their premises, which need no device: the models and frames, the float64 reference
(tests/rnnt_beam_reference.py) with its float32 restatement, and the score tolerance formed from the two.  A helper, no test."""
import functools

import numpy as np

import rnnt_beam_reference as RB

GAP = 1e-3


def model(seed, V, E, H, J, proj, blank=0, scale=2.0, out_scale=3.0, label_bias=0.0):
    rng = np.random.default_rng(seed)
    u = lambda sc, *s: rng.uniform(-sc, sc, s).astype(np.float32)
    G = 4 * H
    bias = u(0.1, V)
    bias[np.arange(V) != blank] += np.float32(label_bias)
    return dict(V=V, E=E, H=H, J=J, blank=blank, embed=u(1.0, V, E),
                lstm=np.concatenate([u(scale * E ** -0.5, E * G), u(scale * H ** -0.5, H * G), u(0.1, G), u(0.1, G)]),
                proj=np.concatenate([u(scale * H ** -0.5, H * J), u(0.1, J)]) if proj else None,
                out=np.concatenate([u(out_scale * J ** -0.5, J * V), bias]), rng=rng)


# seeds chosen on the CPU so that assert_premise holds
SEEDS = {"awkward": 0, "awkward_w3": 0, "awkward_w1": 15, "big_v": 0, "wide_identity": 0, "pruned": 3, "stream": 2}


def case(name):
    """dict(m = the model, enc, n, act, ms = max_symbols_per_frame, W, nbest, max_labels)"""
    if name in ("awkward", "awkward_w3", "awkward_w1", "pruned"):
        # E 7, H 13, J 22 (none a multiple of 4), V 5, tanh, with the projection; batch 3, T 9, one row without frames
        W, nbest, ms, ml = {"awkward": (8, 3, 3, None), "awkward_w3": (3, 2, 1, None), "awkward_w1": (1, 1, 3, None),
                            "pruned": (3, 3, 3, 3)}[name]
        m = model(SEEDS[name], 5, 7, 13, 22, True, label_bias=-1.0 if name != "pruned" else 0.5)
        return dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, (3, 9, 22)).astype(np.float32), n=[9, 4, 0], act="tanh", ms=ms, W=W, nbest=nbest,
                    max_labels=ml)
    if name == "big_v":                              # more classes than lanes, no projection, relu
        m = model(SEEDS[name], 1030, 5, 16, 16, False, blank=1029, label_bias=-1.0)
        return dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, (2, 4, 16)).astype(np.float32), n=[4, 3], act="relu", ms=1, W=3, nbest=2,
                    max_labels=None)
    if name == "wide_identity":                      # more classes than a wavefront, no projection, identity
        m = model(SEEDS[name], 70, 5, 33, 33, False, blank=69, label_bias=-1.5)
        return dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, (2, 6, 33)).astype(np.float32), n=[6, 5], act="identity", ms=3, W=8, nbest=4,
                    max_labels=None)
    if name == "stream":                             # T 12
        m = model(SEEDS[name], 6, 5, 16, 16, False, blank=2, label_bias=-1.0)
        return dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, (3, 12, 16)).astype(np.float32), n=[12, 12, 7], act="tanh", ms=3, W=5, nbest=3,
                    max_labels=12)
    if name == "tie":                                # W_out = 0: the logits are the bias; labels 1 and 3 share it
        m = model(5, 5, 7, 13, 22, True, blank=0)
        m["out"][:22 * 5] = 0.0
        m["out"][22 * 5:] = np.float32([0.5, 0.25, -1.0, 0.25, -2.0])
        return dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, (2, 4, 22)).astype(np.float32), n=[4, 2], act="tanh", ms=2, W=3, nbest=3,
                    max_labels=None)
    raise KeyError(name)


GAP_CASES = ("awkward", "awkward_w3", "awkward_w1", "big_v", "wide_identity", "pruned", "stream")
ALL_CASES = GAP_CASES + ("tie",)


def ml(c):
    return c["max_labels"] if c["max_labels"] is not None else max(1, c["ms"] * c["enc"].shape[1])


def search_kw(c):
    """the case's keyword arguments of rnnt_beam_reference.beam_decode"""
    m = c["m"]
    return dict(n_frames=c["n"], blank=m["blank"], activation=c["act"], max_symbols_per_frame=c["ms"], beam_width=c["W"], nbest=c["nbest"],
                max_labels=ml(c))


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    m, kw = c["m"], search_kw(c)
    r64 = RB.beam_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], **kw)
    r32 = RB.beam_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], dtype=np.float32, **kw)
    return r64, r32


def f32_error(name):
    r64, r32 = reference(name)
    return max([abs(float(x) - float(y)) for a, b in zip(r32["scores"], r64["scores"]) for x, y in zip(a, b)] + [0.0])


@functools.lru_cache(maxsize=None)
def score_tol():
    err = max(f32_error(nm) for nm in ALL_CASES)
    print("largest float32-restatement score error over the cases: %.3e -> tolerance %.3e" % (err, 4 * err))
    assert err > 0
    return 4 * err


def assert_premise(name):
    r64, r32 = reference(name)
    c = case(name)
    live = [b for b, n in enumerate(c["n"]) if n > 0]
    print("%s: cut gap %.3e, order gap %.3e; labels %s" % (name, min(r64["cut_gap"][b] for b in live),
                                                          min(r64["order_gap"][b] for b in live), r64["labels"]))
    assert min(r64["cut_gap"][b] for b in live) >= GAP and min(r64["order_gap"][b] for b in live) >= GAP, name
    assert r32["labels"] == r64["labels"], name
    assert any(len(y) > 0 for b in live for y in r64["labels"][b]), (name, "needs a label")
