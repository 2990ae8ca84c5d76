"""The n-gram language model of the fused CTC beam search: what the host layer decides without a device (csrc/host/ngram_lm.c,
ctc.c) -- every refusal of nntk_ngram_lm_create, nntk_ngram_lm_score against a float64 walk, the ARPA parser, the size functions,
the empty batch.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from nntoolkitcore_amd import capi, layers as NL

INF = float("inf")


def random_trigram(seed, n_classes, blank, n_bi, n_tri, arcs0=None):
    """A random backoff automaton: state 0, n_bi one-label contexts (x) that state 0 reaches, up to n_tri two-label contexts (x, a)
    that the state (x) reaches, each backing off to (a) where that is a state, else to state 0 -> from_arrays' keyword arguments"""
    rng = np.random.default_rng(seed)
    labels = [c for c in range(n_classes) if c != blank]
    uni = sorted(rng.choice(labels, n_bi, replace=False).tolist())
    pick = lambda k, must=(): sorted(set(must) | set(rng.choice(labels, k, replace=False).tolist()))
    arcs = {(): pick(arcs0 if arcs0 is not None else len(labels) - 2, uni)}
    for x in uni:
        arcs[(x,)] = pick(int(rng.integers(2, max(3, len(labels) // 3))))
    pairs = [(x, a) for x in uni for a in arcs[(x,)]]
    for q in sorted(rng.choice(len(pairs), min(n_tri, len(pairs)), replace=False).tolist()):
        arcs[pairs[q]] = pick(int(rng.integers(1, max(2, len(labels) // 3))))
    ctx = sorted(arcs, key=lambda c: (len(c), c))
    sid = {c: i for i, c in enumerate(ctx)}

    def state_of(hist):
        hist = hist[-2:]
        while hist not in sid:
            hist = hist[1:]
        return sid[hist]
    arc_begin, arc_label, arc_logp, arc_next, bo_s, bo_w = [0], [], [], [], [], []
    for c in ctx:
        for a in arcs[c]:
            arc_label.append(a); arc_logp.append(float(np.log(rng.uniform(0.02, 0.9)))); arc_next.append(state_of(c + (a,)))
        arc_begin.append(len(arc_label))
        bo_s.append(-1 if not c else state_of(c[1:]))
        bo_w.append(0.0 if not c else float(np.log(rng.uniform(0.2, 0.9))))
    final = np.log(rng.uniform(0.05, 0.9, len(ctx))).tolist()
    return dict(n_classes=n_classes, blank=blank, arc_begin=arc_begin, arc_label=arc_label, arc_logp=arc_logp, arc_next=arc_next,
                backoff_state=bo_s, backoff_logw=bo_w, final_logp=final, start_state=0, unk_logp=float(np.log(0.01)))


def walk64(t, s, c, alpha, beta):
    """float64 restatement of the walk: -> (ln F, next state, backoffs taken, whether the unknown-label case was hit)"""
    ln, depth = 0.0, 0
    while True:
        lo, hi = t["arc_begin"][s], t["arc_begin"][s + 1]
        lab = t["arc_label"][lo:hi]
        if c in lab:
            q = lo + lab.index(c)
            return ln + alpha * np.float64(np.float32(t["arc_logp"][q])) + beta, t["arc_next"][q], depth, False
        if s == 0:
            return ln + alpha * np.float64(np.float32(t["unk_logp"])) + beta, 0, depth, True
        ln += alpha * np.float64(np.float32(t["backoff_logw"][s]))
        s = t["backoff_state"][s]
        depth += 1


GOOD = dict(n_classes=4, blank=3, arc_begin=[0, 2, 3], arc_label=[0, 2, 1], arc_logp=[-1.0, -2.0, -0.5], arc_next=[1, 0, 0],
            backoff_state=[-1, 0], backoff_logw=[0.0, -0.3], final_logp=[-1.0, -INF], start_state=0, unk_logp=-5.0, alpha=1.0, beta=0.0)
NAN = float("nan")
BAD = {
    "arc_begin_start": dict(arc_begin=[1, 2, 3]),
    "arc_begin_not_monotone": dict(arc_begin=[0, 3, 2]),
    "arc_begin_2_31": dict(arc_begin=[0, 2, 2 ** 31]),
    "label_unsorted": dict(arc_label=[2, 0, 1]),
    "label_repeated": dict(arc_label=[0, 0, 1]),
    "label_range": dict(arc_label=[0, 4, 1]),
    "label_negative": dict(arc_label=[-1, 2, 1]),
    "label_blank": dict(arc_label=[0, 3, 1]),
    "next_range": dict(arc_next=[1, 2, 0]),
    "next_negative": dict(arc_next=[-1, 0, 0]),
    "start_range": dict(start_state=2),
    "start_negative": dict(start_state=-1),
    "backoff_root": dict(backoff_state=[0, 0]),
    "backoff_order": dict(backoff_state=[-1, 1]),
    "backoff_negative": dict(backoff_state=[-1, -1]),
    "arc_nan": dict(arc_logp=[NAN, -2.0, -0.5]),
    "arc_plus_inf": dict(arc_logp=[-1.0, INF, -0.5]),
    "backoff_minus_inf": dict(backoff_logw=[0.0, -INF]),
    "backoff_nan": dict(backoff_logw=[NAN, 0.0]),
    "final_nan": dict(final_logp=[NAN, 0.0]),
    "final_plus_inf": dict(final_logp=[0.0, INF]),
    "unk_nan": dict(unk_logp=NAN),
    "unk_plus_inf": dict(unk_logp=INF),
    "alpha_negative": dict(alpha=-0.5),
    "alpha_nan": dict(alpha=NAN),
    "beta_inf": dict(beta=INF),
    "beta_nan": dict(beta=NAN),
    "blank_range": dict(blank=4),
    "blank_negative": dict(blank=-1),
}


def _create_raw(a):
    """through ctypes directly, so that nothing but the library checks the arrays (2^31 arcs: only arc_begin says so)"""
    ab = np.asarray(a["arc_begin"], np.int64)
    i32 = lambda k: np.asarray(a[k], np.int32)
    f32 = lambda k: np.asarray(a[k], np.float32)
    al, an, bs, ap, bw, fl = i32("arc_label"), i32("arc_next"), i32("backoff_state"), f32("arc_logp"), f32("backoff_logw"), f32("final_logp")
    return capi.load().nntk_ngram_lm_create(a["n_classes"], a["blank"], len(ab) - 1, ab.ctypes.data_as(C.POINTER(C.c_long)),
                                            al.ctypes.data_as(capi.ip), ap.ctypes.data_as(capi.fp), an.ctypes.data_as(capi.ip),
                                            bs.ctypes.data_as(capi.ip), bw.ctypes.data_as(capi.fp), fl.ctypes.data_as(capi.fp),
                                            a["start_state"], a["unk_logp"], a["alpha"], a["beta"])


def test_create_accepts_the_good_table_without_a_device():
    L = capi.load()
    h = _create_raw(GOOD)
    assert h and capi.last_error() == ""
    assert L.nntk_ngram_lm_device_bytes(h) == 16 * (3 + 2 * 2)
    L.nntk_ngram_lm_destroy(h)
    L.nntk_ngram_lm_destroy(None)


@pytest.mark.parametrize("name", list(BAD))
def test_create_refuses(name):
    h = _create_raw(dict(GOOD, **BAD[name]))
    assert not h and capi.last_error().startswith("nntk_ngram_lm_create: "), name


def test_score_equals_a_float64_walk():
    """a sparse random trigram; the sampled strings take 0, 1 and 2 backoffs and hit the unknown-label case (asserted)"""
    t = random_trigram(1, 12, 5, 6, 14, arcs0=3)
    alpha, beta = 0.75, 0.25                                  # exact in float32, the type of the C arguments
    lm = NL.NgramLm.from_arrays(alpha=alpha, beta=beta, **t)
    rng = np.random.default_rng(2)
    labels = [c for c in range(12) if c != 5]
    depths, unk = set(), False
    for _ in range(2000):
        s = rng.choice(labels, int(rng.integers(0, 12))).tolist()
        want, st = 0.0, 0
        for c in s:
            ln, st, d, u = walk64(t, st, c, alpha, beta)
            want += ln
            depths.add(d)
            unk |= u
        got = lm.score(s)
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), s
        fin = lm.score(s, with_final=True)
        assert abs(fin - (want + alpha * np.float64(np.float32(t["final_logp"][st])))) <= 1e-12 * max(1.0, abs(want)), s
    assert depths >= {0, 1, 2} and unk
    assert lm.score([]) == 0.0
    with pytest.raises(capi.NNTKError):
        lm.score([5])
    lm.close()
    # -inf factors: the sum is -inf, not NaN; alpha == 0 switches the model off whatever it holds
    dead = NL.NgramLm.from_arrays(**dict(GOOD, alpha=1.0, unk_logp=-INF))
    assert dead.score([1]) == -INF and dead.score([0], with_final=True) == -INF and dead.score([0, 1, 1]) == -INF
    assert abs(dead.score([0, 0]) - (-1.0 - 0.3 - 1.0)) < 1e-6 and dead.score([0, 1]) == -1.5
    off = NL.NgramLm.from_arrays(**dict(GOOD, alpha=0.0, beta=0.25, unk_logp=-INF))
    assert off.score([1, 0, 0], with_final=True) == 0.75


ARPA = """\\data\\
ngram 1=4
ngram 2=3

\\1-grams:
-1.0 <s> -0.5
-0.7 </s>
-0.4 a -0.3
-0.6 b

\\2-grams:
-0.2 <s> a
-0.1 a b
-0.3 a </s>

\\end\\
"""


def test_from_arpa_on_a_hand_computed_model():
    """states, shortest context first and sorted: 0 = (), 1 = (<s>), 2 = (a), 3 = (b); classes a = 0, b = 2, blank = 1"""
    ln10 = np.log(10.0)
    got = NL.NgramLm.arpa_arrays(ARPA, {"a": 0, "b": 2})
    assert got["arc_begin"] == [0, 2, 3, 4, 4]
    assert got["arc_label"] == [0, 2, 0, 2]                  # () -> a, b;  (<s>) -> a;  (a) -> b;  (b): none
    assert got["arc_next"] == [2, 3, 2, 3]
    np.testing.assert_allclose(got["arc_logp"], np.array([-0.4, -0.6, -0.2, -0.1]) * ln10, rtol=1e-15)
    assert got["backoff_state"] == [-1, 0, 0, 0]
    np.testing.assert_allclose(got["backoff_logw"], np.array([0.0, -0.5, -0.3, 0.0]) * ln10, rtol=1e-15)
    # </s>: the unigram from (); backoff(<s>) + unigram from (<s>); the bigram from (a); backoff(b) = 0 + unigram from (b)
    np.testing.assert_allclose(got["final_logp"], np.array([-0.7, -1.2, -0.3, -0.7]) * ln10, rtol=1e-15)
    assert got["start_state"] == 1
    lm = NL.NgramLm.from_arpa(ARPA, {"a": 0, "b": 2}, blank=1, alpha=1.0, beta=0.0, unk_logp=-9.0)
    # <s> a b </s> = -0.2 + -0.1 + (0 + -0.7);  <s> b = backoff(<s>) + unigram b
    assert abs(lm.score([0, 2], with_final=True) - (-0.2 - 0.1 - 0.7) * ln10) < 1e-6
    assert abs(lm.score([2]) - (-0.5 - 0.6) * ln10) < 1e-6
    lm.close()


def test_size_functions_are_monotone_and_64_bit():
    L = capi.load()
    ws, base_ws = L.nntk_ctc_beam_lm_workspace_floats, L.nntk_ctc_beam_workspace_floats
    base = ws(4, 50, 29, 16, 0)
    assert base > base_ws(4, 50, 29, 16, 0) > 0
    assert ws(5, 50, 29, 16, 0) > base and ws(4, 51, 29, 16, 0) > base and ws(4, 50, 29, 17, 0) > base and ws(4, 50, 29, 16, 5) > base
    assert ws(4096, 4000, 64, 128, 0) > 2 ** 33
    sb, sb0 = L.nntk_ctc_beam_stream_state_bytes_lm, L.nntk_ctc_beam_stream_state_bytes
    assert sb(4, 50, 29, 16, 0, 100) - sb0(4, 50, 29, 16, 0, 100) == 4 * 4 * 16          # 4 more bytes per row and beam entry
    assert sb(5, 50, 29, 16, 0, 100) > sb(4, 50, 29, 16, 0, 100) and sb(4, 50, 29, 17, 0, 100) > sb(4, 50, 29, 16, 0, 100)
    assert sb(4, 51, 29, 16, 0, 100) > sb(4, 50, 29, 16, 0, 100) and sb(4, 50, 29, 16, 0, 101) > sb(4, 50, 29, 16, 0, 100)
    assert sb(4096, 1000, 64, 128, 0, 4096) > 2 ** 34


def test_empty_batch_and_mismatch_need_no_device():
    L = capi.load()
    h = _create_raw(GOOD)
    assert L.nntk_ctc_beam_decode_lm_device(None, 0, 6, 4, None, 3, 4, 0, 2, h, None, None, None, None) == 0
    assert L.nntk_ctc_beam_decode_lm(None, 0, 6, 4, None, 3, 4, 0, 2, h, None, None, None) == 0
    assert L.nntk_ctc_beam_decode_lm_device(None, 0, 6, 4, None, 3, 4, 0, 2, None, None, None, None, None) == 0
    assert capi.last_error() == ""
    s = L.nntk_ctc_beam_stream_create_lm(0, 8, 4, 3, 4, 0, 2, 16, h)
    assert s and L.nntk_ctc_beam_stream_push_device(s, None, None, None, None, None, None) == 0 and capi.last_error() == ""
    L.nntk_ctc_beam_stream_destroy(s)
    # another class count, another blank: refused before any device is touched
    assert L.nntk_ctc_beam_decode_lm_device(None, 2, 6, 5, None, 3, 4, 0, 2, h, None, None, None, None) == -1 and capi.last_error() != ""
    assert L.nntk_ctc_beam_decode_lm(None, 2, 6, 4, None, 2, 4, 0, 2, h, None, None, None) == -1 and capi.last_error() != ""
    assert not L.nntk_ctc_beam_stream_create_lm(2, 8, 5, 3, 4, 0, 2, 16, h) and capi.last_error() != ""
    assert not L.nntk_ctc_beam_stream_create_lm(2, 8, 4, 2, 4, 0, 2, 16, h) and capi.last_error() != ""
    L.nntk_ngram_lm_destroy(h)


def test_the_symbols_are_exported_and_bound():
    L = capi.load()
    for name in ("nntk_ngram_lm_create", "nntk_ngram_lm_score", "nntk_ngram_lm_device_bytes", "nntk_ngram_lm_destroy",
                 "nntk_ctc_beam_lm_workspace_floats", "nntk_ctc_beam_decode_lm_device", "nntk_ctc_beam_decode_lm",
                 "nntk_ctc_beam_stream_create_lm", "nntk_ctc_beam_stream_state_bytes_lm"):
        assert name in capi.SIGNATURES and getattr(L, name).argtypes == capi.SIGNATURES[name][1], name
