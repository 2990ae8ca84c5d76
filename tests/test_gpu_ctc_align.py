"""CTC forced alignment (csrc/hip/ctc_align.hip) against a float64 Viterbi on log-probabilities, against the CTC loss and against the
greedy decoder.

Reference: ``_ref_row`` below, with the tie-break of include/nntoolkitcore_hip.h (candidates s, s - 1, s - 2; a later one wins only
if strictly greater; end state 2L unless 2L - 1 is strictly greater).  It also returns the smallest gap, in ln units, between the
best and the second-best finite candidate over all of the row's decisions (every frame and state, and the choice of the end state).

What parity means.  Score: |score - ref| <= 2 (T_b + 2) 2^-24 + 2^-22 |ref| -- each of the T_b multiplications rounds once to 2^-24
relative, max never rounds, one final conversion; the factor 2 is margin.  It holds even where the device takes another
near-optimal path.  States and spans: equal to the reference's for every row whose smallest gap exceeds 4 (T_b + 2) 2^-24 (no
rounding can flip a decision there); the other rows are left out of the exact comparison only, they are at most a quarter of a
case's rows (asserted), and their paths are still checked for validity.  The seeds are fixed; checked with the reference alone,
test_long_free_paths leaves out 2 of its 16 rows and no other case leaves out any."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from nntoolkitcore_amd import capi, layers as NL

pytestmark = pytest.mark.gpu
NINF = -np.inf


def _softmax(rng, B, T, Cc, scale=3.0):
    z = scale * rng.standard_normal((B, T, Cc))
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def _min_len(lab):
    return len(lab) + sum(1 for i in range(1, len(lab)) if lab[i] == lab[i - 1])


def _ref_row(p, lab, blank, want_gap=True):
    """p [T_b][C] float64, the row's valid frames -> (states or None, ln of the best path's probability, smallest decision gap)"""
    Tb, L = p.shape[0], len(lab)
    S = 2 * L + 1
    if Tb == 0:
        return ([], 0.0, np.inf) if L == 0 else (None, NINF, np.inf)
    cls = np.array([blank if s % 2 == 0 else lab[s // 2] for s in range(S)])
    skip = np.array([s % 2 == 1 and s >= 3 and cls[s] != cls[s - 2] for s in range(S)])
    with np.errstate(divide="ignore"):
        lp = np.log(p[:, cls])
    v = np.full(S, NINF)
    v[:2] = lp[0, :2]
    bp = np.zeros((Tb, S), np.int8)
    gap = np.inf

    def decide(cands):
        nonlocal gap
        if not want_gap:
            return
        c = np.sort(np.stack(cands), 0)[::-1]
        both = np.isfinite(c[1])
        if both.any():
            gap = min(gap, float((c[0][both] - c[1][both]).min()))

    for t in range(1, Tb):
        c0 = v
        c1 = np.concatenate(([NINF], v[:-1]))
        c2 = np.full(S, NINF)
        c2[2:] = np.where(skip[2:], v[:-2], NINF)
        decide((c0, c1, c2))
        best, step = c0.copy(), np.zeros(S, np.int8)
        for k, c in ((1, c1), (2, c2)):
            m = c > best
            best[m], step[m] = c[m], k
        bp[t] = step
        v = best + lp[t]
    end, score = S - 1, v[S - 1]
    if S > 1:
        decide((v[S - 1:S], v[S - 2:S - 1]))
        if v[S - 2] > score:
            end, score = S - 2, v[S - 2]
    if score == NINF:
        return None, NINF, gap
    states = [0] * Tb
    for t in range(Tb - 1, -1, -1):
        states[t] = end
        end -= int(bp[t, end])
    return states, float(score), gap


def _spans_of(states, L):
    sp = np.full((L, 2), -1, np.int32)
    for t, s in enumerate(states):
        if s % 2 == 1:
            i = s // 2
            if sp[i, 0] < 0:
                sp[i, 0] = t
            sp[i, 1] = t + 1
    return sp


def _reference(p, lens, labels, blank, maxL, want_gap=True):
    """-> states [B][T] int32, spans [B][maxL][2] int32, float64 scores [B], the decision gap of every row [B]"""
    B, T, _ = p.shape
    st, sp = np.full((B, T), -1, np.int32), np.full((B, maxL, 2), -1, np.int32)
    sc, gaps = np.full(B, NINF), np.full(B, np.inf)
    for b in range(B):
        states, sc[b], gaps[b] = _ref_row(p[b, :lens[b]].astype(np.float64), labels[b], blank, want_gap)
        if states is not None:
            st[b, :lens[b]] = states
            sp[b, :len(labels[b])] = _spans_of(states, len(labels[b]))
    return st, sp, sc, gaps


def _pad(labels, maxL):
    lab = np.zeros((len(labels), maxL), np.int32)
    for b, l in enumerate(labels):
        lab[b, :len(l)] = l
    return lab, np.array([len(l) for l in labels], np.int32)


def _run(gpu, p, lens, labels, blank, maxL):
    lab, ll = _pad(labels, maxL)
    out = NL.ctc_align_device(torch.from_numpy(p).to(gpu), lab, ll, np.asarray(lens, np.int32), blank)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _tol(Tb, ref):
    return 2.0 * (np.asarray(Tb) + 2) * 2.0 ** -24 + 2.0 ** -22 * np.abs(ref)


def _assert_valid(tag, states, spans, score, Tb, lab, blank):
    """a returned path is an alignment of lab, or the row is marked as having none"""
    L = len(lab)
    assert (states[Tb:] == -1).all() and (spans[L:] == -1).all(), tag
    if np.isneginf(score):
        assert (states == -1).all() and (spans == -1).all(), tag
        return
    s = states[:Tb]
    if Tb == 0:
        assert L == 0, tag
        return
    assert s[0] in (0, 1) and s[-1] in (2 * L - 1, 2 * L) and s.min() >= 0, (tag, s)
    d = np.diff(s)
    assert ((d >= 0) & (d <= 2)).all(), (tag, s)
    for t in np.nonzero(d == 2)[0]:
        k = s[t + 1]
        assert k % 2 == 1 and lab[k // 2] != lab[k // 2 - 1], (tag, t, s)
    np.testing.assert_array_equal(spans[:L], _spans_of(s, L), err_msg=tag)


def _check(tag, got, ref, lens, labels, blank, exact=True):
    st, sp, sc = got
    rst, rsp, rsc, gaps = ref
    lens = np.asarray(lens)
    fin = np.isfinite(rsc)
    np.testing.assert_array_equal(np.isneginf(sc), ~fin, err_msg=tag)
    err = np.abs(sc[fin].astype(np.float64) - rsc[fin])
    tol = _tol(lens[fin], rsc[fin])
    print("%s: largest score error / allowed %.3g" % (tag, (err / tol).max(initial=0.0)))
    assert (err <= tol).all(), (tag, err, tol)
    for b in range(len(lens)):
        _assert_valid("%s row %d" % (tag, b), st[b], sp[b], sc[b], lens[b], labels[b], blank)
    if exact:
        sure = gaps > 4.0 * (lens + 2) * 2.0 ** -24
        print("%s: %d of %d rows left out of the exact comparison (smallest gap %.3g)" % (tag, (~sure).sum(), len(lens), gaps.min()))
        assert 4 * (~sure).sum() <= len(lens), tag
        np.testing.assert_array_equal(st[sure], rst[sure], err_msg=tag)
        np.testing.assert_array_equal(sp[sure], rsp[sure], err_msg=tag)


def _random_labels(rng, B, Cc, blank, maxL, lo=0):
    nonblank = [c for c in range(Cc) if c != blank]
    return [[int(k) for k in rng.choice(nonblank, int(rng.integers(lo, maxL + 1)))] for _ in range(B)]


# ---- 1. parity at small shapes ----
def test_small_ragged_with_every_kind_of_row(gpu):
    rng = np.random.default_rng(0)
    B, T, Cc, maxL, blank = 8, 12, 5, 4, 2
    labels = [[], [3], [1, 1, 4], [0, 3, 3, 1], [4, 0, 1], [1, 1, 1, 1], [3, 4], [0, 1, 3, 4]]
    lens = [9, 12, 10, 5, 0, 6, 11, 4]            # row 3 at its minimum (5), row 5 infeasible (needs 7), row 4 without frames, row 7 at 4
    p = _softmax(rng, B, T, Cc)
    for b in range(B):
        p[b, lens[b]:] = np.nan
    ref = _reference(p, lens, labels, blank, maxL)
    assert np.isneginf(ref[2][[4, 5]]).all() and np.isfinite(ref[2][[0, 1, 2, 3, 6, 7]]).all()
    _check("small", _run(gpu, p, lens, labels, blank, maxL), ref, lens, labels, blank)


def test_random_softmax_batch(gpu):
    rng = np.random.default_rng(0)
    B, T, Cc, maxL, blank = 64, 60, 29, 12, 0
    labels = _random_labels(rng, B, Cc, blank, maxL)
    lens = [int(n) for n in rng.integers(30, T + 1, B)]
    p = _softmax(rng, B, T, Cc)
    for b in range(B):
        p[b, lens[b]:] = np.nan
    _check("random", _run(gpu, p, lens, labels, blank, maxL), _reference(p, lens, labels, blank, maxL), lens, labels, blank)


def test_long_free_paths(gpu):
    """T = 300, L <= 140 (the two-states-per-lane instantiation) on random softmax outputs: with 84000 decisions a row, some rows have a
    decision closer than the threshold; they stay under the cap"""
    rng = np.random.default_rng(0)
    B, T, Cc, maxL, blank = 16, 300, 29, 140, 0
    labels = _random_labels(rng, B, Cc, blank, maxL)
    lens = [max(_min_len(l), int(n)) for l, n in zip(labels, rng.integers(150, T + 1, B))]
    p = _softmax(rng, B, T, Cc)
    for b in range(B):
        p[b, lens[b]:] = np.nan
    _check("long", _run(gpu, p, lens, labels, blank, maxL), _reference(p, lens, labels, blank, maxL), lens, labels, blank)


# ---- 2. one case per instantiation ----
# B = 3, T = 2 max_label_len + 8, every state of the widest row in use.  With T * Smax decisions a row (a million at 520) random
# inputs leave no row whose every decision clears the threshold, and B = 3 allows none to be left out.  So each row gets only two or
# three frames more than its shortest alignment (a state is then reachable in a few frames only and the decisions between two finite
# candidates are a few thousand), the logit scale is 6, and the seeds are those found, with the reference alone, to leave every row in
# the exact comparison.  test_long_free_paths above is the case with long unconstrained paths.
NJ_SEED = {4: 0, 130: 0, 300: 1, 520: 116}


@functools.lru_cache(None)
def _nj_case(maxL):
    rng = np.random.default_rng(NJ_SEED[maxL])
    B, Cc, blank, T = 3, 29, 28, 2 * maxL + 8
    labels = [[int(rng.integers(0, 28))] * maxL,                                    # full length, every label doubled: no skip anywhere
              _random_labels(rng, 1, Cc, blank, maxL, lo=maxL)[0],                  # full length, random
              _random_labels(rng, 1, Cc, blank, maxL // 2, lo=maxL // 2)[0]]
    lens = [_min_len(labels[0]) + 3, _min_len(labels[1]) + 2, _min_len(labels[2]) + 2]
    assert max(lens) <= T
    p = _softmax(rng, B, T, Cc, scale=6.0)
    for b in range(B):
        p[b, lens[b]:] = np.nan
    return p, lens, labels, blank, _reference(p, lens, labels, blank, maxL)


@pytest.mark.parametrize("maxL", sorted(NJ_SEED))
def test_each_instantiation(gpu, maxL):
    p, lens, labels, blank, ref = _nj_case(maxL)
    assert len(labels[0]) == len(labels[1]) == maxL and np.isfinite(ref[2]).all()
    _check("maxL %d" % maxL, _run(gpu, p, lens, labels, blank, maxL), ref, lens, labels, blank)


def test_the_largest_label_length_is_accepted(gpu):
    rng = np.random.default_rng(0)
    maxL, T, Cc, blank = 4000, 4010, 6, 0
    lab = [1]
    for r in rng.integers(1, Cc - 1, maxL - 1):                                     # no adjacent repeats: 4000 labels fit 4010 frames
        lab.append(1 + (lab[-1] - 1 + int(r)) % (Cc - 1))
    assert _min_len(lab) == maxL and min(lab) >= 1 and max(lab) < Cc
    p = _softmax(rng, 1, T, Cc, scale=1.0)
    ref = _reference(p, [T], [lab], blank, maxL, want_gap=False)
    assert np.isfinite(ref[2][0])
    _check("maxL 4000", _run(gpu, p, [T], [lab], blank, maxL), ref, [T], [lab], blank, exact=False)


# ---- 4. the tie-break rule, exactly ----
def test_tie_break_on_flat_probabilities(gpu):
    Cc, blank = 4, 0
    sets = [[], [2], [1, 2, 3], [3, 3]]
    labels, lens = [], []
    for lab in sets:
        for extra in range(6):
            labels.append(lab)
            lens.append(_min_len(lab) + extra)
    B, T = len(labels), max(lens)
    p = np.full((B, T, Cc), 0.25, np.float32)
    ref = _reference(p, lens, labels, blank, 3)
    assert np.isfinite(ref[2]).all()
    st, sp, sc = _run(gpu, p, lens, labels, blank, 3)
    np.testing.assert_array_equal(st, ref[0])
    np.testing.assert_array_equal(sp, ref[1])
    np.testing.assert_allclose(sc, np.asarray(lens) * np.log(0.25), rtol=2.0 ** -23, atol=0)     # every product is exact


# ---- 5. against code we already trust ----
def test_against_the_loss(gpu):
    rng = np.random.default_rng(5)
    B, T, Cc, maxL, blank = 16, 40, 9, 10, 8
    labels = _random_labels(rng, B, Cc, blank, maxL, lo=1)
    labels[3] = [2, 2, 5, 5, 5, 1]
    lens = [int(n) for n in rng.integers(25, T + 1, B)]
    unique = [0, 3, 7, 12]                                                          # input length = minimum: exactly one alignment
    for b in unique:
        lens[b] = _min_len(labels[b])
    p = _softmax(rng, B, T, Cc)
    lab, ll = _pad(labels, maxL)
    loss, _ = NL.ctc_loss_device(torch.from_numpy(p).to(gpu), lab, ll, np.asarray(lens, np.int32), blank, want_grad=False)
    st, sp, sc = _run(gpu, p, lens, labels, blank, maxL)
    nll = -loss.cpu().numpy().astype(np.float64)
    assert np.isfinite(nll).all() and np.isfinite(sc).all()
    tol = _tol(np.asarray(lens), nll)
    for b in range(B):
        _assert_valid("row %d" % b, st[b], sp[b], sc[b], lens[b], labels[b], blank)
        if b in unique:
            assert abs(sc[b] - nll[b]) <= tol[b], (b, sc[b], nll[b], tol[b])
        else:
            assert sc[b] <= nll[b] + tol[b], (b, sc[b], nll[b], tol[b])
    assert (sc < nll - 0.01).any()                                                  # ... and a sum over alignments is more than its largest term


def test_aligning_the_greedy_labels_gives_the_argmax_path(gpu):
    rng = np.random.default_rng(8)
    T, Cc, blank = 50, 7, 2
    base = [2, 2, 1, 1, 1, 2, 1, 3, 3, 2, 2, 3, 4, 4, 4, 4, 5, 2, 5, 5, 6, 0, 0, 2, 0, 1, 6, 6, 2, 2]
    paths = [(base + base)[:T], [int(k) for k in rng.integers(0, Cc, T)], (base[::-1] + base)[:T], [blank] * T, (base + base)[3:3 + T]]
    lens = [50, 37, 0, 50, 41]
    p = rng.uniform(0.0, 0.1, (len(paths), T, Cc)).astype(np.float32)               # (the posteriors of test_gpu_ctc.py's greedy case)
    for b, path in enumerate(paths):
        for t, k in enumerate(path):
            p[b, t, k] = 0.5 + 0.01 * ((t * 7 + b) % 9)
    dp = torch.from_numpy(p).to(gpu)
    out, n = NL.ctc_greedy_decode_device(dp, lens, blank)
    out, n = out.cpu().numpy(), n.cpu().numpy()
    labels = [[int(k) for k in out[b, :n[b]]] for b in range(len(paths))]
    maxL = int(n.max())
    st, sp, sc = _run(gpu, p, lens, labels, blank, maxL)
    for b, path in enumerate(paths):
        _assert_valid("row %d" % b, st[b], sp[b], sc[b], lens[b], labels[b], blank)
        cls = [blank if s % 2 == 0 else labels[b][s // 2] for s in st[b, :lens[b]]]
        assert cls == path[:lens[b]], b
        want = np.log(p[b, np.arange(lens[b]), path[:lens[b]]].astype(np.float64)).sum()
        assert abs(sc[b] - want) <= _tol(lens[b], want), b


# ---- 6. range ----
def test_a_path_probability_near_1e_minus_1200(gpu):
    rng = np.random.default_rng(6)
    T, Cc, blank = 2000, 4, 0
    p = (0.25 + rng.uniform(-0.02, 0.02, (1, T, Cc))).astype(np.float32)
    p /= p.sum(-1, keepdims=True)
    labels = [[1, 2, 2, 3, 1]]
    ref = _reference(p, [T], labels, blank, 5)
    assert -2900 < ref[2][0] < -2600
    got = _run(gpu, p, [T], labels, blank, 5)
    assert np.isfinite(got[2][0])
    _check("range", got, ref, [T], labels, blank, exact=False)


# ---- 7. zeros ----
def test_zeros_force_the_path_or_forbid_it(gpu):
    rng = np.random.default_rng(7)
    B, T, Cc, blank = 4, 10, 5, 0
    labels = [[2], [2, 3], [1, 2], [4]]
    lens = [10, 10, 8, 10]
    p = _softmax(rng, B, T, Cc, scale=1.0)
    p[0, :, 2] = 0.05
    p[0, 4, 2] = 0.9                     # row 0 wants its label at frame 4 ...
    ref_before = _reference(p, lens, labels, blank, 2)
    assert ref_before[0][0, 4] == 1
    p[0, 4, 2] = 0.0                     # ... and may not have it there
    p[1, 3, 0] = 0.0                     # a frame without a blank
    p[2, 5, :] = 0.0                     # zeros on every path
    p[3, :, 4] = 0.0                     # the label never possible
    ref = _reference(p, lens, labels, blank, 2)
    assert ref[0][0, 4] != 1 and np.isfinite(ref[2][:2]).all() and np.isneginf(ref[2][2:]).all()
    got = _run(gpu, p, lens, labels, blank, 2)
    _check("zeros", got, ref, lens, labels, blank)
    assert (got[0][2:] == -1).all() and (got[1][2:] == -1).all() and np.isneginf(got[2][2:]).all()


# ---- 8. determinism ----
def test_bits_do_not_depend_on_the_call_the_batch_or_the_instantiation(gpu):
    for base, others in ((4, (130, 300, 520)), (130, (300, 520))):
        p, lens, labels, blank, _ = _nj_case(base)
        a = _run(gpu, p, lens, labels, blank, base)
        again = _run(gpu, p, lens, labels, blank, base)
        for x, y in zip(a, again):
            assert x.tobytes() == y.tobytes(), base
        for r in range(len(lens)):
            alone = _run(gpu, p[r:r + 1], lens[r:r + 1], labels[r:r + 1], blank, base)
            for x, y in zip(a, alone):
                assert x[r].tobytes() == y[0].tobytes(), (base, r)
        for m in others:                                                            # the same rows, padded into the other branches
            wide = _run(gpu, p, lens, labels, blank, m)
            assert wide[0].tobytes() == a[0].tobytes() and wide[2].tobytes() == a[2].tobytes(), (base, m)
            np.testing.assert_array_equal(wide[1][:, :base], a[1], err_msg=str((base, m)))
            assert (wide[1][:, base:] == -1).all(), (base, m)


# ---- 9. forms ----
def test_forms(gpu):
    rng = np.random.default_rng(9)
    B, T, Cc, maxL, blank = 5, 30, 11, 6, 10
    labels = _random_labels(rng, B, Cc, blank, maxL)
    lens = [30, 22, 30, 17, 29]
    p = _softmax(rng, B, T, Cc)
    lab, ll = _pad(labels, maxL)
    il = np.asarray(lens, np.int32)
    want = _run(gpu, p, lens, labels, blank, maxL)
    host = NL.ctc_align(p, lab, ll, il, blank)
    for x, y in zip(want, host):
        assert x.tobytes() == y.tobytes()
    L = capi.load()
    dp = torch.from_numpy(p).to(gpu)
    need = L.nntk_ctc_align_workspace_floats(B, T, maxL)
    ws = torch.empty(need + 4, dtype=torch.float32, device=gpu)
    st = torch.full((B, T), 7, dtype=torch.int32, device=gpu)
    sp = torch.full((B, maxL, 2), 7, dtype=torch.int32, device=gpu)
    sc = torch.full((B,), 7.0, dtype=torch.float32, device=gpu)
    out = NL.ctc_align_device(dp, lab, ll, il, blank, states=st, spans=sp, scores=sc, workspace=ws[:need])
    torch.cuda.synchronize()
    assert out[0] is st and out[1] is sp and out[2] is sc
    for x, y in zip(want, (st, sp, sc)):
        assert x.tobytes() == y.cpu().numpy().tobytes()
    ip = lambda a: a.ctypes.data_as(capi.ip)
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(st_, sp_, sc_, ws_):
        return L.nntk_ctc_align_device(vp(dp), B, T, Cc, ip(il), ip(lab), ip(ll), maxL, blank, vp(st_), vp(sp_), vp(sc_), vp(ws_))

    for drop in ("states", "spans", "both"):
        st.fill_(7); sp.fill_(7); sc.fill_(7.0)
        assert call(None if drop != "spans" else st, None if drop != "states" else sp, sc, ws) == 0, capi.last_error()
        torch.cuda.synchronize()
        assert want[2].tobytes() == sc.cpu().numpy().tobytes(), drop
        if drop == "states":
            assert (st == 7).all() and want[1].tobytes() == sp.cpu().numpy().tobytes()
        elif drop == "spans":
            assert (sp == 7).all() and want[0].tobytes() == st.cpu().numpy().tobytes()
    st.fill_(7); sp.fill_(7); sc.fill_(7.0)
    assert call(st, sp, sc, ws[1:]) == -1 and "16-byte" in capi.last_error()
    assert call(st, sp, None, ws) == -1 and capi.last_error() != ""
    torch.cuda.synchronize()
    assert (st == 7).all() and (sp == 7).all() and (sc == 7.0).all()
