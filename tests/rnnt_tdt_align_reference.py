"""What the token-and-duration forced-alignment tests compare the library with (a helper, no test): the Viterbi path over the lattice of
rnnt_tdt_reference with the contract's tie-break, in float64 and, as the device tests' yardstick, on a float32 torch log_softmax with
float32 adds; enumeration of every path of a tiny lattice; the aligner's own cases."""
import functools
import math

import numpy as np

import rnnt_tdt_reference as R
from rnnt_reference import log_softmax

NINF = -math.inf


def _arrays(path, T, U, durs, w):
    """the moves (t, u, i, is a label) of a path -> the four int arrays and the two logp arrays of the contract"""
    r = dict(label_frames=np.full(U, -1), label_durations=np.full(U, -1), frame_labels=np.full(T, -1), frame_durations=np.full(T, -1),
             label_logp=np.zeros(U), frame_logp=np.zeros(T))
    for t, u, i, y in path:
        k, at, to = ("label", u, t) if y else ("frame", t, u)
        r[k + ("_frames" if y else "_labels")][at], r[k + "_durations"][at], r[k + "_logp"][at] = to, durs[i], w(t, u, i, y)
    return r


def viterbi_row(lt, ld, lab, blank, durs):
    """lt [T][U + 1][V] / ld [T][U + 1][D]: the log-probabilities of one row's live cells (sigma already taken off lt), of any float
    type: every add stays in it -> dict(score, gap, the six arrays).  gap: the smallest winner minus runner-up over the decisions with at
    least two finite candidates.  No path: score -inf, the int arrays -1, the logp arrays 0"""
    T, U = lt.shape[0], len(lab)
    w = lambda t, u, i, y: lt[t, u, lab[u] if y else blank] + ld[t, u, i]
    v, back, gap = {(0, 0): lt.dtype.type(0)}, {}, math.inf
    for t, u in [(t, u) for t in range(T) for u in range(U + 1)][1:] + [(T, U)]:
        cands = []
        for i, d in enumerate(durs):                                         # the loss's one order
            if t - d >= 0 and d > 0:
                cands.append((v[t - d, u] + w(t - d, u, i, False), (t - d, u, i, False)))
            if t - d >= 0 and u >= 1 and t < T:
                cands.append((v[t - d, u - 1] + w(t - d, u - 1, i, True), (t - d, u - 1, i, True)))
        best = NINF
        for c, move in cands:
            if c > best:
                best, back[t, u] = c, move
        finite = sorted(float(c) for c, _ in cands if c > NINF)
        if len(finite) >= 2:
            gap = min(gap, finite[-1] - finite[-2])
        v[t, u] = lt.dtype.type(best)
    path, at = [], (T, U)
    while at in back:
        path.append(back[at])
        at = back[at][:2]
    return dict(_arrays(path if v[T, U] > NINF else [], T, U, durs, w), score=float(v[T, U]), gap=gap)


def enumerate_row(lt, ld, lab, blank, durs):
    """every path by enumeration -> the best one's arrays and score; among paths of exactly equal score the one whose moves, read from
    the LAST backwards, come first in the order (duration index, blank before label): what the recursion's tie-break selects"""
    T, U = lt.shape[0], len(lab)
    w = lambda t, u, i, y: lt[t, u, lab[u] if y else blank] + ld[t, u, i]
    paths = []

    def walk(t, u, lp, path):
        if (t, u) == (T, U):
            paths.append((lp, path))
        for i, y, t2, u2 in R.moves(T, U, durs, t, u):
            walk(t2, u2, lp + w(t, u, i, y), path + [(t, u, i, y)])

    walk(0, 0, 0.0, [])
    best = max((p[0] for p in paths), default=NINF)
    tied = [p[1] for p in paths if p[0] == best and best > NINF]
    path = min(tied, key=lambda p: [(i, y) for _, _, i, y in reversed(p)]) if tied else []
    return dict(_arrays(path, T, U, durs, w), score=best)


def rows(c, dtype=np.float64, fn=viterbi_row):
    """fn on every row of a case, at `dtype`: float64 numpy log_softmax, or float32 through torch's"""
    import torch
    ls = log_softmax if dtype == np.float64 else lambda a: torch.log_softmax(torch.from_numpy(np.ascontiguousarray(a)), -1).numpy()
    out, V = [], c["x"].shape[3] - len(c["durs"])
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):
        x = c["x"][b, :n, :len(lab) + 1].astype(dtype)
        out.append(fn(ls(x[..., :V]) - dtype(c["sigma"]), ls(x[..., V:]), list(lab), c["blank"], c["durs"]))
    return out


def gap_threshold(Tb, Ub):
    """the classic aligner's threshold (rnnt_align_reference.gap_threshold), doubled because a move is two products"""
    return 16 * (Tb + Ub + 2) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def case(name):
    """the cases of rnnt_tdt_reference.case and the aligner's own ("Token-and-duration forced alignment", says why each seed
    and scale): `long`, `blocks`, `flat`; test_rnnt_tdt_align_host.py asserts their rows' gaps"""
    mk = lambda x, labels, durs: dict(x=x.astype(np.float32), labels=labels, lens=[x.shape[1]], durs=durs, blank=0, sigma=0.0, inf=[])
    if name == "long":
        return mk(np.random.default_rng(3).uniform(-3, 3, (1, 300, 3, 7)), [[1, 1]], [0, 1, 2, 4])
    if name == "blocks":
        rng = np.random.default_rng(2)
        return mk(rng.uniform(-600, 600, (1, 300, 300, 6)), [rng.integers(1, 3, 299).tolist()], [0, 1, 2])
    if name == "flat":
        return mk(np.zeros((1, 3, 3, 6)), [[1, 2]], [0, 1, 2])
    return R.case(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(the float64 rows, the float32 scores) of a case, computed once"""
    return rows(case(name)), [r["score"] for r in rows(case(name), np.float32)]
