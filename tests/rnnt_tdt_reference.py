"""What the token-and-duration transducer tests compare the library with (a helper, no test): the loss and its gradient in float64
numpy, in log space; the same recursion in torch with autograd (float64 pins the numpy gradient, float32 is the device tests' error
yardstick); enumeration of every path of a tiny lattice; the cases of the device tests.  x [B][T][U1][V + D], the D = len(durs)
duration scores last; row b has lens[b] frames and the labels labels[b]; cells with t >= T_b or u > U_b are padding."""
import math

import numpy as np

import rnnt_cases as K
from rnnt_reference import log_softmax

NINF = -math.inf


def _lse(v):
    v = [a for a in v if a > NINF]
    return max(v) + math.log(sum(math.exp(a - max(v)) for a in v)) if v else NINF


def moves(T, U, durs, t, u):
    """the moves out of (t, u): (duration index, is a label, t', u'); a blank lands on T only from u = U, a label never does"""
    for i, d in enumerate(durs):
        if d > 0 and (t + d < T or (t + d == T and u == U)):
            yield i, False, t + d, u
        if u < U and t + d < T:
            yield i, True, t + d, u + 1


def tdt_row(x, lab, blank, durs, sigma=0.0, enumerate_paths=False):
    """float64, one row's live cells x [T][U + 1][V + D] -> (loss, gradient); no path: (inf, zeros).  enumerate_paths: the loss by a
    walk over every single path instead (tiny lattices only), gradient None"""
    T, U, V = x.shape[0], len(lab), x.shape[2] - len(durs)
    lt, ld = log_softmax(x[..., :V]), log_softmax(x[..., V:])
    w = lambda t, u, i, y: lt[t, u, lab[u] if y else blank] - sigma + ld[t, u, i]      # the log mass of a move
    if enumerate_paths:
        walk = lambda t, u, lp: math.exp(lp) if (t, u) == (T, U) else sum(walk(t2, u2, lp + w(t, u, i, y)) for i, y, t2, u2 in moves(T, U, durs, t, u))
        total = walk(0, 0, 0.0)
        return (-math.log(total) if total > 0.0 else math.inf), None
    into = [[[] for _ in range(U + 1)] for _ in range(T + 1)]              # what arrives at a cell, move by move
    alpha, beta = np.full((T + 1, U + 1), NINF), np.full((T + 1, U + 1), NINF)
    for t in range(T):
        for u in range(U + 1):                                              # a source's targets come later in this order
            alpha[t, u] = _lse(into[t][u]) if t + u else 0.0
            for i, y, t2, u2 in moves(T, U, durs, t, u):
                into[t2][u2].append(alpha[t, u] + w(t, u, i, y))
    logp, g = _lse(into[T][U]), np.zeros(x.shape)
    if logp == NINF:
        return math.inf, g
    beta[T, U] = 0.0
    for t in range(T - 1, -1, -1):
        for u in range(U, -1, -1):
            beta[t, u] = _lse([w(t, u, i, y) + beta[t2, u2] for i, y, t2, u2 in moves(T, U, durs, t, u)])
    assert abs(logp - beta[0, 0]) <= 1e-9 * max(1.0, abs(logp))
    occ = np.exp(alpha[:T] + beta[:T] - logp)[:, :, None]
    g[..., :V], g[..., V:] = occ * np.exp(lt), occ * np.exp(ld)
    for t in range(T):
        for u in range(U + 1):
            for i, y, t2, u2 in moves(T, U, durs, t, u):
                f = math.exp(alpha[t, u] + w(t, u, i, y) + beta[t2, u2] - logp)
                g[t, u, lab[u] if y else blank] -= f
                g[t, u, V + i] -= f
    return -logp, g


def torch_row(x, lab, blank, durs, sigma):
    """the loss of one row as a 0-dim tensor at x's precision, plain logsumexp over a cell's terms; None for a row without a path"""
    import torch
    T, U, V = x.shape[0], len(lab), x.shape[2] - len(durs)
    lt, ld = torch.log_softmax(x[..., :V], -1) - sigma, torch.log_softmax(x[..., V:], -1)
    into = [[[] for _ in range(U + 1)] for _ in range(T + 1)]
    for t in range(T):
        for u in range(U + 1):
            if t + u and not into[t][u]:
                continue
            a = torch.logsumexp(torch.stack(into[t][u]), 0) if t + u else torch.zeros((), dtype=x.dtype)
            for i, y, t2, u2 in moves(T, U, durs, t, u):
                into[t2][u2].append(a + lt[t, u, lab[u] if y else blank] + ld[t, u, i])
    return -torch.logsumexp(torch.stack(into[T][U]), 0) if into[T][U] else None


def _rows(x, labels, lens, fn):
    loss, grad = np.zeros(x.shape[0]), np.zeros(x.shape)
    for b in range(x.shape[0]):
        Tb, Ub = int(lens[b]), len(labels[b])
        loss[b], grad[b, :Tb, :Ub + 1] = fn(x[b, :Tb, :Ub + 1], list(labels[b]))
    return loss, grad


def tdt_loss_and_grad(x, labels, lens, durs, blank, sigma=0.0):
    """float64: (loss rows [B], gradient [B][T][U1][V + D], exact zeros in the padding, which is never looked at)"""
    return _rows(np.asarray(x, np.float64), labels, lens, lambda r, lab: tdt_row(r, lab, blank, durs, sigma))


def torch_tdt(x, labels, lens, durations, blank, sigma, dtype):
    """the same in torch on the CPU at `dtype`, differentiated by autograd -> (loss rows, gradient) as float64 numpy"""
    import torch

    def row(r, lab):
        t = torch.from_numpy(np.ascontiguousarray(r)).to(dtype).requires_grad_(True)
        l = torch_row(t, lab, blank, durations, sigma)
        return (math.inf, 0.0) if l is None else (float(l.detach()), torch.autograd.grad(l, t)[0].double().numpy())

    return _rows(x, labels, lens, row)


def case(name):
    """a case of tests/test_gpu_rnnt_tdt.py: dict(x, labels, lens, durs, blank, sigma, inf = the rows without a path)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    mk = lambda shape, labels, lens, durs, blank=0, sigma=0.0, inf=(): dict(
        x=rng.uniform(-3, 3, shape).astype(np.float32), labels=labels, lens=lens, durs=durs, blank=blank, sigma=sigma, inf=list(inf))
    lab = lambda n, V, blank=0: K.labels(rng, n, V, blank)
    if name.startswith("ragged"):                    # the lengths of rnnt_cases.ragged: T = 7 with (7, 4, 1), label lengths (3, 0, 5); D = 5
        V, blank, sigma = (float(v) for v in name.split("_")[1:])
        c = K.ragged(int(V), int(blank))
        return mk((3, 7, 6, int(V) + 5), c["labels"], c["lens"], [0, 1, 2, 3, 4], int(blank), sigma)
    if name == "d12":
        return mk((1, 6, 4, 6), [lab(3, 4)], [6], [1, 2])
    if name == "d12_short":                          # three labels, each a frame at least, in two frames
        return mk((1, 2, 4, 6), [lab(3, 4)], [2], [1, 2], inf=[0])
    if name == "d02":                                # parity: {0, 2} reaches T_b = 4 and not 3
        return mk((2, 4, 2, 6), [[1], [2]], [4, 3], [0, 2], inf=[1])
    if name == "d018":                               # a ring deeper than most diagonals are wide; 8 never usable in the row of 3 frames
        return mk((2, 20, 4, 7), [lab(3, 4), [1, 3]], [20, 3], [0, 1, 8])
    if name == "T300":
        return mk((1, 300, 3, 7), [[1, 1]], [300], [0, 1, 2, 4])
    if name == "U300":
        return mk((2, 5, 301, 6), [lab(300, 3, 1), [0, 2]], [5, 3], [0, 1, 2], blank=1)
    if name == "U512":                               # the general form with the LDS opt-in at Dmax = 4
        return mk((2, 3, 513, 6), [lab(512, 3), [1]], [3, 2], [0, 1, 4])
    if name == "underflow":
        # V = 8: blank 0, labels 1..4, class 7 takes the token mass everywhere; durations {0, 1, 2}.  Off the path every needed token lies
        # 200 below class 7; on it the needed token equals it, except in two cells where it lies 120 below; in two other cells of the
        # path the needed duration lies 150 below the other two
        T, U, labs = 6, 4, [1, 2, 2, 4]
        c = mk((1, T, U + 1, 11), [labs], [T], [0, 1, 2])
        c["x"][..., :8] -= 200.0
        c["x"][..., 7] = 0.0
        t = u = 0
        for k, (y, i) in enumerate([(1, 0), (0, 1), (1, 1), (0, 2), (1, 0), (1, 1), (0, 1)]):
            c["x"][0, t, u, labs[u] if y else 0] = -120.0 if k in (2, 5) else 0.0
            if k in (1, 4):
                c["x"][0, t, u, 8:] = 0.0
                c["x"][0, t, u, 8 + i] = -150.0
            t, u = t + c["durs"][i], u + y
        assert (t, u) == (T, U)
        return c
    raise KeyError(name)


CASES = ["ragged_5_0_0", "ragged_5_4_0", "ragged_64_63_0", "ragged_257_100_0", "ragged_7_3_0", "ragged_5_2_0.05", "d12", "d12_short", "d02",
         "d018", "T300", "U300", "U512", "underflow"]
