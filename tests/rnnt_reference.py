"""What the transducer tests compare the library with (a helper, no test): the RNN-Transducer loss and its gradient with respect to
the unnormalised scores in float64 numpy, in log space; the same recursion in torch at a chosen precision, differentiated by autograd
(float64: a second, independent statement of the gradient; float32: the error a careful float32 implementation has, which sets the
tolerance of the device tests); brute-force enumeration of every alignment for tiny lattices; the joiner and its backward in float64.
Both lattices (lattice64, torch_lattice) are the only ones the transducer loss tests have -- tests/rnnt_pruned_reference.py runs its simple
and banded losses through them -- and both survive -inf scores: a term that is -inf is absent, a row without a path is (inf, zeros).

Conventions: logits [B][T][U1][V], U1 = max_label_len + 1; row b has T_b = lens[b] frames and the labels labels[b] (U_b of them);
cells with t >= T_b or u > U_b are padding."""
import math

import numpy as np


def log_softmax(x):
    """over the last axis; a -inf score stays -inf, and a row whose scores are all -inf comes out all -inf (never NaN)"""
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    dead = m == -math.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        ms = np.where(dead, 0.0, m)
        r = x - ms - np.log(np.exp(x - ms).sum(-1, keepdims=True))
    return np.where(dead, -math.inf, r)


def _lae(a, b):
    if a == -math.inf:
        return b
    if b == -math.inf:
        return a
    m = max(a, b)
    return m + math.log1p(math.exp(-abs(a - b)))


def lattice64(lp, lab, blank, factored=False):
    """The one float64 statement of the lattice, for the stored, the simple and the banded loss.  lp [T][U + 1][V] float64
    log-probabilities of one row's live cells; -inf stands for a zero emission: a score that is -inf, every score of a cell whose scores
    are all -inf, every score of a cell that does not exist (outside a band).  A term that is -inf is absent from every sum (_lae), so
    nothing ever computes inf - inf.  -> (loss, d loss / d scores [T][U + 1][V], occupancy [T][U + 1]); no path: (inf, zeros, zeros).
    factored: the gradient's first term as occupancy x exp(lp), two roundings, as tests/rnnt_pruned_reference.py has always formed it;
    else as one exponential of the sum, as this module has: each caller keeps the float64 bits it had before the two shared a lattice"""
    T, U1, V = lp.shape
    U = U1 - 1
    ninf = -math.inf
    lb = lp[:, :, blank]
    ly = np.full((T, U1), ninf)
    for u in range(U):
        ly[:, u] = lp[:, u, lab[u]]
    alpha = np.full((T, U1), ninf)
    beta = np.full((T + 1, U1 + 1), ninf)
    for t in range(T):
        for u in range(U1):
            if t == 0 and u == 0:
                alpha[0, 0] = 0.0
                continue
            a = alpha[t - 1, u] + lb[t - 1, u] if t > 0 else ninf
            c = alpha[t, u - 1] + ly[t, u - 1] if u > 0 else ninf
            alpha[t, u] = _lae(a, c)
    beta[T, U] = 0.0                                    # stands for 1 in the blank term of the last cell
    for t in range(T - 1, -1, -1):
        for u in range(U, -1, -1):
            beta[t, u] = _lae(lb[t, u] + beta[t + 1, u], ly[t, u] + beta[t, u + 1])
    logp = alpha[T - 1, U] + lb[T - 1, U]
    if logp == ninf:
        return math.inf, np.zeros((T, U1, V)), np.zeros((T, U1))
    assert abs(logp - beta[0, 0]) <= 1e-9 * max(1.0, abs(logp))
    # alpha / P ( p_v beta(t,u) - [v = blank] p_blank beta(t+1,u) - [v = y_{u+1}] p_y beta(t,u+1) ); every argument is a sum of
    # finite values and -inf, and logp is finite: -inf at the worst, a factor of exactly 0
    w = alpha + beta[:T, :U1] - logp
    occ = np.exp(w)
    g = occ[:, :, None] * np.exp(lp) if factored else np.exp(w[:, :, None] + lp)
    g[:, :, blank] -= np.exp(alpha + lb + beta[1:, :U1] - logp)
    for u in range(U):
        g[:, u, lab[u]] -= np.exp(alpha[:, u] + ly[:, u] + beta[:T, u + 1] - logp)
    return -logp, g, occ


def _row(lp, lab, blank):
    """(loss, gradient) of lattice64, for the callers that have no use for the occupancies"""
    return lattice64(lp, lab, blank)[:2]


def rnnt_loss_and_grad(logits, labels, lens, blank):
    """float64: (loss rows [B], gradient [B][T][U1][V], exact zeros in the padding); padding logits are never looked at.  A row
    without a path (P = 0, possible only through -inf scores): loss inf, gradient zeros"""
    B, T, U1, V = logits.shape
    loss, grad = np.zeros(B), np.zeros((B, T, U1, V))
    for b in range(B):
        Tb, Ub = int(lens[b]), len(labels[b])
        loss[b], grad[b, :Tb, :Ub + 1] = _row(log_softmax(logits[b, :Tb, :Ub + 1]), list(labels[b]), blank)
    return loss, grad


def brute_force_loss(logits_row, lab, blank):
    """-log of the summed probability of every alignment of one row [T][U + 1][V], by enumeration (tiny lattices only); inf for a
    zero total"""
    lp = log_softmax(logits_row)
    T, U = lp.shape[0], len(lab)
    total = [0.0]

    def walk(t, u, logp):
        if u < U:
            walk(t, u + 1, logp + lp[t, u, lab[u]])
        if t + 1 < T:
            walk(t + 1, u, logp + lp[t, u, blank])
        elif u == U:
            total[0] += math.exp(logp + lp[t, u, blank])

    walk(0, 0, 0.0)
    return -math.log(total[0]) if total[0] > 0.0 else math.inf


def _tlae(a, b):
    """logaddexp of two torch vectors in which a term that is -inf is absent: which terms are is decided on the detached values, and
    an absent term takes no part in the graph (it is replaced by a constant before logaddexp sees it, and selected away after)"""
    import torch
    na, nb = a.detach() == -math.inf, b.detach() == -math.inf
    if not bool((na | nb).any()):
        return torch.logaddexp(a, b)
    zero = torch.zeros((), dtype=a.dtype)
    both = torch.logaddexp(torch.where(na, zero, a), torch.where(nb, zero, b))
    return torch.where(na, b, torch.where(nb, a, both))


def torch_lattice(x, lab, blank, mask=None):
    """The one torch statement of the lattice, at x's precision, anti-diagonal by anti-diagonal.  x [T][U + 1][V]: the scores of one
    row's live cells, a tensor of any float type, a leaf or not; mask [T][U + 1] bool numpy or None: the cells that exist.  A cell whose
    scores are all -inf counts as one that does not exist: two zero emissions, and its scores take no part in the graph.
    -> (loss, lp): the 0-dim loss, or None for a row without a path (nothing to differentiate); lp = log_softmax(x) with its gradient
    retained where x asks for one, for the occupancies"""
    import torch
    T, U1, _ = x.shape
    U = U1 - 1
    exists = (x.detach() > -math.inf).any(-1)
    if mask is not None:
        exists &= torch.from_numpy(np.ascontiguousarray(mask))
    part = not bool(exists.all())
    if part:
        x = torch.where(exists[:, :, None], x, torch.zeros((), dtype=x.dtype))
    lp = torch.log_softmax(x, -1)
    if lp.requires_grad:
        lp.retain_grad()
    lb = lp[:, :, blank]
    ly = lp[:, :U, :].gather(2, torch.tensor(lab, dtype=torch.long).view(1, U, 1).expand(T, U, 1)).squeeze(2) if U else None
    if part:
        ninf = torch.full((), -math.inf, dtype=x.dtype)
        lb = torch.where(exists, lb, ninf)
        ly = torch.where(exists[:, :U], ly, ninf) if U else None
    lo_prev, prev = 0, torch.zeros(1, dtype=x.dtype)
    for n in range(1, T + U):
        lo, hi = max(0, n - T + 1), min(U, n)
        parts = []
        # u in [lo, min(hi, n - 1)] is reached from (t - 1, u); u in [max(lo, 1), hi] from (t, u - 1)
        t_hi, u_lo = min(hi, n - 1), max(lo, 1)
        ft = fu = None
        if t_hi >= lo:
            u = torch.arange(lo, t_hi + 1)
            ft = prev[u - lo_prev] + lb[n - 1 - u, u]
        if hi >= u_lo:
            u = torch.arange(u_lo, hi + 1)
            fu = prev[u - 1 - lo_prev] + ly[n - u, u - 1]
        if lo == 0:
            parts.append(ft[:1])
        o_lo, o_hi = u_lo, t_hi                           # where both arrive
        if o_hi >= o_lo:
            parts.append(_tlae(ft[o_lo - lo:o_hi - lo + 1], fu[:o_hi - u_lo + 1]))
        if hi == n:
            parts.append(fu[-1:])
        lo_prev, prev = lo, torch.cat(parts)
    assert lo_prev == U and prev.shape[0] == 1
    logp = prev[0] + lb[T - 1, U]
    return (None if float(logp.detach()) == -math.inf else -logp), lp


def torch_rnnt(logits, labels, lens, blank, dtype):
    """the same loss in torch on the CPU at `dtype`, differentiated by autograd -> (loss rows, gradient) as float64 numpy; a row without
    a path: (inf, zeros), and backward is not called"""
    import torch
    B, T, U1, V = logits.shape
    loss, grad = np.zeros(B), np.zeros((B, T, U1, V))
    for b in range(B):
        Tb, Ub = int(lens[b]), len(labels[b])
        x = torch.from_numpy(np.ascontiguousarray(logits[b, :Tb, :Ub + 1])).to(dtype).requires_grad_(True)
        l, _ = torch_lattice(x, list(labels[b]), blank)
        if l is None:
            loss[b] = math.inf
            continue
        loss[b] = float(l.detach())
        grad[b, :Tb, :Ub + 1] = torch.autograd.grad(l, x)[0].double().numpy()
    return loss, grad


def _act(kind, x):
    return np.tanh(x) if kind == "tanh" else np.maximum(x, 0.0) if kind == "relu" else x


def joint(enc, pred, kind):
    """float64: out[b][t][u][:] = act(enc[b][t][:] + pred[b][u][:])"""
    return _act(kind, np.asarray(enc, np.float64)[:, :, None, :] + np.asarray(pred, np.float64)[:, None, :, :])


def joint_backward(out, dout, kind):
    """float64, from the forward OUTPUT: (d enc [B][T][J], d pred [B][U1][J])"""
    out, dout = np.asarray(out, np.float64), np.asarray(dout, np.float64)
    d = dout * (1.0 - out * out if kind == "tanh" else (out > 0) if kind == "relu" else 1.0)
    return d.sum(2), d.sum(1)
