"""What the pruned transducer loss tests compare the library with (a helper, no test): the four operations of csrc/hip/rnnt_pruned.hip
restated in numpy float64 -- the simple loss with its two gradients and the occupancies, the prune ranges, the banded joiner with its
backward, the banded loss with its gradient -- and the two losses once more in torch at a chosen precision, differentiated by autograd
(float32: the error a careful float32 implementation has, which sets the tolerance of the device tests, as in tests/rnnt_reference.py).

One lattice serves both losses: a row's live cells [T_b][U_b + 1] with a mask of the cells that exist.  The simple loss has all of them,
the banded loss those with r[t] <= u < r[t] + S; a path may only pass through cells that exist.

Conventions (tests/rnnt_reference.py): row b has T_b = lens[b] frames and the labels labels[b]; cells with t >= T_b or u > U_b are
padding.  The simple loss's score is the FLOAT32 sum am + lm, rounded once, as the library defines it."""
import math

import numpy as np

import rnnt_reference as R


def feasible(Tb, Ub, S):
    """a connected band of S positions a frame can run from (0, 0) to (T_b - 1, U_b)"""
    return (Tb - 1) * (S - 1) >= Ub + 1 - S


def clamp_ranges(ranges, U1, S):
    return np.clip(np.asarray(ranges, np.int64), 0, U1 - S)


def lattice64(x, lab, blank, mask):
    """x [T][U + 1][V] float64 scores of one row's live cells, mask [T][U + 1] bool -> (loss, d loss / d x, occupancy [T][U + 1]);
    cells outside the mask are never looked at and get zeros.  No path: (inf, zeros, zeros).  The lattice is rnnt_reference.lattice64:
    a cell outside the mask has -inf for every log-probability"""
    lp = np.where(mask[:, :, None], R.log_softmax(np.where(mask[:, :, None], x, 0.0)), -math.inf)
    return R.lattice64(lp, lab, blank, factored=True)


def lattice_torch(x, lab, blank, mask, dtype):
    """the same three results from torch at `dtype` (rnnt_reference.torch_lattice), by autograd, as float64 numpy; the occupancy of a
    cell is what flows out of it: -(d loss / d log p_blank + d loss / d log p_label)"""
    import torch
    T, U1, V = x.shape
    U = U1 - 1
    X = torch.from_numpy(np.where(mask[:, :, None], x, 0.0)).to(dtype).requires_grad_(True)
    loss, lp = R.torch_lattice(X, lab, blank, mask)
    if loss is None:
        return math.inf, np.zeros((T, U1, V)), np.zeros((T, U1))
    loss.backward()
    glp = lp.grad.double().numpy()
    occ = -glp[:, :, blank].copy()
    for u in range(U):
        occ[:, u] -= glp[:, u, lab[u]]
    return float(loss.detach()), np.where(mask[:, :, None], X.grad.double().numpy(), 0.0), np.where(mask, occ, 0.0)


def _lattice(x, lab, blank, mask, dtype):
    return lattice64(x, lab, blank, mask) if dtype is None else lattice_torch(x, lab, blank, mask, dtype)


def simple_loss(am, lm, labels, lens, blank, dtype=None):
    """am [B][T][V], lm [B][U1][V] float32 -> (loss rows [B], d am, d lm, occupancy [B][T][U1]) as float64, zeros in the padding;
    dtype None: numpy float64, else the torch restatement at that precision"""
    am, lm = np.asarray(am, np.float32), np.asarray(lm, np.float32)
    B, T, V = am.shape
    U1 = lm.shape[1]
    loss, dam, dlm, occ = np.zeros(B), np.zeros((B, T, V)), np.zeros((B, U1, V)), np.zeros((B, T, U1))
    for b in range(B):
        Tb, Ub = int(lens[b]), len(labels[b])
        x = (am[b, :Tb, None, :] + lm[b, None, :Ub + 1, :]).astype(np.float64)          # the float32 sum, rounded once
        loss[b], g, occ[b, :Tb, :Ub + 1] = _lattice(x, list(labels[b]), blank, np.ones((Tb, Ub + 1), bool), dtype)
        dam[b, :Tb], dlm[b, :Ub + 1] = g.sum(1), g.sum(0)
    return loss, dam, dlm, occ


def first_choice(occ_row, Tb, Ub, S):
    """s0[t] for t < T_b: the lowest s in [0, fin] whose window sum (float64, u ascending) is the largest"""
    fin = max(0, Ub + 1 - S)
    s0 = np.zeros(Tb, np.int64)
    for t in range(Tb):
        best = None
        for s in range(fin + 1):
            w = np.float64(0.0)
            for u in range(s, s + S):
                w = w + np.float64(occ_row[t, u])
            if best is None or w > best:
                best, s0[t] = w, s
    return s0


def fix_up(s0, Tb, Ub, S):
    fin = max(0, Ub + 1 - S)
    r, prev = np.zeros(Tb, np.int64), 0
    for t in range(Tb):
        lo, hi = max(0, fin - (Tb - 1 - t) * (S - 1)), min(fin, t * (S - 1))
        L, H = max(lo, prev), min(hi, prev + S - 1)
        assert L <= H, (t, Tb, Ub, S)
        prev = r[t] = min(max(int(s0[t]), L), H)
    return r


def prune_ranges(occ, lens, label_lens, S):
    """occ [B][T][U1] -> ranges [B][T] int; frames t >= T_b get fin"""
    B, T, U1 = occ.shape
    assert 1 <= S <= U1
    out = np.zeros((B, T), np.int64)
    for b in range(B):
        Tb, Ub = int(lens[b]), int(label_lens[b])
        assert feasible(Tb, Ub, S), (b, Tb, Ub, S)
        out[b, :Tb] = fix_up(first_choice(occ[b], Tb, Ub, S), Tb, Ub, S)
        out[b, Tb:] = max(0, Ub + 1 - S)
    return out


def pruned_joint(enc, pred, ranges, S, kind):
    """float64: out[b][t][s][:] = act(enc[b][t][:] + pred[b][r[b][t] + s][:]), r clamped into [0, U1 - S]"""
    enc, pred = np.asarray(enc, np.float64), np.asarray(pred, np.float64)
    B, T, J = enc.shape
    r = clamp_ranges(ranges, pred.shape[1], S)
    idx = r[:, :, None] + np.arange(S)[None, None, :]                                    # [B][T][S]
    return R._act(kind, enc[:, :, None, :] + pred[np.arange(B)[:, None, None], idx])


def pruned_joint_backward(out, dout, ranges, U1, kind):
    """float64, from the forward OUTPUT [B][T][S][J]: (d enc [B][T][J], d pred [B][U1][J])"""
    out, dout = np.asarray(out, np.float64), np.asarray(dout, np.float64)
    B, T, S, J = out.shape
    d = dout * (1.0 - out * out if kind == "tanh" else (out > 0) if kind == "relu" else 1.0)
    r = clamp_ranges(ranges, U1, S)
    dpred = np.zeros((B, U1, J))
    for b in range(B):
        for t in range(T):
            dpred[b, r[b, t]:r[b, t] + S] += d[b, t]
    return d.sum(2), dpred


def pruned_loss(logits, ranges, labels, lens, blank, U1, dtype=None):
    """logits [B][T][S][V] on the band `ranges` [B][T] of a lattice U1 wide -> (loss rows [B], gradient [B][T][S][V]) as float64;
    zeros in the padding; a row whose band carries no mass: (inf, zeros)"""
    logits = np.asarray(logits, np.float32)
    B, T, S, V = logits.shape
    r = clamp_ranges(ranges, U1, S)
    loss, grad = np.zeros(B), np.zeros((B, T, S, V))
    for b in range(B):
        Tb, Ub = int(lens[b]), len(labels[b])
        x, mask = np.zeros((Tb, Ub + 1, V)), np.zeros((Tb, Ub + 1), bool)
        for t in range(Tb):
            for s in range(S):
                if r[b, t] + s <= Ub:
                    x[t, r[b, t] + s], mask[t, r[b, t] + s] = logits[b, t, s], True
        loss[b], g, _ = _lattice(x, list(labels[b]), blank, mask, dtype)
        for t in range(Tb):
            for s in range(S):
                if r[b, t] + s <= Ub:
                    grad[b, t, s] = g[t, r[b, t] + s]
    return loss, grad
