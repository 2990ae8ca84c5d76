"""What the fused token-and-duration loss tests compare the library with (a helper, no test), on top of tests/rnnt_fused_reference.py
(the forward: joiner, matmul against the block W [J][V + D] | b [V + D]) and tests/rnnt_tdt_reference.py (the loss on those logits): the
chain rule by hand in float64, the same in torch at a chosen precision, and the cases.  A case is rnnt_cases' fused dict plus durs and
sigma; `out` is the [J + 1][V + D] block."""
import math

import numpy as np

import rnnt_cases as K
import rnnt_fused_reference as FR
import rnnt_tdt_reference as TR


def loss_and_grads(c, kind):
    """float64: (loss rows [B], d enc, d pred, d out) of the sum of the finite loss rows"""
    z, logits = FR.fused_forward(c["enc"], c["pred"], c["out"], c["labels"], c["lens"], kind)
    W = FR.split_block(c["out"], z.shape[3])[0].astype(np.float64)
    loss, dlogits = TR.tdt_loss_and_grad(logits, c["labels"], c["lens"], c["durs"], c["blank"], c["sigma"])
    dz = (dlogits @ W.T) * FR._dact(kind, z)
    return loss, dz.sum(2), dz.sum(1), np.concatenate([np.einsum("btuj,btuv->jv", z, dlogits).reshape(-1), dlogits.sum((0, 1, 2))])


def torch_fused(c, kind, dtype):
    """the same in torch on the CPU at `dtype`, by autograd -> float64 numpy; a row without a path: loss inf, nothing differentiated"""
    import torch
    leaves, rows = FR.torch_fused_logits(c["enc"], c["pred"], c["out"], c["labels"], c["lens"], kind, dtype, grad=True)
    rows = [TR.torch_row(x, list(c["labels"][b]), c["blank"], c["durs"], c["sigma"]) for b, x in enumerate(rows)]
    live = [l for l in rows if l is not None]
    grads = torch.autograd.grad(torch.stack(live).sum(), leaves) if live else [torch.zeros_like(a) for a in leaves]
    return (np.array([math.inf if l is None else float(l.detach()) for l in rows]),) + tuple(a.detach().double().numpy() for a in grads)


def _two_heads(c, J, V, durs, sigma, seed):
    """a classic fused case (labels among V tokens) with the block widened to V + D columns"""
    rng, sc, VD = np.random.default_rng(seed), 1.0 / np.sqrt(J), V + len(durs)
    c.update(out=np.concatenate([rng.uniform(-3 * sc, 3 * sc, J * VD), rng.uniform(-1, 1, VD)]).astype(np.float32), durs=list(durs),
             sigma=sigma)
    return c


def ragged(J, V, durs, blank, sigma=0.0, seed=0):
    """rnnt_cases.fused_ragged: input lengths 7 / 4 / 1 of T = 7, label lengths 3 / 0 / 5; label V - 1 in row 2 unless it is the blank"""
    return _two_heads(K.fused_ragged(J, V, blank, seed), J, V, durs, sigma, 31 * J + V + seed)


def single(T, U, J, V, durs, blank, seed):
    return _two_heads(K.fused_single(T, U, J, V, blank, seed), J, V, durs, 0.0, seed + 1)
