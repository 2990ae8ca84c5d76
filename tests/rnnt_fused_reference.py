"""What the fused transducer-loss and alignment tests compare the library with (a helper, no test), on top of tests/rnnt_reference.py:
the one float64 forward (joiner, matmul with the Dense block W [J,V] | b [V]) and the one torch forward, which
tests/rnnt_align_reference.py uses too; rnnt_loss_and_grad on those logits, and the chain rule by hand back to enc, pred, W
and b -- the gradients of the PLAIN SUM of the loss rows; and the same computation in torch on the CPU at a chosen precision,
differentiated by autograd (float64: an independent statement of the gradients; float32: the error of a careful float32 implementation,
the yardstick of the device tests).

Padding cells (t >= lens[b] or u > len(labels[b])) are never looked at: enc / pred may hold NaN there."""
import numpy as np

import rnnt_reference as R


def split_block(out_block, J):
    out_block = np.asarray(out_block).reshape(-1)
    V = out_block.size // (J + 1)
    assert out_block.size == (J + 1) * V
    return out_block[:J * V].reshape(J, V), out_block[J * V:]


def _dact(kind, z):
    return 1.0 - z * z if kind == "tanh" else (z > 0).astype(np.float64) if kind == "relu" else np.ones_like(z)


def fused_forward(enc, pred, out_block, labels, lens, kind):
    """float64, the one forward of the fused tests: (z [B][T][U1][J] = act(enc + pred), logits [B][T][U1][V] = z W + b) on the live
    cells, zeros in the padding (whose inputs may hold NaN and are never read)"""
    enc, pred = np.asarray(enc, np.float64), np.asarray(pred, np.float64)
    B, T, J = enc.shape
    U1 = pred.shape[1]
    W, bias = (a.astype(np.float64) for a in split_block(out_block, J))
    z, x = np.zeros((B, T, U1, J)), np.zeros((B, T, U1, W.shape[1]))
    for b in range(B):
        n, u1 = int(lens[b]), len(labels[b]) + 1
        z[b, :n, :u1] = R._act(kind, enc[b, :n, None, :] + pred[b, None, :u1, :])
        x[b, :n, :u1] = z[b, :n, :u1] @ W + bias
    return z, x


def fused_loss_and_grads(enc, pred, out_block, labels, lens, blank, kind):
    """float64: (loss rows [B], d enc [B][T][J], d pred [B][U1][J], d out_block [J V + V]) of sum_b loss_b"""
    z, logits = fused_forward(enc, pred, out_block, labels, lens, kind)
    W = split_block(out_block, z.shape[3])[0].astype(np.float64)
    loss, dlogits = R.rnnt_loss_and_grad(logits, labels, lens, blank)                    # exact zeros in the padding
    dz = (dlogits @ W.T) * _dact(kind, z)                                                # so here too: z is 0 there, never NaN
    dW = np.einsum("btuj,btuv->jv", z, dlogits)
    db = dlogits.sum((0, 1, 2))
    return loss, dz.sum(2), dz.sum(1), np.concatenate([dW.reshape(-1), db])


def torch_fused_logits(enc, pred, out_block, labels, lens, kind, dtype, grad=False):
    """the one torch restatement of the forward, on the CPU at `dtype`: ((enc, pred, out_block) as leaves, NaN padding cleaned; the
    logits [T_b][U_b + 1][V] of every row's live cells)"""
    import torch
    J = enc.shape[2]
    clean = lambda a: torch.from_numpy(np.nan_to_num(np.asarray(a, np.float64), nan=0.0)).to(dtype).requires_grad_(grad)
    e, p, o = clean(enc), clean(pred), clean(np.asarray(out_block).reshape(-1))
    V = o.shape[0] // (J + 1)
    W, bias = o[:J * V].view(J, V), o[J * V:]
    act = torch.tanh if kind == "tanh" else torch.relu if kind == "relu" else (lambda x: x)
    return (e, p, o), [act(e[b, :int(lens[b]), None, :] + p[b, None, :len(labels[b]) + 1, :]) @ W + bias for b in range(enc.shape[0])]


def torch_fused(enc, pred, out_block, labels, lens, blank, kind, dtype):
    """the loss in torch on the CPU at `dtype` (rnnt_reference.torch_lattice per row), autograd -> float64 numpy, as above; a row without
    a path has the loss inf and adds nothing to the sum that is differentiated"""
    import torch
    leaves, rows = torch_fused_logits(enc, pred, out_block, labels, lens, kind, dtype, grad=True)
    rows = [R.torch_lattice(x, list(labels[b]), blank)[0] for b, x in enumerate(rows)]
    loss = np.array([np.inf if l is None else float(l.detach()) for l in rows])
    live = [l for l in rows if l is not None]
    grads = torch.autograd.grad(torch.stack(live).sum(), leaves) if live else [torch.zeros_like(a) for a in leaves]
    return (loss,) + tuple(a.detach().double().numpy() for a in grads)
