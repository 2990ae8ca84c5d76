"""What the fused transducer-loss tests compare the library with (a helper, no test), on top of tests/rnnt_reference.py: the joiner, a
float64 matmul with the Dense block W [J,V] | b [V], rnnt_loss_and_grad on those logits, and the chain rule by hand back to enc, pred, W
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


def _live(B, T, U1, labels, lens):
    live = np.zeros((B, T, U1), bool)
    for b in range(B):
        live[b, :int(lens[b]), :len(labels[b]) + 1] = True
    return live


def _dact(kind, z):
    return 1.0 - z * z if kind == "tanh" else (z > 0).astype(np.float64) if kind == "relu" else np.ones_like(z)


def fused_loss_and_grads(enc, pred, out_block, labels, lens, blank, kind):
    """float64: (loss rows [B], d enc [B][T][J], d pred [B][U1][J], d out_block [J V + V]) of sum_b loss_b"""
    enc, pred = np.asarray(enc, np.float64), np.asarray(pred, np.float64)
    B, T, J = enc.shape
    U1 = pred.shape[1]
    W, bias = (a.astype(np.float64) for a in split_block(out_block, J))
    live = _live(B, T, U1, labels, lens)
    pre = np.where(live[..., None], enc[:, :, None, :] + pred[:, None, :, :], 0.0)       # the padding: selected away, NaN included
    z = np.where(live[..., None], R._act(kind, pre), 0.0)
    logits = z @ W + bias
    loss, dlogits = R.rnnt_loss_and_grad(logits, labels, lens, blank)                    # exact zeros in the padding
    dz = (dlogits @ W.T) * _dact(kind, z)
    dz = np.where(live[..., None], dz, 0.0)
    dW = np.einsum("btuj,btuv->jv", z, dlogits)
    db = dlogits.sum((0, 1, 2))
    return loss, dz.sum(2), dz.sum(1), np.concatenate([dW.reshape(-1), db])


def torch_fused(enc, pred, out_block, labels, lens, blank, kind, dtype):
    """the same in torch on the CPU at `dtype` (rnnt_reference._torch_row per row), autograd -> float64 numpy, as above"""
    import torch
    B, T, J = enc.shape
    U1 = pred.shape[1]
    clean = lambda a: torch.from_numpy(np.nan_to_num(np.asarray(a, np.float64), nan=0.0)).to(dtype).requires_grad_(True)
    e, p, o = clean(enc), clean(pred), clean(np.asarray(out_block).reshape(-1))
    V = o.shape[0] // (J + 1)
    W, bias = o[:J * V].view(J, V), o[J * V:]
    act = torch.tanh if kind == "tanh" else torch.relu if kind == "relu" else (lambda x: x)
    rows = []
    for b in range(B):
        Tb, Ub = int(lens[b]), len(labels[b])
        x = act(e[b, :Tb, None, :] + p[b, None, :Ub + 1, :]) @ W + bias
        rows.append(R._torch_row(x, list(labels[b]), blank))
    loss = torch.stack(rows)
    ge, gp, go = torch.autograd.grad(loss.sum(), (e, p, o))
    return tuple(a.detach().double().numpy() for a in (loss, ge, gp, go))
