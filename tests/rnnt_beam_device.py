"""The device side that the transducer beam search's GPU tests share (tests/test_gpu_rnnt_beam.py, _lm, _detail, _wide): tensors to and
from the device, the decoder of a case, bit equality, the comparison with the float64 reference,
and the device's own transducer loss of a hypothesis.  A helper, no test."""
import numpy as np
import torch

import rnnt_decode_reference as R
from nntoolkitcore_amd import layers as NL


def to_device(gpu, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def decoder(gpu, c):
    m = c["m"]
    return NL.RnntDecoder(to_device(gpu, m["embed"]), to_device(gpu, m["lstm"]), to_device(gpu, m["proj"]), to_device(gpu, m["out"]),
                          blank=m["blank"], joint_activation=c["act"], max_symbols_per_frame=c["ms"])


def host(outs):
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in outs)


def same(x, y):
    return all(np.array_equal(p.view(np.int32), q.view(np.int32)) for p, q in zip(x, y))


def lattice_losses(gpu, c, pairs):
    """the transducer loss of (row, labels) pairs, the logits built through the device training path"""
    m = c["m"]
    B, T, J = c["enc"].shape
    V, E, H, blank = m["V"], m["E"], m["H"], m["blank"]
    N = len(pairs)
    U1 = max(len(y) for _, y in pairs) + 1
    x = np.zeros((N, U1, E), np.float32)
    for i, (_, y) in enumerate(pairs):
        x[i] = m["embed"][[blank] + list(y) + [blank] * (U1 - 1 - len(y))]
    lengths = np.array([len(y) for _, y in pairs], np.int32)
    W, U, b_i, b_h = R.split_lstm(m["lstm"], E, H)
    lstm = NL.LSTM(E, H, True, U1)
    lstm.set_weights(W, U, b_i, b_h)
    h = lstm.apply_device_varlen(to_device(gpu, x), lengths=lengths + 1)
    Wp, bp = R.split_dense(m["proj"], H, J)
    tdd = NL.TimeDistributedDense(U1, H, J)
    tdd.set_weights(Wp, bp)
    pred = tdd.apply_device(h)
    enc = to_device(gpu, np.stack([c["enc"][b] for b, _ in pairs]))
    joint = NL.rnnt_joint_device(enc, pred, c["act"])
    Wo, bo = R.split_dense(m["out"], J, V)
    voc = NL.TimeDistributedDense(T * U1, J, V)
    voc.set_weights(Wo, bo)
    logits = voc.apply_device(joint.reshape(N, T * U1, J)).reshape(N, T, U1, V)
    loss, _ = NL.rnnt_loss_device(logits, [list(y) for _, y in pairs], input_lengths=[c["n"][b] for b, _ in pairs], blank=blank,
                                  want_grad=False)
    torch.cuda.synchronize()
    loss = loss.cpu().numpy()
    for o in (lstm, tdd, voc):
        o.destroy()
    return loss


def assert_equals_reference(name, got, r64, nbest, tol):
    """got: (labels, lengths, scores) or, with detail, (labels, lengths, scores, frames, logps).  Labels, lengths and frames equal the
    reference's, the slots behind them are empty, and the scores are within tol(), the calling family's own tolerance."""
    labels, lengths, scores = got[:3]
    frames = got[3] if len(got) > 3 else None
    worst = 0.0
    for b in range(labels.shape[0]):
        have = len(r64["labels"][b])
        for k in range(nbest):
            if k < have:
                y = r64["labels"][b][k]
                assert lengths[b, k] == len(y) and labels[b, k, :len(y)].tolist() == y and (labels[b, k, len(y):] == -1).all(), \
                    (name, b, k, labels[b, k], y)
                if frames is not None:
                    assert frames[b, k, :len(y)].tolist() == r64["frames"][b][k], (name, b, k, frames[b, k], r64["frames"][b][k])
                worst = max(worst, abs(float(scores[b, k]) - float(r64["scores"][b][k])))
            else:
                assert lengths[b, k] == -1 and (labels[b, k] == -1).all() and scores[b, k] == -np.inf, (name, b, k)
                assert frames is None or (frames[b, k] == -1).all(), (name, b, k)
    print("%s: largest device score error %.3e (tolerance %.3e)" % (name, worst, tol()))
    assert worst <= tol(), (name, worst, tol())
