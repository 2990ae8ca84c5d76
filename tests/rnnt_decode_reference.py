"""Greedy RNN-Transducer decoding as INTEGRATION.md "RNN-Transducer: greedy decoding" states it, on the library's weight blocks, in
numpy: the float64 reference the device tests compare with, and a float32 restatement of the same recursion (sequential sums, numpy's
float32 exp / tanh / log) that serves only as the yardstick of what float32 arithmetic costs on the same inputs."""
import numpy as np


def split_lstm(block, E, H):
    """the LSTMGetWeights block -> W [E,4H], U [H,4H], b_i [4H], b_h [4H]"""
    b = np.asarray(block).reshape(-1)
    G = 4 * H
    assert b.shape[0] == G * (E + H + 2)
    return b[:E * G].reshape(E, G), b[E * G:(E + H) * G].reshape(H, G), b[(E + H) * G:(E + H + 1) * G], b[(E + H + 1) * G:]


def split_dense(block, K, N):
    b = np.asarray(block).reshape(-1)
    assert b.shape[0] == (K + 1) * N
    return b[:K * N].reshape(K, N), b[K * N:]


def _act(kind, z):
    return np.tanh(z) if kind == "tanh" else np.maximum(z, 0) if kind == "relu" else z


def _matvec(x, W, sequential):
    if not sequential:
        return x @ W
    acc = np.zeros(W.shape[1], W.dtype)
    for k in range(W.shape[0]):                      # one rounding per product and per sum, k ascending
        acc = acc + x[k] * W[k]
    return acc


def _sum(v, sequential):
    if not sequential:
        return v.sum()
    s = v.dtype.type(0)
    for x in v:
        s = s + x
    return s


def greedy_decode(embed, lstm_block, pred_proj, out, enc, n_frames=None, blank=0, activation="tanh", max_symbols_per_frame=10,
                  max_labels=None, dtype=np.float64):
    """-> dict(labels, frames: per-row lists; scores [B]; gaps [B]: the smallest difference between the best and the second-best logit
    over the row's decisions (inf for a row without decisions); cells: per row the (t, u) of every decision; capped [B]: moves to the
    next frame forced by the cap; ends_on_label [B]).  dtype float32: the sequential restatement."""
    seq = dtype == np.float32
    f = lambda a: np.asarray(a, dtype=dtype)
    embed, enc = f(embed), f(enc)
    V, E = embed.shape
    B, T, J = enc.shape
    H = int(round((-(E + 2) + ((E + 2) ** 2 + np.asarray(lstm_block).size) ** 0.5) / 2))
    W, U, b_i, b_h = (f(a) for a in split_lstm(lstm_block, E, H))
    Wp, bp = (f(a) for a in split_dense(pred_proj, H, J)) if pred_proj is not None else (None, None)
    Wo, bo = (f(a) for a in split_dense(out, J, V))
    one = dtype(1)
    sig = lambda x: one / (one + np.exp(-x))

    def step(k, h, c):
        z = ((_matvec(embed[k], W, seq) + b_i) + _matvec(h, U, seq)) + b_h
        i, fg, g, o = sig(z[:H]), sig(z[H:2 * H]), np.tanh(z[2 * H:3 * H]), sig(z[3 * H:])
        c = fg * c + i * g
        h = o * np.tanh(c)
        return h, c, (_matvec(h, Wp, seq) + bp if Wp is not None else h)

    res = dict(labels=[], frames=[], cells=[], scores=np.zeros(B, dtype), gaps=np.full(B, np.inf), capped=np.zeros(B, int),
               ends_on_label=np.zeros(B, bool))
    for b in range(B):
        n = T if n_frames is None else int(n_frames[b])
        cap = max_symbols_per_frame * T if max_labels is None else max_labels
        h, c, g = step(blank, np.zeros(H, dtype), np.zeros(H, dtype))
        labels, frames, cells = [], [], []
        t = s = 0
        score = dtype(0)
        last = None
        while t < n and len(labels) < cap:
            logits = _matvec(_act(activation, enc[b, t] + g), Wo, seq) + bo
            k = int(np.argmax(logits))               # the first of equal maxima
            top = np.sort(logits)[-2:]
            res["gaps"][b] = min(res["gaps"][b], float(top[1] - top[0]))
            m = logits[k]
            score = score + ((logits[k] - m) - np.log(_sum(np.exp(logits - m), seq)))
            cells.append((t, len(labels)))
            last = k
            if k == blank:
                t, s = t + 1, 0
            else:
                labels.append(k); frames.append(t)
                h, c, g = step(k, h, c)
                s += 1
                if s == max_symbols_per_frame:
                    t, s = t + 1, 0
                    res["capped"][b] += 1
        res["labels"].append(labels); res["frames"].append(frames); res["cells"].append(cells)
        res["scores"][b] = score
        res["ends_on_label"][b] = last is not None and last != blank
    return res
