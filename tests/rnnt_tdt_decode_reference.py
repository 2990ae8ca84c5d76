"""Token-and-duration greedy decoding as INTEGRATION.md "RNN-Transducer: token-and-duration greedy decoding" states it, in numpy: the
float64 reference the device tests compare with, the float32 restatement of the same recursion (sequential sums) that serves only as
the yardstick of what float32 arithmetic costs, and the lattice scores [B][T][U+1][V + D] the loss takes for given labels."""
import numpy as np

from rnnt_decode_reference import _act, _matvec, _sum, split_dense, split_lstm


def _network(embed, lstm_block, pred_proj, out, J, VD, dtype):
    """-> (step(k, h, c) -> h, c, g; H; Wo [J, V + D]; bo)"""
    seq = dtype == np.float32
    f = lambda a: np.asarray(a, dtype=dtype)
    embed = f(embed)
    E = embed.shape[1]
    H = int(round((-(E + 2) + ((E + 2) ** 2 + np.asarray(lstm_block).size) ** 0.5) / 2))
    W, U, b_i, b_h = (f(a) for a in split_lstm(lstm_block, E, H))
    Wp, bp = (f(a) for a in split_dense(pred_proj, H, J)) if pred_proj is not None else (None, None)
    Wo, bo = (f(a) for a in split_dense(out, J, VD))
    one = dtype(1)
    sig = lambda x: one / (one + np.exp(-x))

    def step(k, h, c):
        z = ((_matvec(embed[k], W, seq) + b_i) + _matvec(h, U, seq)) + b_h
        i, fg, g, o = sig(z[:H]), sig(z[H:2 * H]), np.tanh(z[2 * H:3 * H]), sig(z[3 * H:])
        c = fg * c + i * g
        h = o * np.tanh(c)
        return h, c, (_matvec(h, Wp, seq) + bp if Wp is not None else h)
    return step, H, Wo, bo


def _gap(v):
    top = np.sort(v)[-2:]
    return float(top[1] - top[0]) if len(v) > 1 else np.inf


def greedy_decode(embed, lstm_block, pred_proj, out, enc, durations, n_frames=None, blank=0, activation="tanh", max_symbols_per_frame=10,
                  max_labels=None, dtype=np.float64):
    """-> dict(labels, frames, durations: per-row lists; scores [B]; cells: per row the (t, u) of every decision; gaps [B]: the smallest
    best-minus-second gap over both heads' decisions (a blank's duration gap among the positive durations; inf without decisions);
    per-row counts blank_zero (blanks whose unrestricted duration winner was 0), label_zero (labels with duration 0), capped,
    skipped (frames jumped over: never the t of a decision), overshoot (frames the last jump went past n), and ends_exact [B]: the
    last move was a blank landing exactly on n)."""
    seq = dtype == np.float32
    dur = [int(d) for d in durations]
    D = len(dur)
    enc = np.asarray(enc, dtype=dtype)
    B, T, J = enc.shape
    V = np.asarray(embed).shape[0]
    step, H, Wo, bo = _network(embed, lstm_block, pred_proj, out, J, V + D, dtype)
    pos = np.array([d > 0 for d in dur])
    res = dict(labels=[], frames=[], durations=[], cells=[], scores=np.zeros(B, dtype), gaps=np.full(B, np.inf),
               ends_exact=np.zeros(B, bool), **{k: np.zeros(B, int) for k in ("blank_zero", "label_zero", "capped", "skipped", "overshoot")})
    lse = lambda v: v.max() + np.log(_sum(np.exp(v - v.max()), seq))
    for b in range(B):
        n = T if n_frames is None else int(n_frames[b])
        cap = max_symbols_per_frame * T if max_labels is None else max_labels
        h, c, g = step(blank, np.zeros(H, dtype), np.zeros(H, dtype))
        labels, frames, durs, cells = [], [], [], []
        t = s = 0
        score = dtype(0)
        while t < n and len(labels) < cap:
            x = _matvec(_act(activation, enc[b, t] + g), Wo, seq) + bo
            tok, du = x[:V], x[V:]
            k = int(np.argmax(tok))                  # the first of equal maxima
            if k == blank:
                i = int(np.flatnonzero(pos)[np.argmax(du[pos])])
                res["blank_zero"][b] += dur[int(np.argmax(du))] == 0
                dgap = _gap(du[pos])
            else:
                i = int(np.argmax(du))
                dgap = _gap(du)
            res["gaps"][b] = min(res["gaps"][b], _gap(tok), dgap)
            score = score + ((tok[k] - lse(tok)) + (du[i] - lse(du)))
            cells.append((t, len(labels)))
            res["ends_exact"][b] = k == blank and t + dur[i] == n
            if k == blank:
                t, s = t + dur[i], 0
            else:
                labels.append(k); frames.append(t); durs.append(dur[i])
                h, c, g = step(k, h, c)
                if dur[i] > 0:
                    t, s = t + dur[i], 0
                else:
                    res["label_zero"][b] += 1
                    s += 1
                    if s == max_symbols_per_frame:
                        t, s = t + 1, 0
                        res["capped"][b] += 1
        res["skipped"][b] = min(t, n) - len({cell[0] for cell in cells})
        res["overshoot"][b] = max(t - n, 0)
        res["labels"].append(labels); res["frames"].append(frames); res["durations"].append(durs); res["cells"].append(cells)
        res["scores"][b] = score
    return res


def lattice_scores(embed, lstm_block, pred_proj, out, enc, n_durations, labels, blank=0, activation="tanh"):
    """the float64 scores [B][T][U+1][V + D] of the loss's lattice for the given per-row labels, U = the longest row"""
    enc = np.asarray(enc, dtype=np.float64)
    B, T, J = enc.shape
    V = np.asarray(embed).shape[0]
    step, H, Wo, bo = _network(embed, lstm_block, pred_proj, out, J, V + n_durations, np.float64)
    U1 = max(len(l) for l in labels) + 1
    x = np.zeros((B, T, U1, V + n_durations))
    for b in range(B):
        h, c = np.zeros(H), np.zeros(H)
        for u, k in enumerate([blank] + list(labels[b])):
            h, c, g = step(k, h, c)
            x[b, :, u] = _act(activation, enc[b] + g) @ Wo + bo
    return x
