"""What the transducer forced-alignment tests compare the library with (a helper, no test): the Viterbi path through the lattice in
float64 log space with the contract's tie-break; the same recursion's score in torch float32 (the error a careful float32 implementation
has, which sets the tolerance of the device tests); brute-force enumeration of every path for tiny lattices; the shared cases of the
host and device tests; teacher-forced logits of the greedy decoder's model in float64.

Conventions (tests/rnnt_reference.py): logits [B][T][U1][V], U1 = max_label_len + 1; row b has T_b = lens[b] frames and the labels
labels[b] (U_b of them); cells with t >= T_b or u > U_b are padding and are never looked at.

Recursion: v(0, 0) = 0 (ln 1); into cell (t, u) the candidates are v(t-1, u) + ln p_blank(t-1, u) (the blank move), then
v(t, u-1) + ln p_label(t, u-1) (the label move); the label move replaces the blank move only if it is strictly greater.  With equal
candidates everywhere the walk back from (T_b-1, U_b) therefore takes blanks down to frame 0 first: every label is emitted in frame 0."""
import functools
import math

import numpy as np

import rnnt_cases as K
import rnnt_fused_reference as FR
import rnnt_reference as R


def viterbi_row(lp, lab, blank):
    """lp [T][U + 1][V] float64 log-probabilities of one row's live cells -> dict(score; label_frames [U]; frame_labels [T];
    label_logp [U]; frame_logp [T]; gap: the smallest |difference| of the two candidates over the decisions where both are finite,
    inf where there is none).  A row without a path of non-zero probability: score -inf, frames and labels -1, logp 0."""
    T, U1, _ = lp.shape
    U = U1 - 1
    v = np.full((T, U1), -math.inf)
    step = np.zeros((T, U1), np.int8)
    gap = math.inf
    v[0, 0] = 0.0
    for t in range(T):
        for u in range(U1):
            if t == 0 and u == 0:
                continue
            a = v[t - 1, u] + lp[t - 1, u, blank] if t > 0 else -math.inf
            c = v[t, u - 1] + lp[t, u - 1, lab[u - 1]] if u > 0 else -math.inf
            if a > -math.inf and c > -math.inf:
                gap = min(gap, abs(a - c))
            v[t, u], step[t, u] = (c, 1) if c > a else (a, 0)
    score = v[T - 1, U] + lp[T - 1, U, blank]
    res = dict(score=score, gap=gap, label_frames=np.full(U, -1), frame_labels=np.full(T, -1), label_logp=np.zeros(U), frame_logp=np.zeros(T))
    if score == -math.inf:
        return res
    t, u = T - 1, U
    res["frame_labels"][t], res["frame_logp"][t] = u, lp[t, u, blank]
    while (t, u) != (0, 0):
        if step[t, u]:
            u -= 1
            res["label_frames"][u], res["label_logp"][u] = t, lp[t, u, lab[u]]
        else:
            t -= 1
            res["frame_labels"][t], res["frame_logp"][t] = u, lp[t, u, blank]
    return res


def viterbi(logits, labels, lens, blank):
    """float64, per row: viterbi_row on the row's live cells"""
    return [viterbi_row(R.log_softmax(logits[b, :int(lens[b]), :len(labels[b]) + 1]), list(labels[b]), blank) for b in range(logits.shape[0])]


def brute_force_row(lp, lab, blank):
    """every path of one row by enumeration -> (the best score, its label_frames): among paths of exactly equal score the one whose
    LAST move that differs from another's is the blank -- what the recursion's tie-break selects"""
    T, U = lp.shape[0], len(lab)
    paths = []

    def walk(t, u, logp, moves, frames):
        if u < U:
            walk(t, u + 1, logp + lp[t, u, lab[u]], moves + "l", frames + [t])
        if t + 1 < T:
            walk(t + 1, u, logp + lp[t, u, blank], moves + "b", frames)
        elif u == U:
            paths.append((logp + lp[t, u, blank], moves + "b", frames))

    walk(0, 0, 0.0, "", [])
    best = max(p[0] for p in paths)
    tied = [p for p in paths if p[0] == best]
    tied.sort(key=lambda p: p[1][::-1])                  # "b" < "l": the blank first, from the last move backwards
    return best, tied[0][2], len(paths)


def torch_score_row(x, lab, blank):
    """the recursion's score for one row's live cells x [T][U + 1][V], a torch tensor of any float type, diagonal by diagonal"""
    import torch
    T, U1, _ = x.shape
    U = U1 - 1
    lp = torch.log_softmax(x, -1)
    lb = lp[:, :, blank]
    ly = lp[:, :U, :].gather(2, torch.tensor(lab, dtype=torch.long).view(1, U, 1).expand(T, U, 1)).squeeze(2) if U else None
    ninf = torch.full((U1,), -math.inf, dtype=x.dtype)
    v = ninf.clone()
    v[0] = 0
    for n in range(1, T + U):
        lo, hi = max(0, n - T + 1), min(U, n)
        a, c = ninf.clone(), ninf.clone()
        u = torch.arange(lo, min(hi, n - 1) + 1)
        if u.numel():
            a[u] = v[u] + lb[n - 1 - u, u]
        u = torch.arange(max(lo, 1), hi + 1)
        if u.numel():
            c[u] = v[u - 1] + ly[n - u, u - 1]
        v = torch.maximum(a, c)
    return v[U] + lb[T - 1, U]


def torch_scores(logits, labels, lens, blank, dtype):
    """the scores at `dtype` on the CPU -> float64 numpy [B]"""
    import torch
    out = np.zeros(logits.shape[0])
    for b in range(logits.shape[0]):
        x = torch.from_numpy(np.ascontiguousarray(logits[b, :int(lens[b]), :len(labels[b]) + 1])).to(dtype)
        out[b] = float(torch_score_row(x, list(labels[b]), blank))
    return out


def gap_threshold(Tb, Ub):
    """a decision whose candidates differ by more than this is the same on the device: an emission rounded to 2^-23 plus one multiply
    per step on both competing paths, doubled"""
    return 8 * (Tb + Ub + 2) * 2.0 ** -24


# ---- the cases both test files share: float32(scale * standard_normal) from default_rng(seed), labels in [1, V) (blank 0) ----

def random_case(B, T, maxL, V, scale, seed=0, lens=None, ulens=None, blank=0):
    rng = np.random.default_rng(seed)
    x = (scale * rng.standard_normal((B, T, maxL + 1, V))).astype(np.float32)
    lens = [T] * B if lens is None else [int(rng.integers(lens[0], lens[1] + 1)) for _ in range(B)]
    ulens = [maxL] * B if ulens is None else [int(k) for k in ulens]
    labels = [K.labels(rng, n, V, blank) for n in ulens]
    return dict(x=x, labels=labels, lens=lens, blank=blank)


def ragged_case(V, blank, seed=0):
    """B = 8, T = 7, maxL = 4: rows with U = 0, T_b = 1, U_b = maxL, repeated labels"""
    c = random_case(8, 7, 4, V, 3.0, seed=seed, ulens=[0, 4, 4, 2, 3, 1, 4, 0], blank=blank)
    c["lens"] = [7, 1, 7, 4, 5, 1, 3, 1]
    c["labels"][2][1] = c["labels"][2][0]                # repeated labels
    c["labels"][6][3] = c["labels"][6][2] = c["labels"][6][1]
    return c


def instantiation_case(T, maxL):
    """B = 3, V = 3, scale 6, rows (T, maxL), (T, maxL), (T - 1, maxL / 2)"""
    c = random_case(3, T, maxL, 3, 6.0, ulens=[maxL, maxL, maxL // 2])
    c["lens"] = [T, T, T - 1]
    return c


# (T, maxL) -> (NJ of the rnnt_viterbi_kernel instantiation, whether its LDS needs the opt-in above 48 KiB)
INSTANTIATIONS = {(6, 4): (1, False), (6, 200): (1, False), (5, 300): (2, False), (3, 600): (0, False), (2, 1600): (0, True)}
BT_DIAGS = 2048                                      # RNNT_BT_DIAGS: the diagonals of one staged block of the backtrace at most


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "ragged":
        return ragged_case(5, 2)
    if name.startswith("ragged_V"):
        return ragged_case(int(name[8:]), 0)
    if name == "random":
        return random_case(32, 40, 12, 29, 3.0, lens=(20, 40))
    if name == "long":
        return random_case(8, 120, 60, 29, 3.0, seed=4)      # (seeds 0, 1 and 3 leave a row's smallest gap below the threshold)
    if name.startswith("inst_"):
        T, maxL = (int(k) for k in name.split("_")[1:])
        return instantiation_case(T, maxL)
    if name == "two_blocks":                         # a path of T + U = 2102 moves: more than one staged block of the backtrace
        return random_case(2, 2100, 2, 3, 3.0, ulens=[2, 1])
    if name == "flat":                               # every path ties
        c = random_case(3, 5, 3, 4, 0.0, ulens=[3, 2, 0])
        c["lens"] = [5, 3, 4]
        return c
    if name == "peaked":                             # one path holds all of the mass but e^-80: blanks and labels in a fixed pattern
        c = random_case(3, 6, 4, 6, 1.0, ulens=[4, 2, 0], seed=5)
        c["lens"] = [6, 4, 3]
        c["x"] = c["x"].copy()
        paths = []
        for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):
            t = u = 0
            frames, moves = [], []
            while t < n:
                if u < len(lab) and ((t + u) % 2 == 1 or t == n - 1):    # (the last frame emits what is left)
                    moves.append((t, u, lab[u]))
                    frames.append(t)
                    u += 1
                else:
                    moves.append((t, u, c["blank"]))
                    t += 1
            # every blank and every next label 40 below where it was, except on the path: the other paths hold e^-80 of the mass,
            # while the path's own emissions stay ordinary probabilities
            c["x"][b, :, :, c["blank"]] -= 40.0
            for u, k in enumerate(lab):
                c["x"][b, :, u, k] -= 40.0
            for t, u, k in moves:
                c["x"][b, t, u, k] += 40.0
            paths.append(frames)
        c["paths"] = paths
        return c
    if name == "range":
        # the `underflow` construction of tests/test_gpu_rnnt.py, pushed down: class 7 takes the mass everywhere; off the path every
        # needed score lies 2000 below it, on the path it equals it, except in two cells where it lies 1380 below.  Leaving the path
        # costs two off-path moves (4000) against the 2760 of staying on it: the best path's probability is about e^-2763 = 1e-1200
        rng = np.random.default_rng(3)
        T, U, V = 6, 4, 8
        lab = [1, 2, 2, 4]
        x = np.full((1, T, U + 1, V), -2000.0, np.float32) + rng.uniform(-0.5, 0.5, (1, T, U + 1, V)).astype(np.float32)
        x[..., 7] = 0.0
        t = u = 0
        frames = []
        for i, m in enumerate("blbbllbblb"):
            x[0, t, u, 0 if m == "b" else lab[u]] = -1380.0 if i in (3, 6) else 0.0
            if m == "l":
                frames.append(t)
            t, u = (t + 1, u) if m == "b" else (t, u + 1)
        assert (t, u) == (T, U)
        return dict(x=x, labels=[lab], lens=[T], blank=0, paths=[frames])
    if name == "forced":
        # -inf scores: row 0, every blank of frames 0 .. T-2 at u < U forbidden: all labels must come before the first blank, i.e. in
        # frame 0; row 1, the blank of the last cell forbidden: no path at all; row 2 untouched
        c = random_case(3, 5, 3, 4, 2.0, seed=9)
        c["x"] = c["x"].copy()
        c["x"][0, :, :3, 0] = -np.inf
        c["x"][1, 4, 3, 0] = -np.inf
        return c
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(the float64 rows of viterbi, the float32 torch scores) of a case, computed once"""
    import torch
    c = case(name)
    return viterbi(c["x"], c["labels"], c["lens"], c["blank"]), torch_scores(c["x"], c["labels"], c["lens"], c["blank"], torch.float32)


def left_out(name):
    """the rows whose smallest decision gap does not exceed the threshold: left out of the exact comparison of the frames"""
    c = case(name)
    return [b for b, r in enumerate(reference(name)[0]) if not r["gap"] > gap_threshold(c["lens"][b], len(c["labels"][b]))]


# ---- the fused form: the cases of tests/rnnt_cases.py, the forwards of tests/rnnt_fused_reference.py ----

def torch_fused_scores(enc, pred, out_block, labels, lens, blank, kind, dtype):
    """the fused form's scores in torch at `dtype` on the CPU -> float64 numpy [B]"""
    rows = FR.torch_fused_logits(enc, pred, out_block, labels, lens, kind, dtype)[1]
    return np.array([float(torch_score_row(x, list(labels[b]), blank)) for b, x in enumerate(rows)])


FUSED_RAGGED = [(5, 5, 4), (5, 5, 2), (67, 257, 100), (67, 257, 256)]
FUSED_KINDS = ("tanh", "identity", "relu")
FUSED_CELLS = [(4, 4), (4, 7), (3, 10)]              # T x (U + 1) = 20, 32, 33 cells: around one tile of 32
# the device's fused logits are one float32 fmaf chain over J terms each, |error| about J 2^-24 |logit| -- some 1e-5 at J = 67 -- on top
# of the lattice's roundings: the fused cases' decisions have to be clearer than this, whatever gap_threshold says
FUSED_GAP = 1e-3


@functools.lru_cache(maxsize=None)
def fused_case(name):
    if name.startswith("ragged"):
        J, V, blank = (int(k) for k in name.split("_")[1:])
        return K.fused_ragged(J, V, blank)
    if name.startswith("cells"):
        T, U = (int(k) for k in name.split("_")[1:])
        return K.fused_single(T, U, 5, 5, 1, 40 + U, scale=3.0)
    if name == "wide":                               # U = 300: rnnt_viterbi_kernel<2> behind the fused emission writer
        return K.fused_single(4, 300, 6, 4, 0, 11, scale=6.0)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def fused_reference(name, kind):
    """(float64 logits, the float64 rows of viterbi on them, the float32 torch scores)"""
    import torch
    c = fused_case(name)
    x = FR.fused_forward(c["enc"], c["pred"], c["out"], c["labels"], c["lens"], kind)[1]
    return x, viterbi(x, c["labels"], c["lens"], c["blank"]), torch_fused_scores(c["enc"], c["pred"], c["out"], c["labels"], c["lens"],
                                                                                 c["blank"], kind, torch.float32)


# ---- against greedy decoding: the model of tests/test_gpu_rnnt_decode.py, its scores peaked ----

def greedy_model(seed=1945, out_scale=5.0, label_bias=-2.0):
    """_model of tests/test_gpu_rnnt_decode.py (V 5, E 7, H 12, J 20, with the projection), the vocabulary Dense scaled up so that
    the greedy path is also the Viterbi path (seed, scale and bias chosen on the CPU: tests/test_rnnt_align_host.py asserts it)"""
    rng = np.random.default_rng(seed)
    u = lambda sc, *s: rng.uniform(-sc, sc, s).astype(np.float32)
    V, E, H, J, blank, scale = 5, 7, 12, 20, 0, 2.0
    G = 4 * H
    bias = u(0.1, V)
    bias[np.arange(V) != blank] += np.float32(label_bias)
    m = dict(V=V, E=E, H=H, J=J, blank=blank, embed=u(1.0, V, E),
             lstm=np.concatenate([u(scale * E ** -0.5, E * G), u(scale * H ** -0.5, H * G), u(0.1, G), u(0.1, G)]),
             proj=np.concatenate([u(scale * H ** -0.5, H * J), u(0.1, J)]), out=np.concatenate([u(out_scale * J ** -0.5, J * V), bias]))
    m["enc"] = rng.uniform(-1.5, 1.5, (3, 9, J)).astype(np.float32)
    m["n"] = [9, 4, 1]
    return m


def teacher_forced_logits(m, labels, maxL, kind="tanh"):
    """float64 [B][T][maxL + 1][V]: the prediction network run over each row's labels, joiner, vocabulary Dense"""
    import rnnt_decode_reference as D
    E, H, J, V, blank = m["E"], m["H"], m["J"], m["V"], m["blank"]
    W, U, b_i, b_h = (np.asarray(a, np.float64) for a in D.split_lstm(m["lstm"], E, H))
    Wp, bp = (np.asarray(a, np.float64) for a in D.split_dense(m["proj"], H, J))
    Wo, bo = (np.asarray(a, np.float64) for a in D.split_dense(m["out"], J, V))
    sig = lambda z: 1.0 / (1.0 + np.exp(-z))
    B, T, _ = m["enc"].shape
    x = np.zeros((B, T, maxL + 1, V))
    for b in range(B):
        h, c = np.zeros(H), np.zeros(H)
        for u, k in enumerate([blank] + list(labels[b])):
            z = ((np.asarray(m["embed"], np.float64)[k] @ W + b_i) + h @ U) + b_h
            i, fg, g, o = sig(z[:H]), sig(z[H:2 * H]), np.tanh(z[2 * H:3 * H]), sig(z[3 * H:])
            c = fg * c + i * g
            h = o * np.tanh(c)
            x[b, :, u] = D._act(kind, np.asarray(m["enc"], np.float64)[b] + (h @ Wp + bp)) @ Wo + bo
    return x
