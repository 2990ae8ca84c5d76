"""The cases of the transducer loss tests that feed -inf scores (a helper, no test; numpy only, every seed fixed): tests/test_rnnt_masked_host.py
checks their premises without a device, tests/test_gpu_rnnt_masked.py runs them.  -inf goes into LIVE cells only; the padding is the
caller's to fill with NaN (rnnt_cases.with_nan_padding, nan_padded_sum).

Every case is a dict in the conventions of tests/rnnt_cases.py -- stored: x [B][T][U1][V]; simple: am [B][T][V], lm [B][U1][V]; fused:
enc, pred, out = W | b -- with labels, lens, blank and
  finite: per row, whether a path with mass is left (a row that is not has P = 0: loss +inf, every gradient row zero)
  masked: the rows that hold a -inf score (the others must keep the bits of a call without them)

Stored variants, on the shape of rnnt_cases.ragged (B = 3, T = 7, lengths 7 / 4 / 1, max_label_len 5, label lengths 3 / 0 / 5):
  class       one class that is neither the blank nor a label of any row is -inf in every live cell (V = 260: a class of the last quad)
  forced      row 0's blank is -inf at frames 0 .. T_b - 2 for u < U_b: every label comes in frame 0, one path
  wall        row 0's label y_2 is -inf at u = 1 in every frame: no path crosses, P = 0
  last blank  row 2's blank is -inf at (T_b - 1, U_b): P = 0 through the final factor alone, alpha positive everywhere
  dead cell   all V scores of the interior cell (3, 1) of row 0 are -inf: P > 0, the other paths go round it
  all rows    wall on the rows with a label, last blank on the row with none: the whole batch at +inf
  (tiny = True: the same variants on a batch small enough to enumerate, T = 4 and max_label_len 3; the dead cell is (2, 1) there)
Simple variants, on the base case of tests/test_gpu_rnnt_pruned.py (B = 3, T = 9, lengths 9 / 5 / 2, max_label_len 4, label lengths
4 / 0 / 2); a -inf in am or lm is a -inf in every cell of its frame or its column:
  class lm    the class is -inf in lm, every live column;  class am: in am, frames 1, 2 and the last of every row
  forced      lm[0][u][blank] = -inf for u < U_b (one path);  wall: lm[0][1][y_2] = -inf;  last blank: lm[2][U_b][blank] = -inf
  dead cell   lm[0][1][v] = -inf for every v but the label y_2 that leaves column 1, and am[0][4][y_2] = -inf: the sum of cell (4, 1) is
              all -inf and of no other cell; P > 0, the paths cross column 1 in another frame (by y_2 at once: its blank is gone)
  dead column lm[0][2][:] = -inf: a whole column of such cells, which no path can go round (P = 0, the reductions skip the row)
  all rows    wall on the rows with a label, last blank on the row with none
Fused variants (J = 8, V = 300, the lengths of rnnt_cases.fused_ragged, tanh): -inf enters through the bias alone."""
import numpy as np

import rnnt_cases as K

NINF = -np.inf
STORED_VB = [(5, 0), (5, 4), (260, 0), (260, 259)]          # the scalar and the 16-byte paths of rnnt_emit_row / rnnt_grad_row
STORED_VARIANTS = ("class", "forced", "wall", "last blank", "dead cell", "all rows")
SIMPLE_VARIANTS = ("class lm", "class am", "forced", "wall", "last blank", "dead cell", "dead column", "all rows")
SIMPLE_DEAD_CELL = (4, 1)                                   # of row 0 (T_b = 9, U_b = 4)
FUSED_VARIANTS = ("first block", "whole wave", "tail", "blank masked")

# rnnt_fused.hip's forward: FT_WAVES waves take 32 columns of V each, FT_COLS a pass; mirrored, and checked against the source text by
# tests/test_rnnt_masked_host.py
FT_WAVES, FT_BLOCK = 8, 32
FT_COLS = FT_WAVES * FT_BLOCK
FUSED_J, FUSED_V, FUSED_BLANK = 8, 300, 100
FUSED_MASKS = {"first block": list(range(0, 32)), "whole wave": list(range(32, 64)) + list(range(288, 300)), "tail": list(range(288, 300)),
               "blank masked": [FUSED_BLANK]}


def masked_class(V):
    """never the blank of STORED_VB, never drawn as a label; V = 260: in the last quad"""
    return V - 2


def _labels(rng, n, V, blank):
    classes = [k for k in range(V) if k not in (blank, masked_class(V))]
    return [classes[int(k)] for k in rng.integers(0, len(classes), n)]


def stored_base(V, blank):
    """rnnt_cases.ragged's scores and lengths; the labels drawn again without the masked class (row 0 and row 2 still repeat one)"""
    c = K.ragged(V, blank)
    rng = np.random.default_rng(10 * V + blank)
    a, z, r2 = _labels(rng, 1, V, blank)[0], _labels(rng, 1, V, blank)[0], _labels(rng, 5, V, blank)
    r2[2] = r2[1]
    return dict(c, labels=[[a, a, z], [], r2])


def _wall_and_last_blank(x, c, rows):
    for b in rows:
        Tb, lab = c["lens"][b], c["labels"][b]
        if lab:
            x[b, :Tb, min(1, len(lab) - 1), lab[min(1, len(lab) - 1)]] = NINF
        else:
            x[b, Tb - 1, 0, c["blank"]] = NINF


def tiny_base(V, blank):
    """small enough to enumerate: T = 4 with lengths 4 / 3 / 1, max_label_len 3 with label lengths 3 / 0 / 2"""
    rng = np.random.default_rng(77 * V + blank)
    a, z = _labels(rng, 1, V, blank)[0], _labels(rng, 1, V, blank)[0]
    return dict(x=rng.uniform(-3, 3, (3, 4, 4, V)).astype(np.float32), labels=[[a, a, z], [], _labels(rng, 2, V, blank)], lens=[4, 3, 1], blank=blank)


def dead_cell(c):
    """an interior cell of row 0: (3, 1) on the ragged shape"""
    return c["lens"][0] // 2, 1


def stored(V, blank, variant, tiny=False):
    c = tiny_base(V, blank) if tiny else stored_base(V, blank)
    x, lens, labels = c["x"].copy(), c["lens"], c["labels"]
    finite, masked = [True, True, True], [0]
    if variant == "class":
        for b in range(3):
            x[b, :lens[b], :len(labels[b]) + 1, masked_class(V)] = NINF
        masked = [0, 1, 2]
    elif variant == "forced":
        x[0, :lens[0] - 1, :len(labels[0]), blank] = NINF
    elif variant == "wall":
        _wall_and_last_blank(x, c, [0])
        finite[0] = False
    elif variant == "last blank":
        x[2, lens[2] - 1, len(labels[2]), blank] = NINF
        finite[2], masked = False, [2]
    elif variant == "dead cell":
        x[0, dead_cell(c)[0], dead_cell(c)[1], :] = NINF
    elif variant == "all rows":
        _wall_and_last_blank(x, c, [0, 1, 2])
        finite, masked = [False, False, False], [0, 1, 2]
    else:
        raise KeyError(variant)
    return dict(c, x=x, finite=finite, masked=masked, name="%s V %d blank %d" % (variant, V, blank))


def without_rows(c, rows):
    """the same case without the rows `rows` (every per-row entry; out, the Dense block, is shared)"""
    keep = [b for b in range(len(c["lens"])) if b not in rows]
    d = dict(c, labels=[c["labels"][b] for b in keep], lens=[c["lens"][b] for b in keep], finite=[c["finite"][b] for b in keep], masked=[])
    for k in ("x", "am", "lm", "enc", "pred"):
        if k in c:
            d[k] = np.ascontiguousarray(c[k][keep])
    return d, keep


# ---- the simple form ----

SB, ST, SML, SLENS, SLL = 3, 9, 4, [9, 5, 2], [4, 0, 2]


def simple_base(V, blank):
    rng = np.random.default_rng(2000 * V + blank)
    labels = [_labels(rng, n, V, blank) for n in SLL]
    return dict(am=rng.uniform(-3, 3, (SB, ST, V)).astype(np.float32), lm=rng.uniform(-3, 3, (SB, SML + 1, V)).astype(np.float32), labels=labels,
                lens=SLENS, blank=blank)


def simple(V, blank, variant):
    c = simple_base(V, blank)
    am, lm, lens, labels = c["am"], c["lm"], c["lens"], c["labels"]
    finite, masked = [True, True, True], [0]

    def block(b):
        if labels[b]:
            lm[b, 1, labels[b][1]] = NINF                   # the wall: label y_2 out of column u = 1, in every frame
        else:
            lm[b, 0, blank] = NINF                          # the last blank (and every blank of the row: it has one column)

    if variant == "class lm":
        for b in range(SB):
            lm[b, :len(labels[b]) + 1, masked_class(V)] = NINF
        masked = [0, 1, 2]
    elif variant == "class am":
        for b in range(SB):
            am[b, [t for t in (1, 2, lens[b] - 1) if t < lens[b]], masked_class(V)] = NINF
        masked = [0, 1, 2]
    elif variant == "forced":
        lm[0, :len(labels[0]), blank] = NINF
    elif variant == "wall":
        block(0)
        finite[0] = False
    elif variant == "last blank":
        lm[2, len(labels[2]), blank] = NINF
        finite[2], masked = False, [2]
    elif variant == "dead cell":
        t, u = SIMPLE_DEAD_CELL
        y = labels[0][u]
        lm[0, u, [v for v in range(V) if v != y]] = NINF    # column u: only its own label is left, in every frame ...
        am[0, t, y] = NINF                                  # ... and frame t takes that one away: cell (t, u) is all -inf, no other is
    elif variant == "dead column":
        lm[0, 2, :] = NINF
        finite[0] = False
    elif variant == "all rows":
        for b in range(SB):
            block(b)
        finite, masked = [False, False, False], [0, 1, 2]
    else:
        raise KeyError(variant)
    return dict(c, finite=finite, masked=masked, name="simple %s V %d blank %d" % (variant, V, blank))


def nan_padded_sum(c):
    """copies of (am, lm) with NaN in the padding, which nothing may look at"""
    am, lm = c["am"].copy(), c["lm"].copy()
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):
        am[b, n:] = np.nan
        lm[b, len(lab) + 1:] = np.nan
    return am, lm


def sum_tensor(c):
    """the float32 broadcast sum am + lm, rounded once: the stored form of a simple case"""
    x = c["am"][:, :, None, :] + c["lm"][:, None, :, :]
    assert x.dtype == np.float32
    return x


# ---- the fused form ----

def fused(variant):
    """wave 0's blocks of V = 300 are the classes [0, 32) and [256, 288), wave 1's [32, 64) and [288, 300); the labels and the blank lie
    outside every masked set (except in `blank masked`), one label in wave 0's second block and one in wave 2's only block"""
    assert FT_COLS == 256 and FUSED_V > FT_COLS + FT_BLOCK and FUSED_V - (FT_COLS + FT_BLOCK) < FT_BLOCK
    J, V, blank = FUSED_J, FUSED_V, FUSED_BLANK
    c = K.fused_ragged(J, V, blank)
    rng = np.random.default_rng(300)
    free = [k for k in range(64, 288) if k != blank]
    pick = lambda n: [free[int(k)] for k in rng.integers(0, len(free), n)]
    a, z, r2 = pick(1)[0], pick(1)[0], pick(5)
    r2[2], r2[3], r2[4] = r2[1], 70, 287
    mask = FUSED_MASKS[variant]
    out = c["out"].copy()
    out[J * V + np.array(mask)] = NINF
    labels = [[a, a, z], [], r2]
    assert variant == "blank masked" or not set(mask) & ({blank} | set(sum(labels, [])))
    dead = variant == "blank masked"
    return dict(c, out=out, labels=labels, mask=mask, finite=[not dead] * 3, masked=[0, 1, 2], kind="tanh", name="fused " + variant)


# ---- the wide form: B = 2, V = 5, T = 6; the forced pattern on one row, the wall on the other ----

def wide(max_label_len):
    """label lengths (300, 600) under max_label_len 600: rnnt_lattice_kernel<0>; (300, 150) under 300: <2>.  Row 0 forced, row 1 walled"""
    V, T, blank = 5, 6, 0
    ll = (300, 600) if max_label_len == 600 else (300, 150)
    assert max(ll) == max_label_len
    rng = np.random.default_rng(max_label_len)
    labels = [K.labels(rng, n, V, blank) for n in ll]
    x = rng.uniform(-2, 2, (2, T, max_label_len + 1, V)).astype(np.float32)
    lens = [T, T - 1]
    x[0, :lens[0] - 1, :ll[0], blank] = NINF
    x[1, :lens[1], 1, labels[1][1]] = NINF
    return dict(x=x, labels=labels, lens=lens, blank=blank, finite=[True, False], masked=[0, 1], name="wide %d" % max_label_len)
