"""The one home of what the transducer loss / alignment tests share (a helper, no test; numpy only): the random cases of the stored and
the fused form, the tolerance constants, the mirrored constants that pick a lattice kernel, and the refusal table of the three host test
files with its per-call additions.

Conventions (tests/rnnt_reference.py): a stored case is dict(x [B][T][U1][V], labels, lens, blank), a fused case dict(enc [B][T][J],
pred [B][U1][J], out = W [J,V] | b [V], labels, lens, blank); cells with t >= lens[b] or u > len(labels[b]) are padding."""
import ctypes as C

import numpy as np

# the device's error against float64 is at most FACTOR x the error of a float32 torch restatement, or FLOOR where that is smaller
FACTOR = 4.0
FLOOR = 16 * 2.0 ** -24

# the constants of rnnt.hip / rnnt_align.hip that decide the path, mirrored so that a moved threshold turns the premise assertions red
CTC_THREADS, LDS_OPT_IN = 256, 48 * 1024


def lattice_path(max_label_len):
    """(NJ of the rnnt_lattice_kernel / rnnt_viterbi_kernel instantiation, its LDS request in bytes: above LDS_OPT_IN it needs the opt-in)"""
    u1 = max_label_len + 1
    return (1 if u1 <= CTC_THREADS else 2 if u1 <= 2 * CTC_THREADS else 0), 2 * u1 * 16


def labels(rng, n, V, blank):
    classes = [k for k in range(V) if k != blank]
    return [classes[int(k)] for k in rng.integers(0, len(classes), n)]


def ragged(V, blank):
    """stored form: batch 3, T = 7 with lengths (7, 4, 1), max_label_len 5 with label lengths (3, 0, 5)"""
    rng = np.random.default_rng(sum(map(ord, "ragged_%d_%d" % (V, blank))))
    a, c = labels(rng, 2, V, blank)[0], labels(rng, 5, V, blank)
    c[2] = c[1]                                       # (row 2 repeats a label where V allows a choice at all; row 0 always does)
    return dict(x=rng.uniform(-3, 3, (3, 7, 6, V)).astype(np.float32), labels=[[a, a, labels(rng, 1, V, blank)[0]], [], c],
                lens=[7, 4, 1], blank=blank)


def fused_ragged(J, V, blank, seed=0):
    """fused form, the lengths of ragged: input lengths 7 / 4 / 1 of T = 7, label lengths 3 / 0 / 5 of max_label_len 5"""
    rng = np.random.default_rng(1000 * J + V + 7 * blank + seed)
    a, c = labels(rng, 1, V, blank)[0], labels(rng, 5, V, blank)
    c[2] = c[1]
    if blank != V - 1:
        c[4] = V - 1                                  # a label in the last (partial) block of V
    sc = 1.0 / np.sqrt(J)
    return dict(enc=rng.uniform(-1.5, 1.5, (3, 7, J)).astype(np.float32), pred=rng.uniform(-1.5, 1.5, (3, 6, J)).astype(np.float32),
                out=np.concatenate([rng.uniform(-3 * sc, 3 * sc, J * V), rng.uniform(-1, 1, V)]).astype(np.float32),
                labels=[[a, a, labels(rng, 1, V, blank)[0]], [], c], lens=[7, 4, 1], blank=blank)


def fused_single(T, U, J, V, blank, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return dict(enc=rng.uniform(-1, 1, (1, T, J)).astype(np.float32), pred=rng.uniform(-1, 1, (1, U + 1, J)).astype(np.float32),
                out=rng.uniform(-scale, scale, J * V + V).astype(np.float32), labels=[labels(rng, U, V, blank)], lens=[T], blank=blank)


def with_nan_padding(c):
    """copies with NaN in the padding, which nothing may look at: x of a stored case, (enc, pred) of a fused one"""
    if "x" in c:
        x = c["x"].copy()
        for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):
            x[b, n:] = np.nan
            x[b, :, len(lab) + 1:] = np.nan
        return x
    enc, pred = c["enc"].copy(), c["pred"].copy()
    for b, (n, lab) in enumerate(zip(c["lens"], c["labels"])):
        enc[b, n:] = np.nan
        pred[b, len(lab) + 1:] = np.nan
    return enc, pred


# ---- refusals: a good call with dummy device pointers (a call that got past the checks would fault, a refusal never looks at them),
#      and rows (name, what changes, a word of the message).  BAD holds for every loss and alignment entry; the lists after it are the
#      additions of single calls ----

GOOD = dict(B=2, T=6, J=8, V=5, ML=3, act=1, il=[6, 4], lab=[[1, 2, 0], [3, 0, 0]], ll=[2, 1], blank=4,
            x=0x100000, enc=0x100000, pred=0x200000, out=0x300000, loss=0x400000, g=0x500000, denc=0x500000, dpred=0x600000, dout=0x700000,
            lf=0x400000, fl=0x410000, lp=0x420000, fp=0x430000, sc=0x440000, ws=0x800000)
BAD = [("input length > T", dict(il=[7, 4]), "input_lengths"), ("input length 0", dict(il=[6, 0]), "input_lengths"),
       ("input length < 0", dict(il=[6, -1]), "input_lengths"), ("label length > max", dict(ll=[4, 1]), "label_lengths"),
       ("label length < 0", dict(ll=[2, -1]), "label_lengths"), ("label is the blank", dict(lab=[[1, 4, 0], [3, 0, 0]]), "blank"),
       ("label >= V", dict(lab=[[1, 5, 0], [3, 0, 0]]), "not a class"), ("label < 0", dict(lab=[[-1, 2, 0], [3, 0, 0]]), "not a class"),
       ("blank >= V", dict(blank=5), "blank"), ("blank < 0", dict(blank=-1), "blank"), ("V = 1", dict(V=1, blank=0), "V 1"),
       ("V = 0", dict(V=0, blank=0), "V 0"), ("batch < 0", dict(B=-1), "negative"),
       ("NULL labels", dict(lab=None), "NULL"), ("NULL label lengths", dict(ll=None), "NULL"),
       ("max_label_len beyond the limit", dict(ML=4001, lab=np.zeros((2, 4001), np.int32), ll=[0, 0]), "max_label_len"),
       ("T + max_label_len beyond the limit", dict(T=65536 - 2, il=None), "diagonals")]
WS_BAD = [("NULL workspace", dict(ws=None), "NULL"), ("misaligned workspace", dict(ws=0x800004), "aligned")]      # every device form
PLAIN_ONLY = [("NULL logits", dict(x=None), "NULL"), ("misaligned logits", dict(x=0x100004), "aligned")]           # stored scores
FUSED_ONLY = [("activation 3", dict(act=3), "activation"), ("activation -1", dict(act=-1), "activation"), ("J = 0", dict(J=0), "J 0"),
              ("J < 0", dict(J=-4), "J"), ("J above the limit", dict(J=1025), "J 1025"), ("V above the limit", dict(V=8193), "V 8193"),
              ("NULL enc", dict(enc=None), "NULL"), ("NULL pred", dict(pred=None), "NULL"), ("NULL out", dict(out=None), "NULL")]
LOSS_ONLY = [("NULL loss", dict(loss=None), "NULL"), ("misaligned gradient", dict(g=0x500008), "aligned"),
             ("misaligned loss", dict(loss=0x400002), "aligned"), ("gradient overlaps the logits", dict(g=0x100000 + 16), "overlaps")]
FUSED_LOSS_ONLY = [("only d_denc", dict(dpred=None, dout=None), "all NULL or all given"),
                   ("d_dout missing", dict(dout=None), "all NULL or all given"), ("d_denc missing", dict(denc=None), "all NULL or all given"),
                   ("NULL loss", dict(loss=None), "NULL"), ("misaligned enc", dict(enc=0x100002), "aligned"),
                   ("d_denc overlaps d_enc", dict(denc=0x100000 + 16), "overlaps"), ("d_dpred overlaps d_denc", dict(dpred=0x500000 + 64), "overlaps"),
                   ("d_dout overlaps d_out", dict(dout=0x300000), "overlaps"), ("d_dout overlaps the workspace", dict(dout=0x800000 + 32), "overlaps"),
                   ("loss overlaps d_pred", dict(loss=0x200000 + 8), "overlaps"), ("d_denc overlaps the loss", dict(denc=0x400000 - 16), "overlaps")]
ALIGN_ONLY = [("NULL scores", dict(sc=None), "NULL"), ("misaligned label_frames", dict(lf=0x400002), "aligned"),
              ("label_frames overlaps frame_labels", dict(lf=0x410000 + 8), "overlaps"), ("scores overlaps label_logp", dict(sc=0x420000 + 4), "overlaps"),
              ("frame_logp overlaps the workspace", dict(fp=0x800000 + 64), "overlaps"), ("frame_labels overlaps the input", dict(fl=0x100000 + 16), "overlaps")]
FUSED_ALIGN_ONLY = [("misaligned pred", dict(pred=0x200002), "aligned"), ("scores overlaps d_out", dict(sc=0x300000 + 4), "overlaps")]


def ids(rows):
    return [r[0] for r in rows]


def ints(a):
    """a host int array as the C entries take it, None for None"""
    from nntoolkitcore_amd import capi
    return None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(capi.ip)


def ptr(v):
    return None if v is None else C.c_void_p(v)
