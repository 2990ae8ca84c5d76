"""What the tests of the CTC prefix beam search's label timestamps share (test_ctc_beam_detail_host.py, test_gpu_ctc_beam_detail.py):
the float64 restatement of INTEGRATION.md "Label timestamps and confidences" and the cases, with their premises.

Reference: ``ref_row_detail`` is ctc_reference.ref_row_scaled -- the same candidate cells, merge order, canonical-index tie rule and
range guard -- with a ``frames`` tuple per entry: a plain stay keeps it, a plain extension at frame t appends t, and a merge of entry
j's stay into the extend cell (i, c) compares the extension's p_nb' (LM factor included) with j's stay p_nb' before they are summed:
extension > stay, strictly, replaces the last frame of j by t, anything else keeps j's frames.  Next to it every entry carries
``entered``, what an implementation would report that timed a label at the frame its prefix first entered the beam (a merge never
moves it): the cases must tell the two apart.

Besides the outputs the reference returns what the premises of the cases are stated in: the smallest relative W / W+1 gap of
ctc_reference, the smallest relative gap |ext - stay| / max(ext, stay) over all merges of kept entries (a merge of two exact zeros
decides nothing in either precision and is left out), how many kept merges moved a frame and how many did not, how many kept plain
extensions brought a prefix back that had been in the beam before and left it, and whether a reported hypothesis has a frame that
differs from ``entered``."""
import functools
import math

import numpy as np

from ctc_reference import RANGE_FLOOR, RESCALE_BELOW, softmax

GAP = 1e-3                                            # selection and merge premise of every case: float32 decides as float64 does


def ref_row_detail(p, blank, W, cutoff, walk=None):
    """p [T][C] float64, the row's valid frames -> (the last beam in rank order as (labels, p_b, p_nb, state, frames, entered), stats)"""
    T, Cc = p.shape
    beam = [((), 1.0, 0.0, walk.t["start_state"] if walk else 0, (), ())]
    st = dict(gap=np.inf, merge_gap=np.inf, moved=0, unmoved=0, back=0, k=0)
    nonblank = [c for c in range(Cc) if c != blank]
    was_in = {()}
    for t in range(T):
        pt = p[t]
        if cutoff == 0 or cutoff >= Cc - 1:
            E = nonblank
        else:
            E = sorted(sorted(nonblank, key=lambda c: (-pt[c], c))[:cutoff])
        stays, cand = {}, {}
        for i, (l, pb, pnb, s, fr, en) in enumerate(beam):
            stays[l] = (i * (Cc + 1), (pb + pnb) * pt[blank], pnb * pt[l[-1]] if l else 0.0, s, fr, en, None)
        for i, (l, pb, pnb, s, fr, en) in enumerate(beam):
            for c in E:
                v = pb * pt[c] if (l and c == l[-1]) else (pb + pnb) * pt[c]
                nx = s
                if walk:
                    f, nx = walk(s, c)
                    v = f * v
                lc = l + (c,)
                if lc in stays:
                    _, sb, snb, ss, jfr, jen, _ = stays.pop(lc)
                    assert ss == nx
                    cand[lc] = (i * (Cc + 1) + 1 + c, sb, snb + v, nx, jfr[:-1] + (t,) if v > snb else jfr, jen, ("merge", v, snb))
                else:
                    cand[lc] = (i * (Cc + 1) + 1 + c, 0.0, v, nx, fr + (t,), en + (t,), ("back",) if lc in was_in else None)
        for l, v in stays.items():
            cand[l] = v
        items = sorted(((-(sb + snb), idx, l, sb, snb, s, fr, en, how) for l, (idx, sb, snb, s, fr, en, how) in cand.items()
                        if sb + snb != 0.0), key=lambda x: x[:2])
        if len(items) > W:
            a, b = -items[W - 1][0], -items[W][0]
            st["gap"] = min(st["gap"], (a - b) / a)
        for x in items[:W]:
            how = x[8]
            if how and how[0] == "merge" and max(how[1], how[2]) > 0.0:
                st["merge_gap"] = min(st["merge_gap"], abs(how[1] - how[2]) / max(how[1], how[2]))
                st["moved" if how[1] > how[2] else "unmoved"] += 1
            elif how and how[0] == "back":
                st["back"] += 1
        beam = [x[2:8] for x in items[:W]]
        was_in.update(x[0] for x in beam)
        if beam:
            lo, hi = -items[len(beam) - 1][0], -items[0][0]
            if lo < RESCALE_BELOW:
                e = -math.frexp(hi)[1]
                if e > 0:
                    beam = [(l, math.ldexp(sb, e), math.ldexp(snb, e), s, fr, en) for l, sb, snb, s, fr, en in beam]
                    lo, st["k"] = math.ldexp(lo, e), st["k"] + e
            assert lo >= RANGE_FLOOR, "frame %d: a kept total of %.3g is below 2^-900" % (t, lo)
    return beam, st


def reference(p, lens, blank, W, cutoff, nbest, walk=None, cap=None):
    """-> dict: labels / frames [B][nbest][cap or T] (-1 behind), lengths, logps float32 (0 behind; np.log in float64 of the float32
    probability at the reported frame and label, rounded once), entered (like frames), and the premises' figures over all rows"""
    B, T, _ = p.shape
    cap = T if cap is None else cap
    out = dict(labels=np.full((B, nbest, cap), -1, np.int32), frames=np.full((B, nbest, cap), -1, np.int32),
               entered=np.full((B, nbest, cap), -1, np.int32), logps=np.zeros((B, nbest, cap), np.float32),
               lengths=np.full((B, nbest), -1, np.int32), gap=np.inf, merge_gap=np.inf, moved=0, unmoved=0, back=0, later=0,
               reordered=False)
    for b in range(B):
        beam, st = ref_row_detail(p[b, :lens[b]].astype(np.float64), blank, W, cutoff, walk)
        for key in ("gap", "merge_gap"):
            out[key] = min(out[key], st[key])
        for key in ("moved", "unmoved", "back"):
            out[key] += st[key]
        fin = [(-(pb + pnb) * (walk.final(s) if walk else 1.0), k, l, fr, en) for k, (l, pb, pnb, s, fr, en) in enumerate(beam)]
        fin = sorted((x for x in fin if x[0] != 0.0), key=lambda x: x[:2])
        out["reordered"] |= [x[1] for x in fin[:nbest]] != list(range(min(nbest, len(fin))))
        for k in range(min(nbest, len(fin))):
            _, _, l, fr, en = fin[k]
            m = min(len(l), cap)
            out["labels"][b, k, :m], out["frames"][b, k, :m], out["entered"][b, k, :m] = l[:m], fr[:m], en[:m]
            out["logps"][b, k, :m] = np.log(p[b, list(fr[:m]), list(l[:m])].astype(np.float64)).astype(np.float32)
            out["lengths"][b, k] = len(l)
            out["later"] += sum(f > e for f, e in zip(fr, en))
            if k + 1 < len(fin):
                out["gap"] = min(out["gap"], (fin[k + 1][0] - fin[k][0]) / -fin[k][0])
    return out


# ---- the cases: name -> (posterior seed, B, T, C, W, cutoff, nbest, blank, lengths, LM table seed or None, (row, frame) of a frame of
# zeros or None).  The seeds were searched on this reference alone, per shape, for the premises test_ctc_beam_detail_host.py asserts;
# scale 1.0 keeps the posteriors flat enough for merges in both directions ----
ONE_SHOT = {
    "w1": (0, 4, 24, 5, 1, 0, 1, 0, [24, 0, 17, 9], None, None),
    "w4": (0, 4, 24, 6, 4, 0, 4, 5, [24, 13, 0, 20], None, None),
    "w8": (5, 4, 24, 8, 8, 0, 8, 3, [21, 24, 0, 7], None, None),
    "w8_c7": (1, 4, 24, 7, 8, 0, 8, 0, [24, 24, 0, 11], None, None),
    "class_cut": (11, 4, 24, 12, 8, 3, 8, 11, [24, 0, 19, 24], None, None),
    "lm": (2, 4, 24, 6, 8, 0, 8, 5, [24, 16, 0, 24], 5, None),
    "dead_row": (0, 4, 24, 6, 4, 0, 4, 5, [24, 13, 0, 20], None, (1, 5)),
}
LM_ALPHA, LM_BETA = 1.0, 0.0
SCALE = 1.0
# name, seed, scale, B, T, C, W, cutoff, nbest, blank: the backtrack and the commit stage 8192 / 128 = 64 frames a block and walk from
# the last frame, so the row's blocks are its frames [6, 70) and, after them, [0, 6)
EDGE = ("edge", 2, 6.0, 1, 70, 4, 128, 0, 4, 0)
EDGE_SEAM = 6
STREAM_CASE = "w8_c7"                                  # the one-shot case the stream tests push in chunks, and cut at max_labels = 2


def table_and_walk(Cc, blank, seed):
    """the LM of a case: a dense bigram with final_logp (test_gpu_ctc_beam_lm.py's), and its float64 walk"""
    from test_gpu_ctc_beam_lm import Walk, dense_bigram
    t = dense_bigram(seed, Cc, blank, final=True)
    return t, Walk(t, LM_ALPHA, LM_BETA)


@functools.lru_cache(maxsize=None)
def one_shot_case(name):
    """-> (p, lens, table or None, reference dict); computed once, shared, never changed"""
    seed, B, T, Cc, W, cutoff, nbest, blank, lens, lm_seed, dead = ONE_SHOT[name]
    p = softmax(seed, B, T, Cc, SCALE)
    if dead:
        p[dead[0], dead[1]] = 0.0
    t, walk = table_and_walk(Cc, blank, lm_seed) if lm_seed is not None else (None, None)
    ref = reference(p, lens, blank, W, cutoff, nbest, walk)
    p.setflags(write=False)
    return p, lens, t, ref


@functools.lru_cache(maxsize=None)
def edge_case():
    _, seed, scale, B, T, Cc, W, cutoff, nbest, blank = EDGE
    p = softmax(seed, B, T, Cc, scale)
    ref = reference(p, [T] * B, blank, W, cutoff, nbest)
    p.setflags(write=False)
    return p, ref


def tie_case():
    """C = 2, blank 0, two frames of [0.5, 0.5]: at frame 1 the stay of "a" and the extension of "" are both 0.25 -> the frame stays 0"""
    return np.full((1, 2, 2), 0.5, np.float32)
