"""What the GPU tests of the CTC prefix beam search share (test_gpu_ctc_beam.py, test_gpu_ctc_stream.py, test_gpu_ctc_beam_lm.py): the
float64 restatement of the search's semantics -- the project's only oracle for them -- its tolerances, and the drivers of the one-shot
and the streaming calls.

Reference: ``ref_row`` -- dicts of label tuples, linear space, float64, the same candidate cells, merge order and canonical-index tie
rule as INTEGRATION.md "CTC prefix beam search".  Range: float64 holds the small cases without scaling, and that is checked, not
assumed: after every frame the smallest non-zero total the beam keeps must be at least RANGE_FLOOR = 2^-900 (``ref_row_scaled``).  A
row that would fall below RESCALE_BELOW = 2^-512 has its whole beam multiplied by the power of two that brings its largest total into
[0.5, 1) -- exact, so no comparison, no mantissa and no relative gap changes -- and the exponent is carried into the score.  A kept
entry's smaller part (p_b or p_nb) may lie below its total, but a part that later yields a kept candidate on its own is then itself
a kept total, so it was never below the floor: what could go denormal (more than 2^-122 below its total) never decides anything.
With a model (``walk``, ngram_cases.py's Walk): every entry carries an LM state, an extension is multiplied by F(state, c), and after
the last frame every total is multiplied by E(state), zeros are dropped and the rest are ordered again, ties to the lower rank.  Without
one every factor is 1.0 and that last step is the identity.

Label timestamps (INTEGRATION.md "Label timestamps and confidences"; the cases are ctc_beam_detail_reference.py's).  Every entry of
the same search carries a ``frames`` tuple: a plain stay keeps it, a plain extension at frame t appends t, and a merge of entry j's
stay into the extend cell (i, c) compares the extension's p_nb' (LM factor included) with j's stay p_nb' before they are summed:
extension > stay, strictly, replaces the last frame of j by t, anything else keeps j's frames.  Next to it every entry carries
``entered``, what an implementation would report that timed a label at the frame its prefix first entered the beam (a merge never
moves it).  The figures the premises are stated in: ``gap`` as above; ``merge_gap``, the smallest relative gap |ext - stay| /
max(ext, stay) over all merges of kept entries (a merge of two exact zeros decides nothing in either precision and is left out);
``moved`` / ``unmoved``, how many kept merges moved a frame and how many did not; ``back``, how many kept plain extensions brought a
prefix back that had been in the beam before and left it; ``later``, how many reported frames differ from ``entered``."""
import math

import numpy as np
import torch

from nntoolkitcore_amd import layers as NL


_LN2 = 0.69314718055994530942


def softmax(seed, B, T, Cc, scale=2.0):
    rng = np.random.default_rng(seed)
    z = scale * rng.standard_normal((B, T, Cc))
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


RANGE_FLOOR = 2.0 ** -900                             # no kept total below it: far from the denormals (2^-1022)
RESCALE_BELOW = 2.0 ** -512                           # no case of T <= 64 frames comes near it: those are never rescaled


def ref_row(p, blank, W, cutoff, walk=None):
    """p [T][C] float64, the row's valid frames; walk None: acoustic only -> (the last beam in rank order as (labels, p_b, p_nb, state),
    the smallest relative W / W+1 gap).  For rows that need no rescaling (asserted)."""
    beam, gap, k, _ = ref_row_scaled(p, blank, W, cutoff, walk)
    assert k == 0, "this row was rescaled: take its masses from ref_row_scaled"
    return beam, gap


def ref_row_scaled(p, blank, W, cutoff, walk=None, detail=False):
    """ref_row for any length.  detail: -> (the last beam in rank order as (labels, p_b, p_nb, state, frames, entered), st), st = dict of
    gap, merge_gap, moved, unmoved, back (the module text), k (the true masses are the beam's times 2^-k) and floor (the smallest
    non-zero total a frame kept, as it stood, after that frame's rescaling, when the range guard looked at it).  Else the projection
    (beam of (labels, p_b, p_nb, state), gap, k, floor)."""
    T, Cc = p.shape
    beam = [((), 1.0, 0.0, walk.t["start_state"] if walk else 0, (), ())]
    st = dict(gap=np.inf, merge_gap=np.inf, moved=0, unmoved=0, back=0, k=0, floor=np.inf)
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
            st["floor"] = min(st["floor"], lo)
    return (beam, st) if detail else ([x[:4] for x in beam], st["gap"], st["k"], st["floor"])


def reference_detail(p, lens, blank, W, cutoff, nbest, walk=None, cap=None):
    """-> dict: labels / frames [B][nbest][cap or T] (-1 behind), lengths, float64 scores, logps float32 (0 behind; np.log in float64
    of the float32 probability at the reported frame and label, rounded once), entered (like frames), and the premises' figures over
    all rows: gap, merge_gap, moved, unmoved, back, later, and whether the end-of-sentence step reordered the reported part of some
    row's beam"""
    B, T, _ = p.shape
    cap = T if cap is None else cap
    out = dict(labels=np.full((B, nbest, cap), -1, np.int32), frames=np.full((B, nbest, cap), -1, np.int32),
               entered=np.full((B, nbest, cap), -1, np.int32), logps=np.zeros((B, nbest, cap), np.float32),
               lengths=np.full((B, nbest), -1, np.int32), scores=np.full((B, nbest), -np.inf), gap=np.inf, merge_gap=np.inf, moved=0,
               unmoved=0, back=0, later=0, reordered=False)
    for b in range(B):
        beam, st = ref_row_scaled(p[b, :lens[b]].astype(np.float64), blank, W, cutoff, walk, detail=True)
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
            out["scores"][b, k] = np.log(-fin[k][0]) - st["k"] * _LN2 if st["k"] else np.log(-fin[k][0])
            out["later"] += sum(f > e for f, e in zip(fr, en))
            if k + 1 < len(fin):
                out["gap"] = min(out["gap"], (fin[k + 1][0] - fin[k][0]) / -fin[k][0])
    return out


def reference(p, lens, blank, W, cutoff, nbest, walk=None):
    """-> labels [B][nbest][T], lengths, float64 scores, the smallest gap of the premise, whether the end-of-sentence step reordered
    the reported part of some row's beam"""
    r = reference_detail(p, lens, blank, W, cutoff, nbest, walk)
    return r["labels"], r["lengths"], r["scores"], r["gap"], r["reordered"]


def tol(T, ref):
    """the acoustic search's score tolerance (test_gpu_ctc_beam.py's module text)"""
    return 8 * T * 2.0 ** -24 + 4 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def tol_lm(rounds, ref):
    """the fused search's, from its count of roundings (test_gpu_ctc_beam_lm.py's module text)"""
    return 2 * rounds * 2.0 ** -24 + 4 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def rounds(T, D):
    """the float32 roundings a reported total of the fused search carries at most (test_gpu_ctc_beam_lm.py's module text)"""
    return (4 + 2 * D + 2) * T + 2


def assert_scores(tag, n, got, ref, allow=tol):
    """-inf exactly where the reference has it, else within allow(n, ref): tol with n = T, or tol_lm with n = rounds(T, D)"""
    fin = np.isfinite(ref)
    np.testing.assert_array_equal(np.isneginf(got), ~fin, err_msg=tag)
    err = np.abs(got[fin].astype(np.float64) - ref[fin])
    print("%s: largest score error %.3g of %.3g allowed" % (tag, err.max(initial=0.0), allow(n, ref[fin]).min(initial=np.inf)))
    assert (err <= allow(n, ref[fin])).all(), tag


def ctc_loss64(p, labels, blank):
    """float64 CTC loss of one labelling on the row p [T][C], torch on the CPU"""
    lp = torch.log(torch.from_numpy(p.astype(np.float64)))[:, None, :]
    tgt = torch.tensor([list(labels) or [0]], dtype=torch.long)
    loss = torch.nn.functional.ctc_loss(lp, tgt, torch.tensor([p.shape[0]]), torch.tensor([len(labels)]), blank=blank, reduction="none")
    return float(loss[0])


def decode(gpu, p, lens, blank, W, cutoff, nbest, *lm):
    """the one-shot device call on the host array p, downloaded: ctc_beam_decode_device, or with one more argument (an NgramLm or
    None) ctc_beam_decode_lm_device"""
    x = torch.from_numpy(p).to(gpu)
    if lm:
        out = NL.ctc_beam_decode_lm_device(x, lm[0], lens, blank, W, cutoff, nbest)
    else:
        out = NL.ctc_beam_decode_device(x, lens, blank, W, cutoff, nbest)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def eq(got, want, msg=""):
    np.testing.assert_array_equal(got[1], want[1], err_msg=msg)
    np.testing.assert_array_equal(got[0], want[0], err_msg=msg)
    np.testing.assert_array_equal(got[2].view(np.int32), want[2].view(np.int32), err_msg=msg)


def chunk(p, pos, n, max_frames):
    """the block of one push: row b's next n[b] frames, NaN behind them"""
    B, _, Cc = p.shape
    x = np.full((B, max_frames, Cc), np.nan, np.float32)
    for b in range(B):
        x[b, :n[b]] = p[b, pos[b]:pos[b] + n[b]]
    return x


def drive(gpu, dec, p, pushes, max_frames, pos=None, finals=None, after=None):
    """push the rows of p through dec: pushes = one [B] list of frame counts per push.  Returns the last push's outputs as numpy."""
    B = p.shape[0]
    pos = [0] * B if pos is None else pos
    got = None
    for i, n in enumerate(pushes):
        x = torch.from_numpy(chunk(p, pos, n, max_frames)).to(gpu)
        out = dec.push(x, n, None if finals is None else finals[i])
        torch.cuda.synchronize()
        got = tuple(t.cpu().numpy() for t in out)
        for b in range(B):
            pos[b] += n[b]
        if after is not None:
            after(i, list(pos), got)
    return got
