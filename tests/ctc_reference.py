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
With a model (``walk``, test_gpu_ctc_beam_lm.py's Walk): every entry carries an LM state, an extension is multiplied by F(state, c), and after the last frame every total is multiplied by
E(state), zeros are dropped and the rest are ordered again, ties to the lower rank.  Without one every factor is 1.0 and that last step is
the identity."""
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


def ref_row_scaled(p, blank, W, cutoff, walk=None):
    """ref_row for any length -> (beam, gap, k, floor): the true masses are the beam's times 2^-k; floor = the smallest non-zero total
    a frame kept, as it stood (after that frame's rescaling) when the range guard looked at it"""
    T, Cc = p.shape
    beam = [((), 1.0, 0.0, walk.t["start_state"] if walk else 0)]
    gap, k, floor = np.inf, 0, np.inf
    nonblank = [c for c in range(Cc) if c != blank]
    for t in range(T):
        pt = p[t]
        if cutoff == 0 or cutoff >= Cc - 1:
            E = nonblank
        else:
            E = sorted(sorted(nonblank, key=lambda c: (-pt[c], c))[:cutoff])
        stays, cand = {}, {}
        for i, (l, pb, pnb, s) in enumerate(beam):
            stays[l] = (i * (Cc + 1), (pb + pnb) * pt[blank], pnb * pt[l[-1]] if l else 0.0, s)
        for i, (l, pb, pnb, s) in enumerate(beam):
            for c in E:
                v = pb * pt[c] if (l and c == l[-1]) else (pb + pnb) * pt[c]
                nx = s
                if walk:
                    f, nx = walk(s, c)
                    v = f * v
                lc = l + (c,)
                if lc in stays:
                    _, sb, snb, ss = stays.pop(lc)
                    assert ss == nx
                    cand[lc] = (i * (Cc + 1) + 1 + c, sb, snb + v, nx)
                else:
                    cand[lc] = (i * (Cc + 1) + 1 + c, 0.0, v, nx)
        for l, v in stays.items():
            cand[l] = v
        items = sorted(((-(sb + snb), idx, l, sb, snb, s) for l, (idx, sb, snb, s) in cand.items() if sb + snb != 0.0))
        if len(items) > W:
            a, b = -items[W - 1][0], -items[W][0]
            gap = min(gap, (a - b) / a)
        beam = [(l, sb, snb, s) for _, _, l, sb, snb, s in items[:W]]
        if beam:
            lo, hi = -items[len(beam) - 1][0], -items[0][0]
            if lo < RESCALE_BELOW:
                e = -math.frexp(hi)[1]
                if e > 0:
                    beam = [(l, math.ldexp(sb, e), math.ldexp(snb, e), s) for l, sb, snb, s in beam]
                    lo, k = math.ldexp(lo, e), k + e
            assert lo >= RANGE_FLOOR, "frame %d: a kept total of %.3g is below 2^-900" % (t, lo)
            floor = min(floor, lo)
    return beam, gap, k, floor


def reference(p, lens, blank, W, cutoff, nbest, walk=None):
    """-> labels [B][nbest][T], lengths, float64 scores, the smallest gap of the premise, whether the end-of-sentence step reordered
    the reported part of some row's beam"""
    B, T, _ = p.shape
    lab, n, sc = np.full((B, nbest, T), -1, np.int32), np.full((B, nbest), -1, np.int32), np.full((B, nbest), -np.inf)
    gap, reordered = np.inf, False
    for b in range(B):
        beam, g, k2, _ = ref_row_scaled(p[b, :lens[b]].astype(np.float64), blank, W, cutoff, walk)
        gap = min(gap, g)
        fin = [(-(pb + pnb) * (walk.final(s) if walk else 1.0), k, l) for k, (l, pb, pnb, s) in enumerate(beam)]
        fin = sorted(x for x in fin if x[0] != 0.0)
        reordered |= [k for _, k, _ in fin[:nbest]] != list(range(min(nbest, len(fin))))
        for k in range(min(nbest, len(fin))):
            l = fin[k][2]
            lab[b, k, :len(l)] = l
            n[b, k] = len(l)
            sc[b, k] = np.log(-fin[k][0]) - k2 * _LN2 if k2 else np.log(-fin[k][0])
            if k + 1 < len(fin):
                gap = min(gap, (fin[k + 1][0] - fin[k][0]) / -fin[k][0])
    return lab, n, sc, gap, reordered


def tol(T, ref):
    """the acoustic search's score tolerance (test_gpu_ctc_beam.py's module text)"""
    return 8 * T * 2.0 ** -24 + 4 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def tol_lm(rounds, ref):
    """the fused search's, from its count of roundings (test_gpu_ctc_beam_lm.py's module text)"""
    return 2 * rounds * 2.0 ** -24 + 4 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


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
