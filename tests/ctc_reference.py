"""What the GPU tests of the CTC prefix beam search share (test_gpu_ctc_beam.py, test_gpu_ctc_stream.py, test_gpu_ctc_beam_lm.py): the
float64 restatement of the search's semantics -- the project's only oracle for them -- its tolerances, and the drivers of the one-shot
and the streaming calls.

Reference: ``ref_row`` -- dicts of label tuples, linear space, float64 (which holds these sizes without scaling), the same candidate
cells, merge order and canonical-index tie rule as INTEGRATION.md "CTC prefix beam search".  With a model (``walk``, test_gpu_ctc_beam_lm.py's
Walk): every entry carries an LM state, an extension is multiplied by F(state, c), and after the last frame every total is multiplied by
E(state), zeros are dropped and the rest are ordered again, ties to the lower rank.  Without one every factor is 1.0 and that last step is
the identity."""
import numpy as np
import torch

from nntoolkitcore_amd import layers as NL


def softmax(seed, B, T, Cc, scale=2.0):
    rng = np.random.default_rng(seed)
    z = scale * rng.standard_normal((B, T, Cc))
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def ref_row(p, blank, W, cutoff, walk=None):
    """p [T][C] float64, the row's valid frames; walk None: acoustic only -> (the last beam in rank order as (labels, p_b, p_nb, state),
    the smallest relative W / W+1 gap)"""
    T, Cc = p.shape
    beam = [((), 1.0, 0.0, walk.t["start_state"] if walk else 0)]
    gap = np.inf
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
    return beam, gap


def reference(p, lens, blank, W, cutoff, nbest, walk=None):
    """-> labels [B][nbest][T], lengths, float64 scores, the smallest gap of the premise, whether the end-of-sentence step reordered
    the reported part of some row's beam"""
    B, T, _ = p.shape
    lab, n, sc = np.full((B, nbest, T), -1, np.int32), np.full((B, nbest), -1, np.int32), np.full((B, nbest), -np.inf)
    gap, reordered = np.inf, False
    for b in range(B):
        beam, g = ref_row(p[b, :lens[b]].astype(np.float64), blank, W, cutoff, walk)
        gap = min(gap, g)
        fin = [(-(pb + pnb) * (walk.final(s) if walk else 1.0), k, l) for k, (l, pb, pnb, s) in enumerate(beam)]
        fin = sorted(x for x in fin if x[0] != 0.0)
        reordered |= [k for _, k, _ in fin[:nbest]] != list(range(min(nbest, len(fin))))
        for k in range(min(nbest, len(fin))):
            l = fin[k][2]
            lab[b, k, :len(l)] = l
            n[b, k] = len(l)
            sc[b, k] = np.log(-fin[k][0])
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
