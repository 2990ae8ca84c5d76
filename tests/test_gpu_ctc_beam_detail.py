"""Label timestamps and confidences of the CTC prefix beam search (csrc/hip/ctc_beam.hip, the DETAIL instantiations) on the device:
against the float64 restatement of the rule (ctc_beam_detail_reference.py), against the calls without detail, and the streaming form
against the one-shot call.

Verdicts.  Frames are integers: equal to the reference, exactly -- the premises (test_ctc_beam_detail_host.py: selection gap and merge
gap of every case >= 1e-3, far above the float32 roundings of 24 or 70 frames, 16 * T * 2^-24 <= 6.7e-5) make float32 and float64 take
every decision alike.  label_logps: within one float32 ulp of np.log(p.astype(float64)).astype(float32) at the reported frame and label
-- two libms' double logs may differ in their last bit, which moves the float32 rounding by at most one ulp.  Labels, lengths and score
bits with detail: those of the call without it.  Streams: the bits of the one-shot call with detail, all five outputs, after every
push."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ctc_beam_detail_reference as R
from ctc_reference import chunk as _chunk, decode as _plain
from nntoolkitcore_amd import capi, layers as NL

pytestmark = pytest.mark.gpu


def _lm(t):
    return None if t is None else NL.NgramLm.from_arrays(alpha=R.LM_ALPHA, beta=R.LM_BETA, **t)


def _run(gpu, p, lens, blank, W, cutoff, nbest, lm=None):
    """the one-shot device call with detail on the host array p -> the five outputs as numpy"""
    x = torch.from_numpy(np.array(p)).to(gpu)                               # (a copy: the cases' arrays are read-only)
    if lm is None:
        out = NL.ctc_beam_decode_device(x, lens, blank, W, cutoff, nbest, detail=True)
    else:
        out = NL.ctc_beam_decode_lm_device(x, lm, lens, blank, W, cutoff, nbest, detail=True)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same(got, want, msg=""):
    assert len(got) == len(want) == 5
    for g, w, what in zip(got, want, ("labels", "lengths", "scores", "label_frames", "label_logps")):
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg="%s %s" % (msg, what))


def _against_reference(tag, got, ref, p):
    lab, n, sc, fr, lg = got
    np.testing.assert_array_equal(n, ref["lengths"], err_msg=tag)
    np.testing.assert_array_equal(lab, ref["labels"], err_msg=tag)
    np.testing.assert_array_equal(fr, ref["frames"], err_msg=tag)
    held = lab >= 0
    assert (fr[~held] == -1).all() and (lg.view(np.int32)[~held] == 0).all(), tag         # -1 / +0.0f behind, and in an empty slot
    assert np.isfinite(lg).all(), tag
    ulps = np.abs(lg.view(np.int32).astype(np.int64) - ref["logps"].view(np.int32).astype(np.int64))
    print("%s: %d labels, label_logps off by at most %d ulp" % (tag, int(held.sum()), int(ulps.max(initial=0))))
    assert (ulps <= 1).all(), tag
    # the log-probability is the acoustic one at the reported frame and label
    b, k, q = np.nonzero(held)
    want = np.log(p[b, fr[b, k, q], lab[b, k, q]].astype(np.float64)).astype(np.float32)
    assert (np.abs(lg[b, k, q].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)) <= 1).all(), tag
    # frames never decrease along a hypothesis, and two labels cannot share a frame: strictly increasing
    both = held[..., 1:] & held[..., :-1]
    assert (np.diff(fr.astype(np.int64), axis=-1)[both] > 0).all(), tag


@functools.lru_cache(maxsize=None)
def _one_shot(gpu, name):
    """the device's five outputs on a case, computed once"""
    _, B, T, Cc, W, cutoff, nbest, blank, _, _, _ = R.ONE_SHOT[name]
    p, lens, t, _ = R.one_shot_case(name)
    lm = _lm(t)
    got = _run(gpu, p, lens, blank, W, cutoff, nbest, lm)
    if lm:
        lm.close()
    return got


# ---- bits: detail changes no label, length or score ----
def _raw(gpu, p, lens, blank, W, cutoff, nbest, opts, want_detail):
    """nntk_ctc_beam_decode_opt_device itself; opts: None (o = NULL) or (lm handle, frames?, logps?)"""
    B, T, Cc = p.shape
    L = capi.load()
    x = torch.from_numpy(p).to(gpu)
    lab = torch.full((B, nbest, T), 77, dtype=torch.int32, device=gpu)
    n = torch.full((B, nbest), 77, dtype=torch.int32, device=gpu)
    sc = torch.full((B, nbest), 77.0, dtype=torch.float32, device=gpu)
    fr = torch.full((B, nbest, T), 77, dtype=torch.int32, device=gpu)
    lg = torch.full((B, nbest, T), 77.0, dtype=torch.float32, device=gpu)
    o = None
    if opts is not None:
        o = capi.NntkCtcBeamOptions(opts[0], fr.data_ptr() if opts[1] else None, lg.data_ptr() if opts[2] else None)
    need = L.nntk_ctc_beam_opt_workspace_floats(B, T, Cc, W, cutoff, C.byref(o) if o else None)
    ws = torch.empty(need, dtype=torch.float32, device=gpu)
    il = np.asarray(lens, np.int32)
    rc = L.nntk_ctc_beam_decode_opt_device(x.data_ptr(), B, T, Cc, il.ctypes.data_as(capi.ip), blank, W, cutoff, nbest,
                                           C.byref(o) if o else None, lab.data_ptr(), n.data_ptr(), sc.data_ptr(), ws.data_ptr())
    assert rc == 0, capi.last_error()
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (lab, n, sc, fr, lg))


@pytest.mark.parametrize("name", ["w8", "class_cut", "lm"])
def test_detail_changes_no_label_length_or_score_bit(gpu, name):
    _, B, T, Cc, W, cutoff, nbest, blank, _, _, _ = R.ONE_SHOT[name]
    p, lens, t, _ = R.one_shot_case(name)
    p = np.array(p)
    lm = _lm(t)
    want = _plain(gpu, p, lens, blank, W, cutoff, nbest, lm) if lm else _plain(gpu, p, lens, blank, W, cutoff, nbest)
    full = _one_shot(gpu, name)
    for g, w in zip(full[:3], want):
        np.testing.assert_array_equal(_bits(g), _bits(w))
    h = lm.h if lm else None
    for opts in (None, (None, False, False)) if lm is None else ((h, False, False),):
        got = _raw(gpu, p, lens, blank, W, cutoff, nbest, opts, False)
        for g, w in zip(got[:3], want):
            np.testing.assert_array_equal(_bits(g), _bits(w))
        assert (got[3] == 77).all() and (got[4] == 77.0).all()             # nothing asked for, nothing written
    # either output alone: the same bits, the other untouched
    only_fr = _raw(gpu, p, lens, blank, W, cutoff, nbest, (h, True, False), True)
    only_lg = _raw(gpu, p, lens, blank, W, cutoff, nbest, (h, False, True), True)
    _same(only_fr[:4] + (full[4],), full)
    _same(only_lg[:3] + (full[3], only_lg[4]), full)
    assert (only_fr[4] == 77.0).all() and (only_lg[3] == 77).all()
    if lm:
        lm.close()


# ---- one-shot against the reference ----
@pytest.mark.parametrize("name", list(R.ONE_SHOT))
def test_one_shot_equals_the_reference(gpu, name):
    p, lens, t, ref = R.one_shot_case(name)
    got = _one_shot(gpu, name)
    _against_reference(name, got, ref, p)
    dead = R.ONE_SHOT[name][10]
    if dead:
        assert (got[3][dead[0]] == -1).all() and (got[4][dead[0]].view(np.int32) == 0).all() and (got[1][dead[0]] == -1).all()
    assert (got[3][np.asarray(lens) == 0] == -1).all()                      # input_length 0: the empty prefix, no label, no frame


def test_the_exact_tie_keeps_the_frame(gpu):
    p = R.tie_case()
    lab, n, sc, fr, lg = _run(gpu, p, [2], 0, 2, 0, 2)
    assert lab[0, 0].tolist() == [1, -1] and n[0, 0] == 1
    assert fr[0, 0].tolist() == [0, -1]
    assert lg[0, 0, 0] == np.float32(np.log(0.5)) and lg[0, 0, 1] == 0.0
    _against_reference("tie", (lab, n, sc, fr, lg), R.reference(p, [2], 0, 2, 0, 2), p)


def test_backtrack_across_the_block_edge(gpu):
    """W = 128, T = 70: the backtrack stages frames [6, 70), then [0, 6); the mark of a merge lies in the one, its position's extension
    record in the other (the premises: test_ctc_beam_detail_host.py)"""
    _, seed, scale, B, T, Cc, W, cutoff, nbest, blank = R.EDGE
    p, ref = R.edge_case()
    _against_reference("edge", _run(gpu, p, [T], blank, W, cutoff, nbest), ref, p)


# ---- streams: the one-shot call's bits after every push ----
def _push(gpu, dec, p, pos, n, final=None):
    x = torch.from_numpy(_chunk(p, pos, n, dec.T)).to(gpu)
    out = dec.push(x, n, final)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _cut(out, L):
    """a one-shot result as a stream with max_labels = L reports it"""
    lab, n, sc, fr, lg = out
    return lab[..., :L], n, sc, fr[..., :L], lg[..., :L]


def _stream_against_one_shot(gpu, name, pushes, max_frames, max_labels=None):
    _, B, T, Cc, W, cutoff, nbest, blank, _, _, _ = R.ONE_SHOT[name]
    p, lens, t, _ = R.one_shot_case(name)
    p = np.array(p)
    for b in range(B):
        p[b, lens[b]:] = np.nan
    lm = _lm(t)
    dec = NL.CtcBeamStream(B, max_frames, Cc, blank, W, cutoff, nbest, max_labels=T if max_labels is None else max_labels, lm=lm, detail=True)
    pos = [0] * B
    for i, n in enumerate(pushes):
        got = _push(gpu, dec, p, pos, n)
        pos = [a + b for a, b in zip(pos, n)]
        want = _run(gpu, p, pos, blank, W, cutoff, nbest, lm)
        _same(got, _cut(want, dec.max_labels), "%s push %d" % (name, i))
    assert pos == list(lens)
    dec.close()
    if lm:
        lm.close()
    return got


def _frame_by_frame(lens):
    return [[1 if i < l else 0 for l in lens] for i in range(max(lens))]


def _ragged(lens, sizes):
    out, pos = [], [0] * len(lens)
    for i in range(200):
        n = [min(sizes[(i + b) % len(sizes)], l - q) for b, (l, q) in enumerate(zip(lens, pos))]
        if not any(n) and pos == list(lens):
            break
        out.append(n)
        pos = [a + b for a, b in zip(pos, n)]
    return out


@pytest.mark.parametrize("name", [R.STREAM_CASE, "lm"])
@pytest.mark.parametrize("how", ["frame_by_frame", "ragged"])
def test_stream_has_the_one_shot_bits_after_every_push(gpu, name, how):
    lens = R.ONE_SHOT[name][8]
    pushes = _frame_by_frame(lens) if how == "frame_by_frame" else _ragged(lens, [5, 0, 3, 7])
    assert any(0 in n and any(n) for n in pushes)                          # a push with n_frames[b] == 0 next to rows with frames
    got = _stream_against_one_shot(gpu, name, pushes, 8)
    _against_reference(name + " streamed", got, R.one_shot_case(name)[3], R.one_shot_case(name)[0])


@pytest.mark.parametrize("name", [R.STREAM_CASE, "lm"])
def test_stream_cut_at_two_labels(gpu, name):
    """max_labels = 2 on rows that grow past it: labels, frames and log-probabilities are cut alike, the length stays true, a move at
    position 1 applies and one at position 2 is dropped -- in later pushes than the ones that made the labels.  "lm": the same through
    the commit's report by slot, on a beam that the end-of-sentence step reorders"""
    _, B, T, Cc, W, cutoff, nbest, blank, lens, lm_seed, _ = R.ONE_SHOT[name]
    got = _stream_against_one_shot(gpu, name, _frame_by_frame(lens), 4, max_labels=2)
    p, _, _, ref = R.one_shot_case(name)
    assert got[0].shape[-1] == 2 and (got[1] > 2).any()
    np.testing.assert_array_equal(got[1], ref["lengths"])
    np.testing.assert_array_equal(got[3], ref["frames"][..., :2])
    np.testing.assert_array_equal(got[0], ref["labels"][..., :2])
    walk = R.table_and_walk(Cc, blank, lm_seed)[1] if lm_seed is not None else None
    cut = R.reference(p, lens, blank, W, cutoff, nbest, walk, cap=2)
    assert cut["reordered"] == (name == "lm") and min(cut["gap"], cut["merge_gap"]) >= R.GAP
    _against_reference(name + " cut at 2", got, cut, p)


def test_final_and_reset_restart_the_frame_count(gpu):
    name = R.STREAM_CASE
    _, B, T, Cc, W, cutoff, nbest, blank, _, _, _ = R.ONE_SHOT[name]
    p = np.array(R.one_shot_case(name)[0])
    dec = NL.CtcBeamStream(B, 12, Cc, blank, W, cutoff, nbest, max_labels=T, detail=True)
    first = _push(gpu, dec, p, [0] * B, [12, 9, 0, 5], final=[1, 0, 0, 0])
    _same(first, _run(gpu, p, [12, 9, 0, 5], blank, W, cutoff, nbest), "first push")
    dec.reset([3])
    # row 0 (final) and row 3 (reset) start over at frame 0 of what they are given; row 1 goes on from frame 9
    got = _push(gpu, dec, p, [12, 9, 0, 7], [12, 12, 0, 4])
    q = np.array(p)
    q[0, :12], q[3, :4] = p[0, 12:24], p[3, 7:11]
    want = _run(gpu, q, [12, 21, 0, 4], blank, W, cutoff, nbest)
    _same(got, want, "second push")
    assert got[3][0].max() < 12 and got[3][3].max() < 4 and got[3][1].max() >= 12
    dec.close()


def test_commit_across_the_block_edge(gpu):
    """the 70-frame push of the W = 128 case: the commit kernel stages two blocks"""
    _, seed, scale, B, T, Cc, W, cutoff, nbest, blank = R.EDGE
    p, ref = R.edge_case()
    p = np.array(p)
    dec = NL.CtcBeamStream(B, T, Cc, blank, W, cutoff, nbest, max_labels=T, detail=True)
    got = _push(gpu, dec, p, [0], [T])
    _same(got, _run(gpu, p, [T], blank, W, cutoff, nbest), "one push")
    _against_reference("edge, one push", got, ref, p)
    # and pushed in two: a mark of the second push for a label the first push made
    dec.reset([0])
    _push(gpu, dec, p, [0], [R.EDGE_SEAM])
    got = _push(gpu, dec, p, [R.EDGE_SEAM], [T - R.EDGE_SEAM])
    _against_reference("edge, two pushes", got, ref, p)
    dec.close()


# ---- determinism, independence, the host forms ----
def test_same_bits_every_call_and_rows_do_not_see_each_other(gpu):
    name = "w8"
    _, B, T, Cc, W, cutoff, nbest, blank, _, _, _ = R.ONE_SHOT[name]
    p, lens, _, _ = R.one_shot_case(name)
    p = np.array(p)
    first = _one_shot(gpu, name)
    _same(_run(gpu, p, lens, blank, W, cutoff, nbest), first, "second call")
    q = np.array(p)
    for b in range(B):
        q[b, lens[b]:] = np.nan
    _same(_run(gpu, q, lens, blank, W, cutoff, nbest), first, "NaN in the padding")
    for b in range(B):
        alone = _run(gpu, q[b:b + 1], lens[b:b + 1], blank, W, cutoff, nbest)
        _same(alone, tuple(a[b:b + 1] for a in first), "row %d alone" % b)


def test_host_forms(gpu):
    name = R.STREAM_CASE
    _, B, T, Cc, W, cutoff, nbest, blank, _, _, _ = R.ONE_SHOT[name]
    p, lens, _, _ = R.one_shot_case(name)
    p = np.array(p)
    want = _one_shot(gpu, name)
    _same(NL.ctc_beam_decode(p, lens, blank, W, cutoff, nbest, detail=True), want, "ctc_beam_decode")
    _same(NL.ctc_beam_decode_lm(p, None, lens, blank, W, cutoff, nbest, detail=True), want, "ctc_beam_decode_lm")
    assert len(NL.ctc_beam_decode(p, lens, blank, W, cutoff, nbest)) == 3
    dec = NL.CtcBeamStream(B, T, Cc, blank, W, cutoff, nbest, detail=True)
    _same(dec.push_host(p, lens), want, "push_host")
    dec.close()
