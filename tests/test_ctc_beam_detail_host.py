"""Label timestamps of the CTC prefix beam search: what can be checked without a device.

1. The premises of test_gpu_ctc_beam_detail.py's cases, on the float64 reference alone (ctc_beam_detail_reference.py).  Every case keeps
   the selection gap of the beam-search tests and the new merge gap at 1e-3 or more, so that float32 and float64 take every selection
   and every merge decision alike; the set as a whole has merges that move a frame and merges that do not, a reported label timed later
   than the frame its prefix first entered the beam (an implementation reporting THAT frame fails the GPU cases), and a prefix that left
   the beam and was extended back in.  The block-edge case has a label timed before the seam of the two staged blocks next to a
   position moved behind it, and a position whose extension record lies before the seam and whose moving merge lies behind it.
2. The exact tie: C = 2, blank 0, two frames of [0.5, 0.5].  At frame 1 the stay of "a" and the extension of "" are both 0.25: the
   frame stays 0.
3. The refusals of the option form that need no device, the sizes, and that every new name is declared, exported and bound."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ctc_beam_detail_reference as R
from nntoolkitcore_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["nntk_ctc_beam_opt_workspace_floats", "nntk_ctc_beam_decode_opt_device", "nntk_ctc_beam_decode_opt",
       "nntk_ctc_beam_stream_create_opt", "nntk_ctc_beam_stream_state_bytes_opt", "nntk_ctc_beam_stream_push_opt_device",
       "nntk_ctc_beam_stream_push_opt"]


# ---- 1: premises ----
@pytest.mark.parametrize("name", list(R.ONE_SHOT))
def test_case_premises(name):
    _, B, T, Cc, W, cutoff, nbest, blank, lens, lm_seed, dead = R.ONE_SHOT[name]
    p, lens, t, ref = R.one_shot_case(name)
    print("%s: selection gap %.3g, merge gap %.3g, merges moved %d / not %d, back in %d, timed later than entered %d"
          % (name, ref["gap"], ref["merge_gap"], ref["moved"], ref["unmoved"], ref["back"], ref["later"]))
    assert ref["gap"] >= R.GAP and ref["merge_gap"] >= R.GAP, "the premise does not hold for this seed"
    assert 0 in lens and len(set(lens)) > 1 and max(lens) <= 24 and B == 4 and nbest == W
    if W > 1:
        assert ref["moved"] > 0 and ref["unmoved"] > 0 and ref["later"] > 0
    if lm_seed is not None:
        assert ref["reordered"], "the end-of-sentence factors must reorder the report"
    if dead:
        assert (ref["lengths"][dead[0]] == -1).all() and (ref["frames"][dead[0]] == -1).all() and (ref["logps"][dead[0]] == 0).all()
    held = ref["labels"] >= 0
    assert np.isfinite(ref["logps"]).all() and (ref["logps"][held] < 0).all() and (ref["frames"][held] >= 0).all()
    # what the GPU test asserts of the device, of the reference itself: strictly increasing frames along a hypothesis
    fr = ref["frames"].astype(np.int64)
    both = held[..., 1:] & held[..., :-1]
    assert (np.diff(fr, axis=-1)[both] > 0).all()


def test_the_case_set_distinguishes_the_rule():
    refs = [R.one_shot_case(n)[3] for n in R.ONE_SHOT]
    assert sum(r["moved"] for r in refs) > 0 and sum(r["unmoved"] for r in refs) > 0
    assert sum(r["later"] for r in refs) > 0, "no reported label is timed later than its prefix entered the beam"
    assert sum(r["back"] for r in refs) > 0, "no prefix left the beam and was extended back in"
    assert all((r["frames"] != r["entered"]).any() for r, n in zip(refs, R.ONE_SHOT) if R.ONE_SHOT[n][4] > 1)


def test_block_edge_premises():
    _, seed, scale, B, T, Cc, W, cutoff, nbest, blank = R.EDGE
    p, ref = R.edge_case()
    seam = R.EDGE_SEAM
    assert (W, Cc, T) == (128, 4, 70) and 8192 // W == 64 and seam == T - 64
    print("edge: selection gap %.3g, merge gap %.3g, moved %d / not %d" % (ref["gap"], ref["merge_gap"], ref["moved"], ref["unmoved"]))
    assert ref["gap"] >= R.GAP and ref["merge_gap"] >= R.GAP
    fr, en = ref["frames"][0], ref["entered"][0]
    held = fr >= 0
    # a label timed in the row's first frames while a merge behind the seam moved another position of the same hypothesis
    assert ((held & (fr < seam)).any(-1) & (held & (fr != en) & (fr >= seam)).any(-1)).any()
    # a position whose extension record lies before the seam and whose moving merge lies behind it: the mark crosses the staged blocks
    assert (held & (en < seam) & (fr >= seam)).any()


def test_stream_premises():
    """max_labels = 2 on the "w8_c7" case: a reported hypothesis longer than 2 whose positions 1 and 2 were both moved by a merge, the
    one at position 1 in a later frame than the label entered (frame-by-frame pushes: a later push)"""
    ref = R.one_shot_case(R.STREAM_CASE)[3]
    fr, en, n = ref["frames"], ref["entered"], ref["lengths"]
    assert ((n > 2) & (fr[..., 1] > en[..., 1]) & (fr[..., 2] > en[..., 2])).any()


# ---- 2: the exact tie ----
def test_exact_tie_keeps_the_frame():
    p = R.tie_case()
    ref = R.reference(p, [2], 0, 2, 0, 2)
    assert ref["merge_gap"] == 0.0 and ref["unmoved"] == 1 and ref["moved"] == 0
    assert ref["labels"][0, 0].tolist() == [1, -1] and ref["frames"][0, 0].tolist() == [0, -1]
    assert ref["logps"][0, 0, 0] == np.float32(np.log(0.5))


# ---- 3: the host layer ----
def _declared():
    header = open(os.path.join(ROOT, "include", "nntoolkitcore_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    return set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", header)), header


@pytest.mark.parametrize("name", NEW)
def test_declared_exported_and_bound(built_lib, name):
    assert name in _declared()[0], "not declared in include/nntoolkitcore_hip.h"
    assert hasattr(built_lib, name), "not exported by the library"
    assert name in capi.SIGNATURES, "not bound in capi.py"
    res, args = capi.SIGNATURES[name]
    fn = getattr(built_lib, name)
    assert fn.restype is res and list(fn.argtypes) == list(args)


def test_the_option_struct_is_the_headers():
    assert re.search(r"typedef struct \{\s*NntkNgramLm lm;\s*int \*label_frames;\s*float \*label_logps;\s*\} NntkCtcBeamOptions;",
                     _declared()[1])
    assert [f[0] for f in capi.NntkCtcBeamOptions._fields_] == ["lm", "label_frames", "label_logps"]
    assert C.sizeof(capi.NntkCtcBeamOptions) == 3 * C.sizeof(C.c_void_p)


def _opts(frames=None, logps=None, lm=None):
    return C.byref(capi.NntkCtcBeamOptions(lm, frames, logps))


def test_workspace_and_state_sizes():
    L = capi.load()
    plain, lm = L.nntk_ctc_beam_workspace_floats(4, 50, 29, 16, 0), L.nntk_ctc_beam_lm_workspace_floats(4, 50, 29, 16, 0)
    assert L.nntk_ctc_beam_opt_workspace_floats(4, 50, 29, 16, 0, None) == plain
    assert L.nntk_ctc_beam_opt_workspace_floats(4, 50, 29, 16, 0, _opts()) == plain
    assert L.nntk_ctc_beam_opt_workspace_floats(4, 50, 29, 16, 0, _opts(64, 128)) == plain
    assert L.nntk_ctc_beam_opt_workspace_floats(4, 50, 29, 16, 0, _opts(lm=4096)) == lm
    sb = L.nntk_ctc_beam_stream_state_bytes_opt
    assert sb(4, 50, 29, 16, 0, 100, 0, 0) == L.nntk_ctc_beam_stream_state_bytes(4, 50, 29, 16, 0, 100)
    assert sb(4, 50, 29, 16, 0, 100, 1, 0) == L.nntk_ctc_beam_stream_state_bytes_lm(4, 50, 29, 16, 0, 100)
    for with_lm in (0, 1):
        # 16 * max_labels bytes more per row and beam entry: two halves of the frames and of the log-probabilities
        assert sb(4, 50, 29, 16, 0, 100, with_lm, 1) - sb(4, 50, 29, 16, 0, 100, with_lm, 0) == 4 * 16 * 16 * 100
    per_entry = (sb(4, 50, 29, 17, 0, 100, 0, 1) - sb(4, 50, 29, 16, 0, 100, 0, 1) - 4 * 50 * 8) / 4
    assert per_entry == 40 + 2 * 4 * 100 + 16 * 100
    assert sb(4096, 1000, 64, 128, 0, 4096, 1, 1) > 2 ** 35


A = dict(probs=0x100000, labels=0x200000, lengths=0x300000, scores=0x400000, ws=0x500000, frames=0x600000, logps=0x700000)


def _decode(frames, logps, **kw):
    """nntk_ctc_beam_decode_opt_device on addresses that are never dereferenced: B 2, T 8, C 5, W 4, nbest 2"""
    a = dict(A, **kw)
    return capi.load().nntk_ctc_beam_decode_opt_device(a["probs"], 2, 8, 5, None, 4, 4, 0, 2, _opts(frames, logps), a["labels"],
                                                       a["lengths"], a["scores"], a["ws"])


def test_one_shot_refusals_need_no_device():
    nl = 2 * 2 * 8 * 4                                     # bytes of a [2][2][8] output
    assert _decode(A["frames"] + 2, None) == -1 and "d_label_frames is not 4-byte aligned" in capi.last_error()
    assert _decode(None, A["logps"] + 1) == -1 and "d_label_logps is not 4-byte aligned" in capi.last_error()
    assert _decode(A["frames"], A["frames"] + nl - 4) == -1 and "d_label_frames overlaps d_label_logps" in capi.last_error()
    assert _decode(A["labels"] + nl - 4, None) == -1 and "d_label_frames overlaps d_labels_out" in capi.last_error()
    assert _decode(None, A["lengths"]) == -1 and "d_label_logps overlaps d_out_lengths" in capi.last_error()
    assert _decode(A["scores"] - nl + 4, None) == -1 and "d_label_frames overlaps d_scores" in capi.last_error()
    assert _decode(None, A["probs"] + 2 * 8 * 5 * 4 - 4) == -1 and "d_label_logps overlaps d_probs" in capi.last_error()
    ws = 4 * capi.load().nntk_ctc_beam_workspace_floats(2, 8, 5, 4, 0)
    assert _decode(A["ws"] + ws - 4, None) == -1 and "d_label_frames overlaps d_workspace" in capi.last_error()
    # everything the plain call refuses, first
    L = capi.load()
    assert L.nntk_ctc_beam_decode_opt_device(A["probs"], 2, 8, 5, None, 4, 4, 0, 5, _opts(A["frames"], A["logps"]), A["labels"],
                                             A["lengths"], A["scores"], A["ws"]) == -1 and "nbest" in capi.last_error()
    bad = np.asarray([3, 9], np.int32)
    assert L.nntk_ctc_beam_decode_opt_device(A["probs"], 2, 8, 5, bad.ctypes.data_as(capi.ip), 4, 4, 0, 2, _opts(A["frames"], None),
                                             A["labels"], A["lengths"], A["scores"], A["ws"]) == -1 and capi.last_error() != ""
    assert L.nntk_ctc_beam_decode_opt_device(A["probs"], 2, 8, 5, None, 4, 4, 0, 2, _opts(A["frames"], None), A["labels"], None,
                                             A["scores"], A["ws"]) == -1 and "NULL" in capi.last_error()
    # the empty batch: nothing to do, with or without detail
    assert L.nntk_ctc_beam_decode_opt_device(None, 0, 8, 5, None, 4, 4, 0, 2, _opts(A["frames"] + 1, None), None, None, None, None) == 0
    assert L.nntk_ctc_beam_decode_opt(None, 0, 8, 5, None, 4, 4, 0, 2, None, None, None, None) == 0 and capi.last_error() == ""


GOOD = dict(batch=2, max_frames=8, C=5, blank=4, W=4, cut=0, nbest=2, max_labels=16)
BAD = [dict(W=0), dict(W=129, nbest=1), dict(nbest=0), dict(nbest=5), dict(cut=-1), dict(blank=5), dict(max_frames=0), dict(max_labels=0),
       dict(batch=-1), dict(W=128, C=130, nbest=1)]


def _create(a, detail=1):
    return capi.load().nntk_ctc_beam_stream_create_opt(a["batch"], a["max_frames"], a["C"], a["blank"], a["W"], a["cut"], a["nbest"],
                                                       a["max_labels"], None, detail)


@pytest.mark.parametrize("change", BAD, ids=lambda c: ",".join("%s=%s" % kv for kv in c.items()))
def test_create_opt_refuses_what_create_refuses(change):
    assert not _create(dict(GOOD, **change)) and capi.last_error() != ""


def test_stream_refusals_need_no_device():
    """a stream takes the pushes of its kind only; every refusal comes before the handle's device memory is reserved"""
    L = capi.load()
    lab, n, sc = np.full((2, 2, 16), 7, np.int32), np.full((2, 2), 7, np.int32), np.full((2, 2), 7.0, np.float32)
    fr, lg = np.full((2, 2, 16), 7, np.int32), np.full((2, 2, 16), 7.0, np.float32)
    p = np.full((2, 8, 5), 0.2, np.float32)
    nf = np.asarray([1, 1], np.int32)
    host = (p.ctypes.data_as(capi.fp), nf.ctypes.data_as(capi.ip), None, lab.ctypes.data_as(capi.ip), n.ctypes.data_as(capi.ip),
            sc.ctypes.data_as(capi.fp))
    dev = (A["probs"], nf.ctypes.data_as(capi.ip), None, A["labels"], A["lengths"], A["scores"])
    plain, detail = _create(GOOD, 0), _create(GOOD, 1)
    assert plain and detail and capi.last_error() == ""
    # created without detail, pushed with detail pointers
    assert L.nntk_ctc_beam_stream_push_opt(plain, *host, fr.ctypes.data_as(capi.ip), None) == -1 and "without detail" in capi.last_error()
    assert L.nntk_ctc_beam_stream_push_opt(plain, *host, None, lg.ctypes.data_as(capi.fp)) == -1 and "without detail" in capi.last_error()
    assert L.nntk_ctc_beam_stream_push_opt_device(plain, *dev, A["frames"], A["logps"]) == -1 and "without detail" in capi.last_error()
    # created with detail, pushed through the old calls
    assert L.nntk_ctc_beam_stream_push(detail, *host) == -1 and "with detail" in capi.last_error()
    assert L.nntk_ctc_beam_stream_push_device(detail, *dev) == -1 and "with detail" in capi.last_error()
    # a detail output that is misaligned or overlaps
    assert L.nntk_ctc_beam_stream_push_opt_device(detail, *dev, A["frames"] + 2, None) == -1 and "aligned" in capi.last_error()
    assert L.nntk_ctc_beam_stream_push_opt_device(detail, *dev, A["labels"], None) == -1 and "overlaps d_labels_out" in capi.last_error()
    assert L.nntk_ctc_beam_stream_push_opt_device(detail, *dev, A["frames"], A["frames"] + 4) == -1 and "overlaps" in capi.last_error()
    assert L.nntk_ctc_beam_stream_push_opt_device(detail, *dev, None, A["probs"]) == -1 and "overlaps d_probs" in capi.last_error()
    # what every push refuses
    bad = np.asarray([3, 9], np.int32)
    assert L.nntk_ctc_beam_stream_push_opt(detail, host[0], bad.ctypes.data_as(capi.ip), *host[2:], fr.ctypes.data_as(capi.ip),
                                           lg.ctypes.data_as(capi.fp)) == -1 and "n_frames" in capi.last_error()
    assert L.nntk_ctc_beam_stream_push_opt(None, *host, None, None) == -1 and "NULL handle" in capi.last_error()
    for a in (lab, n, fr):
        assert (a == 7).all()
    assert (sc == 7.0).all() and (lg == 7.0).all()
    L.nntk_ctc_beam_stream_destroy(plain)
    L.nntk_ctc_beam_stream_destroy(detail)
    empty = _create(dict(GOOD, batch=0))
    assert empty and L.nntk_ctc_beam_stream_push_opt_device(empty, None, None, None, None, None, None, None, None) == 0
    assert L.nntk_ctc_beam_stream_push_opt(empty, None, None, None, None, None, None, None, None) == 0 and capi.last_error() == ""
    L.nntk_ctc_beam_stream_destroy(empty)
