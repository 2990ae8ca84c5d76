"""What the tests of the CTC prefix beam search's label timestamps share (test_ctc_beam_detail_host.py, test_gpu_ctc_beam_detail.py):
the cases, with the constants of their premises.  The float64 restatement of INTEGRATION.md "Label timestamps and confidences" is
ctc_reference.py's, the one reference of the search: ``reference`` here is its ``reference_detail`` (a dict; ``cap`` cuts the strings
as a stream's max_labels does).  The cases must tell a label's reported frame from ``entered``, the frame its prefix first entered
the beam."""
import functools

import numpy as np

from ctc_reference import reference_detail as reference, softmax
from ngram_cases import Walk, dense_bigram

GAP = 1e-3                                            # selection and merge premise of every case: float32 decides as float64 does

# ---- the cases: name -> (posterior seed, B, T, C, W, cutoff, nbest, blank, lengths, LM table seed or None, (row, frame) of a frame of
# zeros or None).  The seeds were searched on the reference alone, per shape, for the premises test_ctc_beam_detail_host.py asserts;
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
    """the LM of a case: a dense bigram with final_logp, and its float64 walk"""
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
