"""The cases of the long CTC beam-search tests (tests/test_gpu_ctc_beam_long.py) and their premises (tests/test_ctc_long_premises.py checks
them without a device): the inputs, the float64 references, the constants of csrc/hip/ctc_beam.hip / nntk_shim.h that decide how many
blocks of frames the backtrack and the commit stage, and the block arithmetic itself.  A helper, no test.

ctc_beam_backtrack_kernel<FIN> and ctc_beam_commit_kernel<FIN> stage BEAM_BT_RECORDS records per block: TC = max(1, 8192 / W) frames, walked
from the row's last frame back, so the FIRST frames of a row form the short block (``blocks``).  Every case of test_gpu_ctc_beam.py,
test_gpu_ctc_beam_lm.py and test_gpu_ctc_stream.py has T * W <= 8192: one block.  The cases here have two.

The seeds of PARITY were searched on the CPU, per shape and scale, for the premise of test_gpu_ctc_beam.py, and every one holds under
ctc_reference.reference (smallest gaps 2.2e-4, 4.0e-4, 1.3e-3, 2.5e-3); nothing about them comes from a device.  Random posteriors at
scale 2.0 do not meet the premise at these lengths, peaked ones (scale 6.0 and 8.0) do.  None of the four needs the reference's
rescaling (smallest kept total 2^-240); tests/test_ctc_long_premises.py runs that on a flatter row."""
import functools

import numpy as np

from ctc_reference import reference, ref_row_scaled, softmax
from ngram_cases import sparse_trigram

# mirrored from csrc/hip/ctc_beam.hip and csrc/hip/nntk_shim.h; test_ctc_long_premises.py reads them from the source text
BT_RECORDS = 8192                                   # BEAM_BT_RECORDS
CUT_GRID_CAP, CUT_FRAMES_PER_WG = 16384, 4          # beam_launch's cap on ctc_beam_cut_kernel's grid; a wavefront per frame, 4 a workgroup
MAX_W, MAX_CELLS = 128, 16384                       # NNTK_CTC_BEAM_MAX_W, NNTK_CTC_BEAM_MAX_CELLS


def blocks(T, W):
    """the frames of each staged block of a row (or push) of T frames, in frame order: the kernels walk them from the last one"""
    TC = max(1, BT_RECORDS // W)
    out, t1 = [], T
    while t1 > 0:
        out.append(t1 - max(0, t1 - TC))
        t1 -= TC
    return out[::-1]


def premise(T):
    """test_gpu_ctc_beam.py's: the smallest relative gap a parity case may have"""
    return 16 * T * 2.0 ** -24


# ---- 1: parity with the float64 reference across a block seam.  B = 1, blank = C - 1, no class cut ----
# name: (seed, scale, T, C, W, nbest, the blocks the table of the test's module text claims)
PARITY = {
    "w128_T96": (8, 6.0, 96, 40, 128, 8, [32, 64]),
    "w100_T90": (2, 6.0, 90, 40, 100, 8, [9, 81]),          # W not a power of two: TC = 81, 8100 records a block
    "w16_T560": (10, 6.0, 560, 9, 16, 4, [48, 512]),
    "w8_T1100": (0, 8.0, 1100, 9, 8, 4, [76, 1024]),        # the best string has more labels than the 8 low bits of a record hold
}


def parity_probs(name):
    seed, scale, T, Cc, W, nbest, _ = PARITY[name]
    return softmax(seed, 1, T, Cc, scale)


@functools.lru_cache(maxsize=None)
def parity_reference(name):
    """(labels, lengths, float64 scores, the smallest gap of the premise); computed once, shared by every test, never changed"""
    seed, scale, T, Cc, W, nbest, _ = PARITY[name]
    return reference(parity_probs(name), [T], Cc - 1, W, 0, nbest)[:4]


@functools.lru_cache(maxsize=None)
def parity_range(name):
    """(k, floor) of ctc_reference.ref_row_scaled: the power of two the reference carried, the smallest total it kept"""
    seed, scale, T, Cc, W, nbest, _ = PARITY[name]
    _, _, k, floor = ref_row_scaled(parity_probs(name)[0].astype(np.float64), Cc - 1, W, 0)
    return k, floor


def parity_premise(name):
    """the reference is unambiguous on this case (the premise of test_gpu_ctc_beam.py, unchanged) -> its reference"""
    T = PARITY[name][2]
    ref = parity_reference(name)
    print("%s: smallest relative gap %.3g, premise %.3g; best string %d labels" % (name, ref[3], premise(T), ref[1][0, 0]))
    assert ref[3] >= premise(T), "the premise does not hold for this seed"
    return ref


# ---- 2: utterance length.  No float64 parity: a 1000-frame row cannot be kept clear of near-ties ----
# rows of two blocks (488 + 512), two blocks (1 + 512) and exactly one block; 64 frames a push: every commit stages one block
UTT = dict(seed=3, scale=8.0, B=3, T=1000, C=30, W=16, nbest=4, blank=29, lens=[1000, 513, 512], mf=64)
# the recipe of test_gpu_ctc_beam_lm.py's "sparse_trigram" table (seed 2, n_bi = 8, n_tri = 20, arcs0 = 12) at the case's class count,
# with end-of-sentence factors, so that the FIN backtrack reads forder / fmass and the FIN commit reports by slot; D = 2
LM = dict(seed=2, n_bi=8, n_tri=20, arcs0=12, final=True, alpha=0.75, beta=0.25, D=2)


def lm_table(Cc, blank):
    return sparse_trigram(LM["seed"], Cc, blank, n_bi=LM["n_bi"], n_tri=LM["n_tri"], arcs0=LM["arcs0"], final=LM["final"])


@functools.lru_cache(maxsize=None)
def utt_probs():
    """frames past a row's length are NaN"""
    c = UTT
    p = softmax(c["seed"], c["B"], c["T"], c["C"], c["scale"])
    for b, n in enumerate(c["lens"]):
        p[b, n:] = np.nan
    return p


def largest(lens, mf):
    """pushes of mf frames a row until it is through (test_gpu_ctc_stream.py's schedule of that name)"""
    return [[min(mf, max(0, l - i * mf)) for l in lens] for i in range((max(lens) + mf - 1) // mf)]


# ---- 3: one push longer than a block: w128_T96 in one push of 96 frames (the commit stages 32 + 64), and 32 frames a push ----
PUSH = dict(name="w128_T96", long_mf=96, short_mf=32)

# ---- 4: the class cut beyond its grid: 67200 frames, more than 16384 workgroups x 4; 12 parts of 100 rows (5600 frames) have no stride ----
CUT = dict(seed=7, B=1200, T=56, C=12, cutoff=4, W=2, nbest=2, blank=11, part=100)


@functools.lru_cache(maxsize=None)
def cut_case():
    """(probs, lens): ragged, some rows of 0 frames and of 1, the rows of the stride loop's second round among the long ones; NaN padding"""
    c = CUT
    rng = np.random.default_rng(c["seed"] + 1000)
    lens = rng.integers(0, c["T"] + 1, c["B"])
    lens[[3, 500, 1180]] = 0
    lens[[4, 501, 1181]] = 1
    lens[[0, 1175, 1190, c["B"] - 1]] = c["T"]
    p = softmax(c["seed"], c["B"], c["T"], c["C"])
    for b, n in enumerate(lens):
        p[b, n:] = np.nan
    return p, [int(n) for n in lens]
