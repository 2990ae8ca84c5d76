"""The cases of the wide transducer-decoder tests (tests/test_gpu_rnnt_decode_wide.py, tests/test_gpu_rnnt_beam_wide.py) and their premises
(tests/test_rnnt_decode_wide_premises.py checks them without a device): the models, the float64 references and float32 restatements,
the constants of csrc/hip/rnnt_dec_common.hpp / nntk_shim.h that decide a path, and the arithmetic side of each threshold.
A helper, no test.

The models come from the recipe of the existing decoder tests (_model).  Seeds and label_bias were searched on the CPU (out_scale stayed the recipe's 3) so that
the reference's smallest decision gap is at least GAP, its float32 restatement returns the same labels and the output holds blanks and
labels; nothing about them comes from a device.  With wide V the label bias sits near -log V, or no row ever takes a blank."""
import functools

import numpy as np

import rnnt_beam_reference as RB
import rnnt_decode_reference as R
from test_gpu_rnnt_decode import _case as _small_greedy_case, _model

GAP = 1e-3
# mirrored from csrc/hip/rnnt_dec_common.hpp and csrc/hip/nntk_shim.h: every case asserts on which side of them it stands
LANES = 1024                                        # RD_THREADS: one pass of a `for (n = tid; n < N; n += RD_THREADS)` loop
WAVE = 64
RED_SUM_BYTES = 8 * (LANES // WAVE)                 # red_sum [1][RD_WAVES] doubles, the first member of RdShared<1> / RbShared<1>
LDS_OPT_IN = 48 * 1024                              # above it the launcher asks for the dynamic LDS
LDS_MAX = 152 * 1024                                # RD_LDS_MAX
GROUP, GROUP_BATCH = 4, 512                         # NNTK_RNNT_DEC_GROUP, NNTK_RNNT_DEC_GROUP_BATCH
BEAM_MAX_W = 32                                     # NNTK_RNNT_BEAM_MAX_W
MAX_WIDTH, MAX_V = 1024, 8192                       # NNTK_RNNT_DEC_MAX_WIDTH, NNTK_RNNT_DEC_MAX_V


def _pad4(x):
    return (x + 3) & ~3


def greedy_float_lds(R_, H, J, V):
    """the float arrays of rnnt_greedy_kernel<R>'s LDS, h | c | g | z | buf, in bytes: a lower bound of what the launcher requests"""
    return 4 * R_ * (2 * _pad4(H) + 2 * _pad4(J) + _pad4(max(4 * H, V)))


def beam_float_lds(R_, H, J, V):
    """the float arrays of rnnt_beam_kernel<R>'s LDS, h | c | z | buf, in bytes: a lower bound of what the launcher requests"""
    return 4 * R_ * (2 * _pad4(H) + _pad4(J) + _pad4(max(4 * H, V)))


# ---- greedy -------------------------------------------------------------------------------------------------------------------------

GREEDY_SEEDS = {"g1": 27, "g2": 3, "g3": 1, "g4": 3, "g5": 2}
GREEDY_LABEL_BIAS = {"g1": -4.5, "g2": -4.5, "g3": -4.5, "g4": -4.5, "g5": -4.5}
GREEDY_CASES = ("g1", "g2", "g3", "g4", "g5", "g6")


def greedy_case(name):
    """dict(m = the model, enc, n: the live rows' frames and counts, act, ms = max_symbols_per_frame, batch, rows: where the live rows
    sit in the batch; every other row of the batch has no frames)"""
    if name == "g6":                                # the small stream model of test_gpu_rnnt_decode.py, its three rows repeated
        c = _small_greedy_case("stream")
        batch = GROUP_BATCH + 6                     # 129 full groups and a ragged one of two
        return dict(m=c["m"], enc=c["enc"], n=c["n"], act=c["act"], ms=c["ms"], batch=batch, rows=None)
    seed, lb = GREEDY_SEEDS[name], GREEDY_LABEL_BIAS[name]
    if name == "g1":                                # 4H = 1040: two passes of the gate loop; V: three passes, the last partial; J % 4 = 2
        m, n, T, act, ms = _model(seed, 2100, 9, 260, 258, True, blank=1050, label_bias=lb), [8, 3, 0], 8, "tanh", 3
        batch, rows = 3, [0, 1, 2]
    elif name == "g2":                              # no projection; H = J = 4 * 75 + 1: rd_matvec's tail of one; 4H > V > 1024
        m, n, T, act, ms = _model(seed, 1100, 5, 301, 301, False, blank=1099, label_bias=lb), [6, 4], 6, "relu", 3
        batch, rows = 2, [0, 1]
    elif name == "g3":                              # the limits
        m, n, T, act, ms = _model(seed, MAX_V, 6, MAX_WIDTH, MAX_WIDTH, True, blank=0, label_bias=lb), [4, 2], 4, "tanh", 3
        batch, rows = 2, [0, 1]
    elif name == "g4":                              # four rows a workgroup, with the LDS opt-in; a ragged last group of three
        m, n, T, act, ms = _model(seed, 2100, 7, 256, 256, True, blank=0, label_bias=lb), [4, 2, 3, 4, 1, 3], 4, "tanh", 3
        batch = GROUP_BATCH + 3
        rows = [0, 1, 2, batch - 3, batch - 2, batch - 1]
    elif name == "g5":                              # above the grouping batch, but four rows do not fit the LDS: one row a workgroup
        m, n, T, act, ms = _model(seed, MAX_V, 6, 512, 512, True, blank=0, label_bias=lb), [3, 2, 3, 3], 3, "tanh", 3
        batch = GROUP_BATCH + 1
        rows = [0, 1, 2, batch - 1]
    else:
        raise KeyError(name)
    enc = m["rng"].uniform(-1.5, 1.5, (len(n), T, m["J"])).astype(np.float32)
    return dict(m=m, enc=enc, n=n, act=act, ms=ms, batch=batch, rows=rows)


@functools.lru_cache(maxsize=None)
def greedy_reference(name):
    """(float64 reference, float32 restatement) of the live rows; computed once, shared by every test, never changed"""
    c = greedy_case(name)
    m = c["m"]
    kw = dict(n_frames=c["n"], blank=m["blank"], activation=c["act"], max_symbols_per_frame=c["ms"])
    return (R.greedy_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], **kw),
            R.greedy_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], dtype=np.float32, **kw))


def greedy_f32_error(name):
    r64, r32 = greedy_reference(name)
    return float(np.abs(r32["scores"].astype(np.float64) - r64["scores"]).max())


@functools.lru_cache(maxsize=None)
def greedy_score_tol():
    """4 x the largest |float32 restatement - float64| score over the greedy cases (4: the device's summation order differs)"""
    err = max(greedy_f32_error(nm) for nm in GREEDY_CASES)
    print("greedy, wide: largest float32-restatement score error %.3e -> tolerance %.3e" % (err, 4 * err))
    assert err > 0
    return 4 * err


def greedy_premise(name):
    """the reference is unambiguous on this case, float32 arithmetic decodes it identically, and it holds blanks and labels"""
    r64, r32 = greedy_reference(name)
    c = greedy_case(name)
    live = [b for b, n in enumerate(c["n"]) if n > 0]
    gap = min(r64["gaps"][b] for b in live)
    print("%s: smallest decision gap %.3e; labels %s" % (name, gap, r64["labels"]))
    assert gap >= GAP, (name, r64["gaps"])
    assert r32["labels"] == r64["labels"] and r32["frames"] == r64["frames"], name
    decisions = sum(len(x) for x in r64["cells"])
    n_labels = sum(len(x) for x in r64["labels"])
    assert 0 < n_labels < decisions, (name, "needs blanks and labels")
    assert any(len(r64["labels"][b]) > 0 for b in live), (name, "a live row emits")
    return r64


def greedy_thresholds(name):
    """the arithmetic side of the branches the case is there for; -> the (batch, H, J, V) to ask the shim about"""
    c = greedy_case(name)
    m = c["m"]
    H, J, V, batch = m["H"], m["J"], m["V"], c["batch"]
    assert H <= MAX_WIDTH and J <= MAX_WIDTH and V <= MAX_V
    if name == "g1":
        assert LANES < 4 * H < 2 * LANES and 2 * LANES < V < 3 * LANES and V % LANES          # gates: 2 passes; classes: 3, the last partial
        assert V > 4 * H and J % 4 == 2 and m["proj"] is not None and batch <= GROUP_BATCH    # buf's pitch comes from V
    elif name == "g2":
        assert 4 * H > V > LANES and H % 4 == 1 and H == J and m["proj"] is None and batch <= GROUP_BATCH
    elif name == "g3":
        assert H == J == MAX_WIDTH and V == MAX_V and m["proj"] is not None and batch <= GROUP_BATCH
        # rnnt_greedy_kernel<1> with the opt-in.  At the limits the float part is 48 KiB to the byte, so it alone does not exceed the
        # threshold; the request is above it by RdShared<1>, of which red_sum [1][16] doubles alone are 128 bytes: still a lower bound
        assert greedy_float_lds(1, H, J, V) == LDS_OPT_IN and greedy_float_lds(1, H, J, V) + RED_SUM_BYTES > LDS_OPT_IN
        assert 4 * V * 4 * H == 128 << 20                                                     # the folded table
    elif name == "g4":
        assert batch > GROUP_BATCH and batch % GROUP == 3 and V > 2 * LANES
        assert LDS_OPT_IN < greedy_float_lds(GROUP, H, J, V)
    elif name == "g5":
        assert batch > GROUP_BATCH and greedy_float_lds(GROUP, H, J, V) > LDS_MAX             # the float part alone is too much for four
    elif name == "g6":
        assert batch >= GROUP_BATCH + 3 and batch % GROUP == 2
    return batch, H, J, V


def greedy_expected_rows_per_group(name):
    return {"g1": 1, "g2": 1, "g3": 1, "g4": GROUP, "g5": 1, "g6": GROUP}[name]


# ---- beam ---------------------------------------------------------------------------------------------------------------------------

BEAM_SEEDS = {"b1": 3, "b2": 1, "b3": 0, "b4": 125}
BEAM_LABEL_BIAS = {"b1": -4.5, "b2": -5.0, "b3": -5.0, "b4": -1.5}
BEAM_OUT_SCALE = {"b1": 3.0, "b2": 3.0, "b3": 3.0, "b4": 3.0}
BEAM_CASES = ("b1", "b2", "b3", "b4")               # (b5, the stream, runs b1's model)
B4_WIDTH = BEAM_MAX_W


def beam_case(name):
    """dict(m = the model, enc, n, act, ms = max_symbols_per_frame, W, nbest, max_labels)"""
    seed, lb, osc = BEAM_SEEDS[name], BEAM_LABEL_BIAS[name], BEAM_OUT_SCALE[name]
    if name == "b1":                                # 4H = 1040, V in three passes, J in groups of four; the group of four needs the opt-in
        m, n, T, act, ms, W, nbest = _model(seed, 2300, 9, 260, 260, True, blank=0, out_scale=osc, label_bias=lb), [4, 3], 4, "tanh", 2, 8, 3
    elif name == "b2":                              # four hypotheses do not fit the LDS: one by one without anything pinned
        m, n, T, act, ms, W, nbest = _model(seed, MAX_V, 6, 512, 512, True, blank=0, out_scale=osc, label_bias=lb), [3, 2], 3, "tanh", 2, 4, 2
    elif name == "b3":                              # the limits
        m, n, T, act, ms, W, nbest = _model(seed, MAX_V, 6, MAX_WIDTH, MAX_WIDTH, True, blank=0, out_scale=osc, label_bias=lb), [3, 2], 3, \
            "tanh", 2, 2, 2
    elif name == "b4":                              # the widest beam on the wide_identity family of test_gpu_rnnt_beam.py
        m, n, T, act, ms, W, nbest = _model(seed, 70, 5, 33, 33, False, blank=69, out_scale=osc, label_bias=lb), [4, 3], 4, "identity", 3, \
            B4_WIDTH, 4
    else:
        raise KeyError(name)
    enc = m["rng"].uniform(-1.5, 1.5, (len(n), T, m["J"])).astype(np.float32)
    return dict(m=m, enc=enc, n=n, act=act, ms=ms, W=W, nbest=nbest, max_labels=ms * T)


def beam_run(c, n=None, dtype=np.float64):
    m = c["m"]
    return RB.beam_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], n_frames=c["n"] if n is None else n, blank=m["blank"],
                          activation=c["act"], max_symbols_per_frame=c["ms"], beam_width=c["W"], nbest=c["nbest"],
                          max_labels=c["max_labels"], dtype=dtype)


@functools.lru_cache(maxsize=None)
def beam_reference(name):
    """(float64 reference, float32 restatement); computed once, shared by every test, never changed"""
    c = beam_case(name)
    return beam_run(c), beam_run(c, dtype=np.float32)


def beam_f32_error(name):
    r64, r32 = beam_reference(name)
    return max([abs(float(x) - float(y)) for a, b in zip(r32["scores"], r64["scores"]) for x, y in zip(a, b)] + [0.0])


@functools.lru_cache(maxsize=None)
def beam_score_tol():
    """4 x the largest |float32 restatement - float64| score over the beam cases (4: the device's summation order differs)"""
    err = max(beam_f32_error(nm) for nm in BEAM_CASES)
    print("beam, wide: largest float32-restatement score error %.3e -> tolerance %.3e" % (err, 4 * err))
    assert err > 0
    return 4 * err


def beam_premise(name):
    """the reference is unambiguous at every cut and in the final order, float32 arithmetic returns the same labels, and a live row's
    n-best holds labels"""
    r64, r32 = beam_reference(name)
    c = beam_case(name)
    live = [b for b, n in enumerate(c["n"]) if n > 0]
    cut, order = min(r64["cut_gap"][b] for b in live), min(r64["order_gap"][b] for b in live)
    print("%s: cut gap %.3e, order gap %.3e, largest |B| %s; labels %s" % (name, cut, order, r64["max_b"], r64["labels"]))
    assert cut >= GAP and order >= GAP, (name, cut, order)
    assert r32["labels"] == r64["labels"], name
    assert any(len(y) > 0 for b in live for y in r64["labels"][b]), (name, "needs a label")
    assert r64["cuts"].sum() > 0, (name, "needs a cut")
    return r64


@functools.lru_cache(maxsize=None)
def beam_stream_reference():
    """b5: b1 after its first push (two frames a row), for the size of the carried set"""
    c = beam_case("b1")
    return beam_run(c, n=B5_FIRST)


B5_FIRST = [2, 1]                                   # the frames of b5's first push; the second brings the rest


def beam_thresholds(name):
    """the arithmetic side of the branches the case is there for; -> the (W, H, J, V) to ask the shims about"""
    c = beam_case(name)
    m = c["m"]
    H, J, V, W = m["H"], m["J"], m["V"], c["W"]
    assert H <= MAX_WIDTH and J <= MAX_WIDTH and V <= MAX_V and 1 <= c["nbest"] <= W <= BEAM_MAX_W
    if name == "b1":
        assert LANES < 4 * H < 2 * LANES and 2 * LANES < V < 3 * LANES and J > 4 and m["proj"] is not None
        assert LDS_OPT_IN < beam_float_lds(GROUP, H, J, V) and W > 1
    elif name == "b2":
        assert W > 1 and beam_float_lds(GROUP, H, J, V) >= LDS_MAX                # (the fixed part adds to it)
    elif name == "b3":
        assert H == J == MAX_WIDTH and V == MAX_V and W > 1
    elif name == "b4":
        assert W == B4_WIDTH and W % GROUP == 0 and W // GROUP == 8 and (c["ms"] + 1) * W > WAVE
    return W, H, J, V


def beam_expected_group(name):
    return {"b1": GROUP, "b2": 1, "b3": 1, "b4": GROUP}[name]
