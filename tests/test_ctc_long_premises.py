"""The premises of the long CTC beam-search tests (tests/test_gpu_ctc_beam_long.py), checked without a device: the constants of
csrc/hip/ctc_beam.hip and csrc/hip/nntk_shim.h that tests/ctc_long_cases.py mirrors are the ones in the source text; every case stands
where its table says (the staged blocks per row and per push, the cell limit, the cut kernel's grid); the float64 reference of the four
parity cases is unambiguous (the gap premise of test_gpu_ctc_beam.py, unchanged) and stays in range (ctc_reference's 2^-900 guard); and
no earlier GPU case of test_gpu_ctc_beam.py, test_gpu_ctc_beam_lm.py or test_gpu_ctc_stream.py stages more than one block, which is why
the new file exists.  A wrong seed or a moved constant turns red here.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

import ctc_long_cases as K
import ctc_reference as R

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nntoolkitcore_amd", "csrc", "hip")


def _text(name):
    with open(os.path.join(HIP, name)) as f:
        return f.read()


def _define(text, name):
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, text, re.M)
    assert m, name
    return int(m.group(1))


def test_the_mirrored_constants_are_the_source_texts():
    hip, shim = _text("ctc_beam.hip"), _text("nntk_shim.h")
    assert _define(hip, "BEAM_BT_RECORDS") == K.BT_RECORDS == 8192
    assert _define(shim, "NNTK_CTC_BEAM_MAX_W") == K.MAX_W == 128
    assert _define(shim, "NNTK_CTC_BEAM_MAX_CELLS") == K.MAX_CELLS == 16384
    # backtrack and commit: the same block of frames, walked from the last one -- one walk, which both kernels call
    assert hip.count("const int TC = max(1, BEAM_BT_RECORDS / W);") == 1
    assert hip.count("for (int t1 = Tb; t1 > 0; t1 -= TC) {") == 1
    assert hip.count("beam_walk_records<DETAIL>(rec, hrow, Tb, W, tid, ") == 2
    # the record: length << 8 | parent rank
    assert hip.count("rank = r.x & 0xff;") == 1 and "len = hrow[(long)(Tb - 1) * W + rank].x >> 8;" in hip and "const int pos = (r.x >> 8) - 1;" in hip
    # the cut kernel: a wavefront per frame, four a workgroup, the grid capped, the rest by stride
    m = re.search(r"long g = \(frames \+ 3\) / 4;\s*if \(g > (\d+)\) g = (\d+);", hip)
    assert m and int(m.group(1)) == int(m.group(2)) == K.CUT_GRID_CAP == 16384
    assert "f < frames; f += gridDim.x * 4L)" in hip and "blockIdx.x * 4L + (threadIdx.x >> 6)" in hip and K.CUT_FRAMES_PER_WG == 4


def test_block_arithmetic():
    assert K.blocks(64, 128) == [64] and K.blocks(65, 128) == [1, 64] and K.blocks(129, 128) == [1, 64, 64]
    assert K.blocks(81, 100) == [81] and K.blocks(8192, 1) == [8192] and K.blocks(8193, 1) == [1, 8192] and K.blocks(0, 16) == []


@pytest.mark.parametrize("name", list(K.PARITY))
def test_parity_case_premises(name):
    seed, scale, T, Cc, W, nbest, want_blocks = K.PARITY[name]
    assert 1 <= nbest <= W <= K.MAX_W and W * ((Cc - 1) + 1) <= K.MAX_CELLS
    assert K.blocks(T, W) == want_blocks and len(want_blocks) == 2 and T * W > K.BT_RECORDS
    if name == "w100_T90":
        assert W & (W - 1) and K.BT_RECORDS % W                                      # a block is not 8192 records
    lab, n, sc, gap = K.parity_premise(name)                                         # the gap premise
    k, floor = K.parity_range(name)                                                  # ... and the range guard ran on every frame
    print("%s: the reference carried 2^-%d, smallest kept total 2^%.1f" % (name, k, math.log2(floor)))
    assert floor >= R.RANGE_FLOOR
    assert (n[0] >= 0).all() and np.isfinite(sc).all() and (np.diff(sc[0]) < 0).all()
    # labels are written in both blocks: every entry of the beam at the seam holds labels, and every reported string is longer than
    # any of them
    seam, _, _, _ = R.ref_row_scaled(K.parity_probs(name)[0, :want_blocks[0]].astype(np.float64), Cc - 1, W, 0)
    at_seam = [len(l) for l, _, _, _ in seam]
    assert min(at_seam) >= 1 and n[0].min() > max(at_seam), (at_seam, n[0])
    if name == "w8_T1100":
        assert n[0, 0] > 255                                                          # beyond the record's low byte


def test_rescaling_by_a_power_of_two_changes_nothing():
    """the reference on a row that leaves 2^-512, against the same row with every frame doubled (exactly): the same strings, the same
    gap to the bit, and totals that differ by exactly the powers of two carried"""
    T, Cc, W, blank = 400, 30, 4, 29
    p = R.softmax(1, 1, T, Cc)[0].astype(np.float64)
    beam1, gap1, k1, floor1 = R.ref_row_scaled(p, blank, W, 0)
    beam2, gap2, k2, floor2 = R.ref_row_scaled(2.0 * p, blank, W, 0)
    assert k1 > 0 and k1 != k2 + T and min(floor1, floor2) >= R.RANGE_FLOOR
    assert gap1 == gap2 and len(beam1) == len(beam2) == W
    for (l1, pb1, pnb1, _), (l2, pb2, pnb2, _) in zip(beam1, beam2):
        assert l1 == l2 and math.ldexp(pb1, k2 + T - k1) == pb2 and math.ldexp(pnb1, k2 + T - k1) == pnb2
    with pytest.raises(AssertionError):
        R.ref_row(p, blank, W, 0)                                                    # the unscaled form refuses such a row


def test_utterance_case_blocks():
    c = K.UTT
    W, mf = c["W"], c["mf"]
    assert 1 <= c["nbest"] <= W <= K.MAX_W and W * c["C"] <= K.MAX_CELLS and c["blank"] == c["C"] - 1
    assert [K.blocks(n, W) for n in c["lens"]] == [[488, 512], [1, 512], [512]]
    assert mf * W <= K.BT_RECORDS and all(len(K.blocks(n, W)) <= 1 for push in K.largest(c["lens"], mf) for n in push)
    assert [sum(push[b] for push in K.largest(c["lens"], mf)) for b in range(c["B"])] == c["lens"]
    p = K.utt_probs()
    for b, n in enumerate(c["lens"]):
        assert np.isfinite(p[b, :n]).all() and np.isnan(p[b, n:]).all()


def test_long_push_blocks():
    seed, scale, T, Cc, W, nbest, want_blocks = K.PARITY[K.PUSH["name"]]
    assert K.PUSH["long_mf"] == T and K.PUSH["long_mf"] * W > K.BT_RECORDS and K.blocks(K.PUSH["long_mf"], W) == want_blocks
    assert K.PUSH["short_mf"] * W <= K.BT_RECORDS and T % K.PUSH["short_mf"] == 0


def test_cut_case_is_beyond_the_grid():
    c = K.CUT
    p, lens = K.cut_case()
    frames = c["B"] * c["T"]
    assert frames == 67200 > K.CUT_GRID_CAP * K.CUT_FRAMES_PER_WG and c["part"] * c["T"] <= K.CUT_GRID_CAP * K.CUT_FRAMES_PER_WG
    assert c["B"] % c["part"] == 0 and c["B"] // c["part"] == 12
    assert 0 < c["cutoff"] < c["C"] - 1 and c["W"] * (c["cutoff"] + 1) <= K.MAX_CELLS and c["T"] * c["W"] <= K.BT_RECORDS
    assert lens.count(0) >= 3 and lens.count(1) >= 3 and len(set(lens)) > 40
    # rows whose frames only the stride loop's second round reaches, with frames
    second = [b for b in range(c["B"]) if b * c["T"] >= K.CUT_GRID_CAP * K.CUT_FRAMES_PER_WG]
    assert len(second) >= 20 and sum(lens[b] > 0 for b in second) >= 15 and lens[c["B"] - 1] == c["T"]
    for b, n in enumerate(lens):
        assert np.isnan(p[b, n:]).all()


def _table_cases():
    """(file, case, T, W) of every table of cases in the three earlier files"""
    import test_gpu_ctc_beam as A
    import test_gpu_ctc_beam_lm as M
    import test_gpu_ctc_stream as S
    out = [("test_gpu_ctc_beam.py", k, v[2], v[4]) for k, v in A.PARITY.items()]
    out += [("test_gpu_ctc_beam_lm.py", k, v[2], v[4]) for k, v in M.PARITY.items()]
    out += [("test_gpu_ctc_beam_lm.py", "CH", M.CH["T"], M.CH["W"]), ("test_gpu_ctc_stream.py", "CH", S.CH["T"], S.CH["W"])]
    out += [("test_gpu_ctc_stream.py", k, v[2], v[4]) for k, v in S.PATHS.items()]
    return out


def _inline_cases():
    """(file, line, T, W) of every `..., T, ..., W, ... = ints` line of the three files"""
    here = os.path.dirname(os.path.abspath(__file__))
    out = []
    for name in ("test_gpu_ctc_beam.py", "test_gpu_ctc_beam_lm.py", "test_gpu_ctc_stream.py"):
        with open(os.path.join(here, name)) as f:
            for line in f:
                m = re.match(r"^\s+([A-Za-z_][\w, ]*?) = ([\d, ]+)$", line.rstrip())
                if not m:
                    continue
                names, values = [x.strip() for x in m.group(1).split(",")], [int(x) for x in m.group(2).split(",")]
                if "T" in names and "W" in names and len(names) == len(values):
                    out.append((name, line.strip(), values[names.index("T")], values[names.index("W")]))
    return out


def test_no_earlier_case_stages_more_than_one_block():
    """why test_gpu_ctc_beam_long.py exists.  (test_stack_into_beam_stream... takes T from its stack: at most 7000 samples at a hop of
    160, W = 8.)"""
    tables, inline = _table_cases(), _inline_cases()
    assert len(tables) >= 27 and len(inline) >= 12, (len(tables), len(inline))
    for f, case, T, W in tables + inline:
        assert T * W <= K.BT_RECORDS and len(K.blocks(T, W)) == 1, (f, case, T, W)
    print("largest T * W of the earlier cases: %d" % max(T * W for _, _, T, W in tables + inline))
    assert max(T for _, _, T, _ in tables + inline) <= 200
