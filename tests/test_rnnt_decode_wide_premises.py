"""The premises of the wide transducer-decoder tests (tests/test_gpu_rnnt_decode_wide.py, tests/test_gpu_rnnt_beam_wide.py), checked without a
device: on every case of tests/rnnt_wide_cases.py the float64 reference is unambiguous (decision gaps of at least GAP), its float32
restatement returns the same labels, the output is not degenerate, the case stands on the intended side of each threshold of the kernels
(the arithmetic ones, and the answers of the shims that need no device), and the references hold what the tests rely on: winners in the
second and third pass of a lane, more than 64 entries in B, a carried set beyond one pass of the copy loops.  A wrong seed or a moved
constant turns red here.  No GPU."""
import pytest

import rnnt_wide_cases as K
from nntoolkitcore_amd import capi


@pytest.mark.parametrize("name", K.GREEDY_CASES)
def test_greedy_case_premises_and_thresholds(name):
    r64 = K.greedy_premise(name)
    batch, H, J, V = K.greedy_thresholds(name)
    rpg = capi.load().nntk_shim_rnnt_dec_rows_per_group
    assert rpg(batch, H, J, V) == K.greedy_expected_rows_per_group(name)
    assert rpg(K.GROUP_BATCH, H, J, V) == 1                                          # at or below the grouping batch: one row a workgroup
    labels = [v for row in r64["labels"] for v in row]
    if name == "g1":                                # winners in each pass of a lane's scan
        assert min(labels) < K.LANES and any(K.LANES <= v < 2 * K.LANES for v in labels) and max(labels) >= 2 * K.LANES, labels
        assert r64["labels"][2] == []
    if name in ("g2", "g3", "g4", "g5"):
        assert max(labels) >= K.LANES, labels
    if name in ("g4", "g5"):                        # the first and the last workgroup both decide something
        c = K.greedy_case(name)
        assert r64["labels"][0] and r64["labels"][-1] and c["rows"][0] == 0 and c["rows"][-1] == c["batch"] - 1
        assert len(c["rows"]) <= K.GROUP_BATCH                                       # the same rows fit a batch that is never grouped


def test_greedy_tolerance_comes_from_the_float32_restatement():
    tol = K.greedy_score_tol()
    assert 0 < tol < 1e-3, tol                      # far below any score difference a wrong label or a dropped term would make


@pytest.mark.parametrize("name", K.BEAM_CASES)
def test_beam_case_premises_and_thresholds(name):
    L = capi.load()
    r64 = K.beam_premise(name)
    W, H, J, V = K.beam_thresholds(name)
    L.nntk_shim_rnnt_beam_set_group(0)
    assert L.nntk_shim_rnnt_beam_fits(H, J, V) == 1
    assert L.nntk_shim_rnnt_beam_group(W, H, J, V) == K.beam_expected_group(name)    # nothing pinned
    if name == "b4":
        assert r64["max_b"].max() > K.WAVE, r64["max_b"]                             # the merge scan goes beyond one pass of a wavefront
        assert r64["merges"].sum() > 0 and all(len(f) == W for f in r64["final"])    # ... and finds something; W survivors a row
        assert W == K.BEAM_MAX_W                                                      # a 32-way cut met GAP: no narrower beam was needed
    else:
        labels = [v for row in r64["labels"] for y in row for v in y]
        assert max(labels) >= K.LANES, labels


def test_beam_stream_carries_more_than_one_pass_of_the_copy_loops():
    c = K.beam_case("b1")
    r = K.beam_stream_reference()
    SF = 2 * c["m"]["H"] + c["m"]["J"]
    for b, first in enumerate(K.B5_FIRST):
        assert 0 < first < c["n"][b]
        assert len(r["final"][b]) * SF > K.LANES, (b, len(r["final"][b]), SF)        # nA * (2H + J): the state save / restore loops


def test_beam_tolerance_comes_from_the_float32_restatement():
    tol = K.beam_score_tol()
    assert 0 < tol < 1e-3, tol
