"""The premises of tests/test_gpu_rnnt_beam_detail.py, on the CPU alone (tests/rnnt_beam_detail_cases.py): on every case the device test
uses, the float64 reference is unambiguous -- its smallest gap at a cut (cut_gap), in the reported order (order_gap), between a merged
candidate and the entry's lead where the two sides' frames differ (lead_gap) and, with length normalisation, between consecutive keys
(key_gap) is at least GAP = 1e-3 -- and its float32 restatement returns the same labels and the same frames.  The tie case is exempt
by construction: its merges with differing frames are exact ties, which keep what the entry has.  With length normalisation the report is the
one without it, ranked again: the same search without it returns plain_labels."""
import numpy as np
import pytest

import rnnt_beam_detail_cases as DC


@pytest.mark.parametrize("name", DC.ALL_CASES)
def test_the_reference_is_unambiguous_on_the_case(name):
    r64 = DC.assert_premise(name)
    c = DC.case(name)
    for b, n in enumerate(c["n"]):                   # the structure the device test asserts holds for the reference itself
        for y, fr, lp in zip(r64["labels"][b], r64["frames"][b], r64["lps"][b]):
            assert len(fr) == len(y) == len(lp)
            assert all(0 <= t < n for t in fr) and all(s <= t for s, t in zip(fr, fr[1:])), (name, b, fr)
            assert all(fr.count(t) <= c["ms"] for t in fr) and sum(lp) <= 0.0, (name, b, fr, lp)


def test_some_merge_switches_the_arrays_and_some_merge_does_not():
    sw = {nm: DC.reference(nm)[0]["lead_switches"].sum() for nm in DC.GAP_CASES}
    mg = {nm: DC.reference(nm)[0]["merges"].sum() for nm in DC.GAP_CASES}
    print("switches", sw, "merges", mg)
    assert any(v > 0 for v in sw.values())
    assert any(mg[nm] > 0 and sw[nm] == 0 for nm in DC.GAP_CASES), "a case that merges without a switch"
    assert all(mg[nm] > sw[nm] for nm in DC.GAP_CASES if sw[nm] > 0)     # ... and merges that keep the arrays next to those that do not


@pytest.mark.parametrize("name", DC.NORM_CASES)
def test_length_normalisation_really_reorders(name):
    r64 = DC.reference(name)[0]
    assert r64["reordered"].any() and any(a != b for a, b in zip(r64["labels"], r64["plain_labels"])), name
    for rep in r64["final"]:                         # the report is the plain report's set, ranked by the key
        keys = [float(s) / (len(y) + 1) for y, s, _, _ in rep]
        assert keys == sorted(keys, reverse=True), (name, keys)


def test_the_drop_case_drops_before_it_ranks():
    r64 = DC.reference("lm_norm_drop")[0]
    carried = r64["carried"][0]
    assert len(r64["final"][0]) < len(carried) and all(np.isfinite(float(s)) for _, s, _, _ in r64["final"][0])


def test_the_tolerances_come_from_the_float32_restatement():
    assert 0 < DC.lps_tol() < 1e-4 and 0 < DC.score_tol() < 1e-3


def test_a_stream_counts_frames_from_its_start():
    """the reference on the second half of a row with t0 set is no test of the carried beam, only of the offset's meaning"""
    r = DC.run("stream", n_frames=[3, 0, 2], t0=[5, 0, 1])
    for b, (n, t0) in enumerate(zip([3, 0, 2], [5, 0, 1])):
        assert all(t0 <= t < t0 + n for fr in r["frames"][b] for t in fr)
