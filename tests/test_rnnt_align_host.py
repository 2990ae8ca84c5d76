"""CPU only: the references of the transducer forced-alignment tests (tests/rnnt_align_reference.py) against enumeration and against
the loss reference; the premises of the device cases (tests/test_gpu_rnnt_align.py), so that a case that no longer tests what it is
there for turns red without a device; and the host-side refusals of nntk_rnnt_align* / nntk_rnnt_fused_align*, which need no device."""
import math

import numpy as np
import pytest
import torch

import rnnt_align_reference as A
import rnnt_cases as K
import rnnt_reference as R
from nntoolkitcore_amd import capi

@pytest.mark.parametrize("T,U,V,seed", [(1, 0, 3, 0), (1, 3, 3, 1), (3, 0, 4, 2), (2, 2, 3, 3), (4, 3, 5, 4), (3, 3, 2, 5), (4, 2, 4, 6)])
def test_float64_reference_equals_enumeration(T, U, V, seed):
    rng = np.random.default_rng(seed)
    blank = int(rng.integers(0, V))
    lab = K.labels(rng, U, V, blank)
    lp = R.log_softmax(rng.uniform(-3, 3, (T, U + 1, V)))
    r = A.viterbi_row(lp, lab, blank)
    best, frames, n_paths = A.brute_force_row(lp, lab, blank)
    assert n_paths == math.comb(T - 1 + U, U)
    assert r["score"] == best and r["label_frames"].tolist() == frames
    assert abs(r["label_logp"].sum() + r["frame_logp"].sum() - r["score"]) <= 1e-12 * abs(best)
    for t in range(T):
        assert r["frame_labels"][t] == sum(f <= t for f in frames)


@pytest.mark.parametrize("T,U", [(4, 3), (3, 2), (1, 3), (4, 0)])
def test_tie_break_on_flat_scores(T, U):
    """every path ties exactly; the blank move wins every decision, so the walk back from (T - 1, U) takes blanks down to frame 0 and
    every label is emitted in frame 0"""
    lp = R.log_softmax(np.zeros((T, U + 1, 4)))
    lab = [1, 2, 2][:U]
    r = A.viterbi_row(lp, lab, 0)
    best, frames, _ = A.brute_force_row(lp, lab, 0)
    assert r["score"] == best and r["label_frames"].tolist() == frames == [0] * U
    assert r["frame_labels"].tolist() == [U] * T
    assert r["gap"] == (0.0 if T > 1 and U > 0 else math.inf)


@pytest.mark.parametrize("name", ["ragged", "random", "peaked", "forced"])
def test_score_is_at_most_minus_the_loss(name):
    c = A.case(name)
    rows = A.reference(name)[0]
    for b, r in enumerate(rows):
        if r["score"] == -math.inf:
            continue
        n, lab = c["lens"][b], c["labels"][b]
        loss, _ = R._row(R.log_softmax(c["x"][b, :n, :len(lab) + 1]), list(lab), c["blank"])
        assert r["score"] <= -loss + 1e-12 * abs(loss), (name, b)


def test_float32_restatement_follows_the_float64_reference():
    for name in ("ragged", "random"):
        rows, s32 = A.reference(name)
        for b, r in enumerate(rows):
            assert abs(s32[b] - r["score"]) <= 1e-5 * abs(r["score"]), (name, b)


# ---- the premises of the device cases ----

GAP_CASES = ["ragged", "ragged_V64", "ragged_V5", "ragged_V257", "random", "long", "two_blocks", "peaked", "range"] + \
            ["inst_%d_%d" % k for k in A.INSTANTIATIONS]


@pytest.mark.parametrize("name", GAP_CASES)
def test_no_row_is_left_out_of_the_exact_comparison(name):
    c = A.case(name)
    rows = A.reference(name)[0]
    gaps = [r["gap"] for r in rows]
    thr = max(A.gap_threshold(n, len(lab)) for n, lab in zip(c["lens"], c["labels"]))
    print("%s: smallest gap %.3e, largest threshold %.3e" % (name, min(gaps), thr))
    assert A.left_out(name) == [], (name, gaps)
    assert all(np.isfinite(r["score"]) for r in rows)


def test_ragged_premise():
    c = A.case("ragged")
    assert c["x"].shape == (8, 7, 5, 5) and c["blank"] == 2
    u = [len(r) for r in c["labels"]]
    assert 0 in u and 4 in u and 1 in c["lens"] and any(r[k] == r[k + 1] for r in c["labels"] for k in range(len(r) - 1))
    assert all(k != 2 for r in c["labels"] for k in r)
    for v in (64, 5, 257):
        assert A.case("ragged_V%d" % v)["x"].shape[3] == v
    rows = A.reference("ragged")[0]
    assert any(len(set(r["label_frames"].tolist())) > 1 for r in rows)          # labels in different frames


def test_random_and_long_premise():
    c = A.case("random")
    assert c["x"].shape == (32, 40, 13, 29) and min(c["lens"]) >= 20 and max(c["lens"]) <= 40 and len(set(c["lens"])) > 4
    assert A.case("long")["x"].shape == (8, 120, 61, 29)


@pytest.mark.parametrize("T,maxL", list(A.INSTANTIATIONS))
def test_instantiation_premise(T, maxL):
    c = A.case("inst_%d_%d" % (T, maxL))
    assert c["x"].shape == (3, T, maxL + 1, 3) and c["lens"] == [T, T, T - 1] and [len(r) for r in c["labels"]] == [maxL, maxL, maxL // 2]
    nj, lds = K.lattice_path(maxL)
    assert (nj, lds > K.LDS_OPT_IN) == A.INSTANTIATIONS[(T, maxL)]


def test_two_blocks_premise():
    c = A.case("two_blocks")
    B, T, U1, _ = c["x"].shape
    assert min(65536 // min(T, U1), A.BT_DIAGS) == A.BT_DIAGS                     # rnnt_bt_block_diags: the cap decides here
    assert c["lens"][0] + len(c["labels"][0]) > A.BT_DIAGS                        # the path's moves do not fit one block


def test_peaked_and_range_and_forced_premises():
    c = A.case("peaked")
    for b, r in enumerate(A.reference("peaked")[0]):
        assert r["label_frames"].tolist() == c["paths"][b]
        n, lab = c["lens"][b], c["labels"][b]
        loss, _ = R._row(R.log_softmax(c["x"][b, :n, :len(lab) + 1]), list(lab), c["blank"])
        assert abs(r["score"] + loss) <= 1e-9
    assert len(set(c["paths"][0])) > 2
    c = A.case("range")
    r = A.reference("range")[0][0]
    assert r["label_frames"].tolist() == c["paths"][0]
    assert -2780.0 < r["score"] < -2750.0                                        # ln 1e-1200 = -2763: far below float32 and float64
    assert math.exp(r["score"]) == 0.0
    rows = A.reference("forced")[0]
    assert rows[0]["label_frames"].tolist() == [0, 0, 0] and np.isfinite(rows[0]["score"])
    free = A.viterbi(np.where(np.isinf(A.case("forced")["x"]), 0.0, A.case("forced")["x"]), A.case("forced")["labels"], [5, 5, 5], 0)
    assert free[0]["label_frames"].tolist() != [0, 0, 0]                         # the -inf scores do force the path
    assert rows[1]["score"] == -math.inf and (rows[1]["label_frames"] == -1).all() and (rows[1]["frame_labels"] == -1).all()
    assert np.isfinite(rows[2]["score"])


@pytest.mark.parametrize("kind", A.FUSED_KINDS)
@pytest.mark.parametrize("name", ["ragged_%d_%d_%d" % k for k in A.FUSED_RAGGED] + ["cells_%d_%d" % k for k in A.FUSED_CELLS] + ["wide"])
def test_fused_premise(name, kind):
    if not name.startswith("ragged") and kind != "tanh":
        return
    c = A.fused_case(name)
    _, rows, s32 = A.fused_reference(name, kind)
    gaps = [r["gap"] for r in rows]
    print("%s %s: smallest gap %.3e" % (name, kind, min(gaps)))
    assert min(gaps) > A.FUSED_GAP, (name, kind, gaps)
    if name.startswith("cells"):
        assert c["enc"].shape[1] * c["pred"].shape[1] in (20, 32, 33)
    if name == "wide":
        assert c["pred"].shape[1] == 301


def test_greedy_path_is_the_viterbi_path():
    import rnnt_decode_reference as D
    m = A.greedy_model()
    g = D.greedy_decode(m["embed"], m["lstm"], m["proj"], m["out"], m["enc"], n_frames=m["n"], blank=m["blank"], activation="tanh",
                        max_symbols_per_frame=100)
    g32 = D.greedy_decode(m["embed"], m["lstm"], m["proj"], m["out"], m["enc"], n_frames=m["n"], blank=m["blank"], activation="tanh",
                          max_symbols_per_frame=100, dtype=np.float32)
    assert g["capped"].sum() == 0 and g32["labels"] == g["labels"] and g32["frames"] == g["frames"]
    maxL = max(len(r) for r in g["labels"])
    assert maxL >= 3 and any(len(set(f)) > 1 for f in g["frames"])
    x = A.teacher_forced_logits(m, g["labels"], maxL).astype(np.float32)
    rows = A.viterbi(x, g["labels"], m["n"], m["blank"])
    for b, r in enumerate(rows):
        assert r["label_frames"].tolist() == g["frames"][b], b
        assert r["gap"] > A.gap_threshold(m["n"][b], len(g["labels"][b])), (b, r["gap"])
        assert abs(r["score"] - g["scores"][b]) <= 1e-4 * max(1.0, abs(r["score"]))     # the greedy path's own score


# ---- refusals: no device needed ----

GOOD, _ints, _p = K.GOOD, K.ints, K.ptr
BAD = K.BAD + K.WS_BAD + K.ALIGN_ONLY
PLAIN_ONLY, FUSED_ONLY = K.PLAIN_ONLY, K.FUSED_ONLY + K.FUSED_ALIGN_ONLY


@pytest.mark.parametrize("name,change,word", BAD + PLAIN_ONLY, ids=K.ids(BAD + PLAIN_ONLY))
def test_device_form_rejects_before_touching_a_device(name, change, word):
    """dummy device pointers: a call that got past the checks would fault, a refusal never looks at them"""
    a = dict(GOOD, **change)
    rc = capi.load().nntk_rnnt_align_device(_p(a["x"]), a["B"], a["T"], a["V"], _ints(a["il"]), _ints(a["lab"]), _ints(a["ll"]), a["ML"],
                                            a["blank"], _p(a["lf"]), _p(a["fl"]), _p(a["lp"]), _p(a["fp"]), _p(a["sc"]), _p(a["ws"]))
    assert rc == -1 and word in capi.last_error(), (name, capi.last_error())


@pytest.mark.parametrize("name,change,word", BAD + FUSED_ONLY, ids=K.ids(BAD + FUSED_ONLY))
def test_fused_device_form_rejects_before_touching_a_device(name, change, word):
    a = dict(GOOD, **change)
    rc = capi.load().nntk_rnnt_fused_align_device(_p(a["enc"]), _p(a["pred"]), _p(a["out"]), a["B"], a["T"], a["J"], a["V"], a["act"],
                                                  _ints(a["il"]), _ints(a["lab"]), _ints(a["ll"]), a["ML"], a["blank"], _p(a["lf"]),
                                                  _p(a["fl"]), _p(a["lp"]), _p(a["fp"]), _p(a["sc"]), _p(a["ws"]))
    assert rc == -1 and word in capi.last_error(), (name, capi.last_error())


HOST_BAD = [b for b in BAD if b[0].split()[0] not in ("misaligned", "NULL", "label_frames", "scores", "frame_logp", "frame_labels")
            or b[0] in ("NULL labels", "NULL label lengths", "NULL scores")]


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name,change,word", HOST_BAD, ids=K.ids(HOST_BAD))
def test_host_forms_reject_and_write_nothing(name, change, word, fused):
    L = capi.load()
    a = dict(GOOD, **change)
    n = 1 << 12                                           # never read: the refusal comes first
    x = np.zeros(n, np.float32)
    outs = {k: np.full(n, 7.0, np.float32) for k in ("lf", "fl", "lp", "fp", "sc")}
    q = lambda k, t: None if a[k] is None else outs[k].ctypes.data_as(t)
    xp = x.ctypes.data_as(capi.fp)
    tail = (_ints(a["il"]), _ints(a["lab"]), _ints(a["ll"]), a["ML"], a["blank"], q("lf", capi.ip), q("fl", capi.ip), q("lp", capi.fp),
            q("fp", capi.fp), q("sc", capi.fp))
    if fused:
        rc = L.nntk_rnnt_fused_align(xp, xp, xp, a["B"], a["T"], a["J"], a["V"], a["act"], *tail)
    else:
        rc = L.nntk_rnnt_align(xp, a["B"], a["T"], a["V"], *tail)
    assert rc == -1 and word in capi.last_error(), (name, capi.last_error())
    assert all((o == 7.0).all() for o in outs.values())


def test_the_empty_batch_is_not_an_error():
    L = capi.load()
    assert L.nntk_rnnt_align_device(None, 0, 6, 5, None, None, None, 3, 4, None, None, None, None, None, None) == 0
    assert L.nntk_rnnt_align(None, 0, 6, 5, None, None, None, 3, 4, None, None, None, None, None) == 0
    assert L.nntk_rnnt_fused_align_device(None, None, None, 0, 6, 8, 5, 1, None, None, None, 3, 4, None, None, None, None, None, None) == 0
    assert L.nntk_rnnt_fused_align(None, None, None, 0, 6, 8, 5, 1, None, None, None, 3, 4, None, None, None, None, None) == 0
    assert capi.last_error() == ""


def test_workspace_is_the_loss_only_workspace_plus_the_backpointers():
    L = capi.load()
    up = lambda v: (v + 3) & ~3
    for B, T, ML, J, V in [(2, 6, 3, 8, 5), (3, 40, 12, 64, 29), (1, 2, 1600, 5, 3), (8, 120, 60, 67, 257)]:
        bp = up((B * (T + ML) * min(T, ML + 1) + 3) // 4) + 4
        assert L.nntk_rnnt_align_workspace_floats(B, T, ML) == up(L.nntk_rnnt_workspace_floats(B, T, ML, 0)) + bp
        assert L.nntk_rnnt_fused_align_workspace_floats(B, T, ML, J, V) == up(L.nntk_rnnt_fused_workspace_floats(B, T, ML, J, V, 0)) + bp
