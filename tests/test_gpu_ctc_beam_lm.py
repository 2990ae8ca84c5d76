"""CTC prefix beam search fused with an n-gram language model (csrc/hip/ctc_beam.hip, the LM instantiations; csrc/host/ngram_lm.c)
against a float64 restatement of its semantics, against the acoustic-only call, the CTC loss and the host scorer, and the streaming
form against the one-shot call.

Reference: ``ref_row`` of ctc_reference.py -- the float64 prefix beam search (dicts of label tuples, linear space, the same candidate
cells, merge order and canonical-index tie rule) given the model (``Walk`` of ngram_cases.py): every entry carries an LM state, an extension is
multiplied by F(state, c) = exp(sum of alpha * backoff_logw along the walk + alpha * arc_logp + beta) (or the unknown-label factor),
and after the last frame every total is multiplied by E(state), zeros are dropped and the rest are ordered again, ties to the lower
rank.  The table's float32 inputs are taken as they are; everything else is float64.

Roundings.  r counts the float32 roundings (2^-24 each) that one frame can apply to a total.  The acoustic search has r = 4
(test_gpu_ctc_beam.py).  With a table whose longest backoff chain is D, an extension's factor is a product of up to D + 1 stored
factors, each rounded once when the table is built (D + 1), multiplied from left to right (D multiplies), and multiplied into the
mass (1): r = 4 + 2 D + 2.  The end-of-sentence step adds two more roundings once per row (E's own, and its multiply), so a reported
total carries at most r * T + 2 roundings.  Dense bigram: D = 1, r = 8; trigram: D = 2, r = 10.

Premise of every parity case, asserted in float64 on the reference: at every frame the relative gap between the W-th and the (W+1)-th
candidate total, and after the end-of-sentence step between adjacent hypotheses up to the one behind the last reported, is at least
4 * (r * T + 2) * 2^-24.  Score tolerance where the labels match: 2 * (r * T + 2) * 2^-24 + 4 * ulp_f32(|ref|).  The seeds are fixed
and meet the premise."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ctc_reference import (assert_scores, ctc_loss64 as _ctc_loss64, decode as _run_acoustic, drive as _drive, eq as _eq,
                           ref_row as _ref_row, reference as _reference, rounds as _rounds, softmax as _softmax, tol_lm as _tol)
from ngram_cases import Walk, dense_bigram, sparse_trigram
from nntoolkitcore_amd import capi, layers as NL

pytestmark = pytest.mark.gpu
INF = float("inf")
_assert_scores = functools.partial(assert_scores, allow=_tol)                  # (tag, rounds, got, ref)


def _run(gpu, p, lm, lens, blank, W, cutoff, nbest):
    return _run_acoustic(gpu, p, lens, blank, W, cutoff, nbest, lm)


# name: (posterior seed, B, T, C, W, cutoff, nbest, blank, lengths, table, alpha, beta, D)
TRI = lambda seed, C_, blank, **kw: ("tri", seed, C_, blank, kw)
PARITY = {
    "dense_bigram": (0, 2, 24, 12, 8, 0, 4, 11, None, ("bi", 1, 12, 11, {}), 0.75, 0.25, 1),
    "sparse_trigram": (0, 3, 32, 20, 8, 0, 4, 19, None, TRI(2, 20, 19, n_bi=8, n_tri=20, arcs0=12), 0.75, 0.25, 2),
    "unk_dead": (0, 2, 32, 20, 8, 0, 4, 19, None, TRI(2, 20, 19, n_bi=8, n_tri=20, arcs0=12, unk=-INF), 0.5, 0.0, 2),
    "ragged": (0, 4, 40, 9, 8, 0, 3, 8, [40, 0, 1, 17], TRI(3, 9, 8, n_bi=4, n_tri=8, arcs0=6, final=True), 0.75, 0.25, 2),
    "blank_mid": (0, 2, 32, 20, 8, 0, 4, 7, None, TRI(4, 20, 7, n_bi=8, n_tri=20, arcs0=12), 1.0, 0.5, 2),
    "final_reorders": (0, 2, 24, 12, 8, 0, 4, 11, None, ("bi", 5, 12, 11, dict(final=True)), 1.0, 0.0, 1),
    "class_cut": (0, 2, 24, 300, 8, 6, 2, 299, None, TRI(6, 300, 299, n_bi=40, n_tri=60, arcs0=150), 0.5, 0.25, 2),
    "cell_limit": (0, 1, 8, 128, 128, 0, 4, 127, None, TRI(7, 128, 127, n_bi=30, n_tri=60, arcs0=70), 0.5, 0.25, 2),
    "unstaged": (0, 1, 8, 12000, 1, 0, 1, 11999, None, TRI(8, 12000, 11999, n_bi=40, n_tri=60, arcs0=6000), 0.5, 0.25, 2),
}


def _make_table(spec):
    kind, seed, Cc, blank, kw = spec
    return dense_bigram(seed, Cc, blank, **kw) if kind == "bi" else sparse_trigram(seed, Cc, blank, **kw)


@functools.lru_cache(maxsize=None)
def _parity_case(name):
    seed, B, T, Cc, W, cutoff, nbest, blank, lens, spec, alpha, beta, D = PARITY[name]
    p = _softmax(seed, B, T, Cc)
    lens = [T] * B if lens is None else lens
    t = _make_table(spec)
    walk = Walk(t, alpha, beta)
    return p, lens, t, walk, _reference(p, lens, blank, W, cutoff, nbest, walk)


@pytest.mark.parametrize("name", list(PARITY))
def test_parity_with_the_float64_reference(gpu, name):
    """case 1: labels, lengths and padding equal, scores within the tolerance; r = 8 (bigram) or 10 (trigram), see the module text"""
    seed, B, T, Cc, W, cutoff, nbest, blank, _, spec, alpha, beta, D = PARITY[name]
    p, lens, t, walk, (lab, n, sc, gap, reordered) = _parity_case(name)
    rounds = _rounds(T, D)
    print("%s: smallest relative gap %.3g, premise %.3g; backoff depths %s, unknown %s, dead extensions %d, reordered %s"
          % (name, gap, 4 * rounds * 2.0 ** -24, sorted(walk.depths), walk.unk, walk.dead, reordered))
    assert gap >= 4 * rounds * 2.0 ** -24, "the premise does not hold for this seed"
    if name == "sparse_trigram":
        assert walk.depths >= {0, 1, 2} and walk.unk
    if name == "unk_dead":
        assert walk.dead > 0
    if name == "final_reorders":
        assert reordered
    lm = NL.NgramLm.from_arrays(alpha=alpha, beta=beta, **t)
    got_lab, got_n, got_sc = _run(gpu, p, lm, lens, blank, W, cutoff, nbest)
    lm.close()
    np.testing.assert_array_equal(got_n, n)
    np.testing.assert_array_equal(got_lab, lab)
    _assert_scores(name, rounds, got_sc, sc)


@pytest.mark.parametrize("cutoff", [0, 4])
def test_the_unit_model_gives_the_acoustic_bits(gpu, cutoff):
    """case 2: alpha = 0, beta = 0, no final_logp -- every factor is exactly one -- and lm = None, on ragged rows"""
    B, T, Cc, W, nbest, blank = 4, 40, 9, 8, 3, 8
    p = _softmax(6, B, T, Cc)
    lens = [40, 0, 1, 17]
    t = dict(sparse_trigram(3, Cc, blank, n_bi=4, n_tri=8, arcs0=6), final_logp=None, unk_logp=-INF)
    want = _run_acoustic(gpu, p, lens, blank, W, cutoff, nbest)
    lm = NL.NgramLm.from_arrays(alpha=0.0, beta=0.0, **t)
    _eq(_run(gpu, p, lm, lens, blank, W, cutoff, nbest), want, "unit model")
    _eq(_run(gpu, p, None, lens, blank, W, cutoff, nbest), want, "lm = None")
    lm.close()


def test_the_model_decides(gpu):
    """case 3: the acoustic top-1 and the fused top-1 differ (float64 first); the device agrees with each reference in its own call"""
    T, Cc, W, blank = 4, 4, 8, 3
    p = np.array([[[0.90, 0.04, 0.03, 0.03], [0.03, 0.03, 0.04, 0.90], [0.05, 0.50, 0.40, 0.05], [0.03, 0.04, 0.03, 0.90]]], np.float32)
    t = dense_bigram(1, Cc, blank)
    q = t["arc_begin"][1]                                   # state (0): after label 0, label 2 is likely and label 1 is not
    t["arc_logp"][q:q + 3] = [float(np.log(0.1)), float(np.log(0.1)), float(np.log(0.8))]
    walk = Walk(t, 1.0, 0.0)
    a_lab, a_n, a_sc, a_gap, _ = _reference(p, [T], blank, W, 0, 2, None)
    f_lab, f_n, f_sc, f_gap, _ = _reference(p, [T], blank, W, 0, 2, walk)
    assert list(a_lab[0, 0, :2]) == [0, 1] and list(f_lab[0, 0, :2]) == [0, 2] and a_n[0, 0] == f_n[0, 0] == 2
    assert min(a_gap, f_gap) >= 4 * _rounds(T, 1) * 2.0 ** -24
    lm = NL.NgramLm.from_arrays(alpha=1.0, beta=0.0, **t)
    got = _run(gpu, p, lm, [T], blank, W, 0, 2)
    np.testing.assert_array_equal(got[0], f_lab)
    _assert_scores("fused", _rounds(T, 1), got[2], f_sc)
    got = _run_acoustic(gpu, p, [T], blank, W, 0, 2)
    np.testing.assert_array_equal(got[0], a_lab)
    _assert_scores("acoustic", _rounds(T, 1), got[2], a_sc)
    lm.close()


def test_exhaustive_beam_equals_the_ctc_loss_plus_the_model_score(gpu):
    """case 4: nothing is ever pruned, so every score is ln(CTC likelihood) + the host scorer's sum with the end-of-sentence term"""
    T, Cc, W, blank = 5, 3, 128, 2
    p = _softmax(3, 1, T, Cc)
    t = dense_bigram(2, Cc, blank, final=True)
    beam, _ = _ref_row(p[0].astype(np.float64), blank, W, 0, Walk(t, 0.75, 0.25))
    nbest = len(beam)
    assert 20 < nbest <= 63
    lm = NL.NgramLm.from_arrays(alpha=0.75, beta=0.25, **t)
    lab, n, sc = _run(gpu, p, lm, [T], blank, W, 0, nbest)
    assert (n[0] >= 0).all() and len({tuple(lab[0, k, :n[0, k]]) for k in range(nbest)}) == nbest
    want = np.array([-_ctc_loss64(p[0], lab[0, k, :n[0, k]], blank) + lm.score(lab[0, k, :n[0, k]], with_final=True) for k in range(nbest)])
    _assert_scores("exhaustive", _rounds(T, 1), sc[0], want)
    assert (np.diff(sc[0]) <= 0).all()
    lm.close()


# ---- streaming ----
CH = dict(B=3, T=40, C=9, W=8, nbest=3, blank=8, lens=[40, 17, 1], mf=8)
IRREGULAR = [[5, 0, 1], [0, 3, 0], [8, 0, 0], [0, 0, 0], [2, 8, 0], [7, 1, 0], [1, 5, 0], [8, 0, 0], [0, 0, 0], [8, 0, 0], [1, 0, 0]]


def _ch_lm():
    return NL.NgramLm.from_arrays(alpha=0.75, beta=0.25, **sparse_trigram(3, CH["C"], CH["blank"], n_bi=4, n_tri=8, arcs0=6, final=True))


@pytest.mark.parametrize("schedule", ["frame_by_frame", "irregular"])
def test_every_chunking_gives_the_one_shot_bits(gpu, schedule):
    """case 5: after every push, every row equals the one-shot fused call on the frames it has seen (the E step included)"""
    B, T, Cc, W, nbest, blank, lens, mf = (CH[k] for k in ("B", "T", "C", "W", "nbest", "blank", "lens", "mf"))
    p = _softmax(0, B, T, Cc)
    lm = _ch_lm()
    pushes = [[1 if t < l else 0 for l in lens] for t in range(max(lens))] if schedule == "frame_by_frame" else IRREGULAR
    assert [sum(n[b] for n in pushes) for b in range(B)] == lens

    def check(i, pos, got):
        if schedule == "frame_by_frame" and i % 5 and i + 1 < len(pushes):
            return
        want = _run(gpu, p[:, :max(max(pos), 1)].copy(), lm, pos, blank, W, 0, nbest)
        for b in range(B):
            m = min(want[0].shape[2], T)
            np.testing.assert_array_equal(got[1][b], want[1][b], err_msg="push %d row %d" % (i, b))
            np.testing.assert_array_equal(got[0][b][:, :m], want[0][b][:, :m], err_msg="push %d row %d" % (i, b))
            assert (got[0][b][:, m:] == -1).all()
            np.testing.assert_array_equal(got[2][b].view(np.int32), want[2][b].view(np.int32), err_msg="push %d row %d" % (i, b))
    dec = NL.CtcBeamStream(B, mf, Cc, blank, W, 0, nbest, max_labels=T, lm=lm)
    _drive(gpu, dec, p, pushes, mf, after=check)
    dec.close()
    lm.close()


def test_final_reset_and_independence_of_the_other_rows_chunking(gpu):
    """case 5: a final flag and a reset start single rows again; a row's bits do not depend on how the other rows are chunked"""
    B, T, Cc, W, nbest, blank, lens, mf = (CH[k] for k in ("B", "T", "C", "W", "nbest", "blank", "lens", "mf"))
    p = _softmax(0, B, T, Cc)
    lm = _ch_lm()
    whole = _run(gpu, p, lm, lens, blank, W, 0, nbest)
    one = NL.CtcBeamStream(B, mf, Cc, blank, W, 0, nbest, max_labels=T, lm=lm)
    got = _drive(gpu, one, p, IRREGULAR, mf)
    _eq(got, whole, "irregular")
    two = NL.CtcBeamStream(B, mf, Cc, blank, W, 0, nbest, max_labels=T, lm=lm)
    largest = [[min(mf, max(0, l - i * mf)) for l in lens] for i in range((max(lens) + mf - 1) // mf)]
    finals = [[0, 1 if sum(n[1] for n in largest[:i + 1]) == lens[1] and largest[i][1] else 0, 0] for i in range(len(largest))]
    assert sum(f[1] for f in finals) == 1
    at_final = {}

    def keep(i, pos, got):
        if finals[i][1]:
            at_final["row 1"] = tuple(g[1].copy() for g in got)
    got = _drive(gpu, two, p, largest, mf, finals=finals, after=keep)
    for k in range(3):                                                         # row 1: the outputs of the push that carried its flag
        np.testing.assert_array_equal(at_final["row 1"][k].view(np.int32), whole[k][1].view(np.int32), err_msg="largest, row 1")
        np.testing.assert_array_equal(got[k][[0, 2]].view(np.int32), whole[k][[0, 2]].view(np.int32), err_msg="largest, rows 0 and 2")
    # ... after which it holds the empty prefix alone, with the end-of-sentence factor of the start state
    np.testing.assert_array_equal(got[1][1], [0, -1, -1])
    assert abs(float(got[2][1, 0]) - lm.score([], with_final=True)) <= 1e-6 and (got[0][1] == -1).all()
    # the push that completes row 1 carried its final flag: its outputs stood, and the row starts again; row 2 is reset by hand;
    # row 0 brings no frame and only has its n-best rewritten
    two.reset([2])
    _eq(_drive(gpu, two, p, [[0, 8, 1], [0, 8, 0], [0, 1, 0]], mf), whole, "after final and reset")
    for d in (one, two):
        d.close()
    lm.close()


def test_determinism_and_row_independence(gpu):
    """case 6"""
    B, T, Cc, W, nbest, blank = 4, 40, 9, 8, 3, 8
    p = _softmax(6, B, T, Cc)
    lens = [40, 23, 31, 0]
    lm = _ch_lm()
    one = _run(gpu, p, lm, lens, blank, W, 0, nbest)
    for a, c in zip(one, _run(gpu, p, lm, lens, blank, W, 0, nbest)):
        assert a.tobytes() == c.tobytes()
    alone = _run(gpu, p[2:3].copy(), lm, lens[2:3], blank, W, 0, nbest)
    for a, c in zip(one, alone):
        assert a[2].tobytes() == c[0].tobytes()
    q = p.copy()
    for b in range(B):
        q[b, lens[b]:] = np.nan
    for a, c in zip(one, _run(gpu, q, lm, lens, blank, W, 0, nbest)):
        assert a.tobytes() == c.tobytes()
    for cutoff in (Cc - 1, Cc + 5):
        for a, c in zip(one, _run(gpu, p, lm, lens, blank, W, cutoff, nbest)):
            assert a.tobytes() == c.tobytes(), cutoff
    lm.close()


def test_argument_errors_write_nothing(gpu):
    """case 7: -1, a message, the outputs and the head of the workspace as they were"""
    L = capi.load()
    B, T, Cc = 2, 6, 5
    x = torch.full((B, T, Cc), 0.2, device=gpu)
    xl = torch.full((B, T, 130), 1.0 / 130, device=gpu)
    dp = lambda t: C.c_void_p(t.data_ptr())
    lm5 = NL.NgramLm.from_arrays(alpha=1.0, beta=0.0, **dense_bigram(1, 5, 4))
    lm130 = NL.NgramLm.from_arrays(alpha=1.0, beta=0.0, **sparse_trigram(1, 130, 4, n_bi=4, n_tri=4, arcs0=8))
    lm6 = NL.NgramLm.from_arrays(alpha=1.0, beta=0.0, **dense_bigram(1, 6, 4))
    lmb = NL.NgramLm.from_arrays(alpha=1.0, beta=0.0, **dense_bigram(1, 5, 3))
    good = dict(il=[6, 4], blank=4, W=4, nbest=2, cut=0, C=Cc, lm=lm5)
    bad = [dict(lm=lm6), dict(lm=lmb), dict(il=[7, 4]), dict(il=[6, -1]), dict(blank=5), dict(blank=-1), dict(W=0), dict(W=129, nbest=1),
           dict(nbest=0), dict(nbest=5), dict(cut=-1), dict(W=128, C=130, nbest=1, lm=lm130), dict(misalign=1)]
    for change in bad:
        a = dict(good, **change)
        nb = max(a["nbest"], 1)
        lab = torch.full((B, nb, T), 7, dtype=torch.int32, device=gpu)
        n = torch.full((B, nb), 7, dtype=torch.int32, device=gpu)
        sc = torch.full((B, nb), 7.0, device=gpu)
        ws = torch.full((4096 + L.nntk_ctc_beam_lm_workspace_floats(B, T, a["C"], 128, 0),), 7.0, device=gpu)
        il = np.asarray(a["il"], np.int32)
        wsp = C.c_void_p(ws.data_ptr() + 4 * a.get("misalign", 0))
        rc = L.nntk_ctc_beam_decode_lm_device(dp(xl if a["C"] == 130 else x), B, T, a["C"], il.ctypes.data_as(capi.ip), a["blank"], a["W"],
                                              a["cut"], a["nbest"], a["lm"].h, dp(lab), dp(n), dp(sc), wsp)
        assert rc == -1 and capi.last_error() != "", {k: v for k, v in change.items() if k != "lm"}
        torch.cuda.synchronize()
        assert (lab == 7).all() and (n == 7).all() and (sc == 7.0).all() and (ws[:4096] == 7.0).all(), change
    for m in (lm5, lm130, lm6, lmb):
        m.close()


def test_host_form_equals_the_device_form(gpu):
    """case 8, on the ragged parity case"""
    seed, B, T, Cc, W, cutoff, nbest, blank, _, spec, alpha, beta, D = PARITY["ragged"]
    p, lens, t, _, _ = _parity_case("ragged")
    lm = NL.NgramLm.from_arrays(alpha=alpha, beta=beta, **t)
    dev = _run(gpu, p, lm, lens, blank, W, cutoff, nbest)
    host = NL.ctc_beam_decode_lm(p, lm, lens, blank, W, cutoff, nbest)
    for a, c in zip(dev, host):
        assert a.tobytes() == c.tobytes()
    lm.close()
