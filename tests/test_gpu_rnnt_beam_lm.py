"""RNN-Transducer beam search fused with an n-gram language model on the device (csrc/hip/rnnt_beam.hip, the LM instantiations;
csrc/host/rnnt_decode.c, ngram_lm.c) against tests/rnnt_beam_reference.py, against the acoustic call, the device's own transducer loss
with the host scorer, and the streaming form against the one-shot call.

The rules are those of test_gpu_rnnt_beam.py.  Labels and lengths are compared for EQUALITY with the float64 reference, on cases whose
premises (gaps of at least GAP = 1e-3 at every cut and in the reported order, the float32 restatement returning the same labels, a
backoff and an unknown label met by the sparse tables) tests/test_rnnt_beam_lm_host.py asserts on the CPU; the exact-tie case is the
exception by construction.  Score tolerance, from the CPU alone: 4 x the largest |float32 restatement - float64| reported score over
the cases of tests/rnnt_beam_lm_cases.py (4 because the device's summation order differs), printed with the device's largest error by
every test that compares scores.  Measured: largest float32 error 2.043e-6, so the tolerance is 8.171e-6; the device's largest error
on these cases is 1.018e-6 (wide_identity), and 5.662e-7 against the device's own transducer loss in the exhaustive cases, whose
tolerance is that of the acoustic exhaustive test (1.353e-5).  Every table has alpha a power of two."""
import ctypes as C

import numpy as np
import pytest
import torch

import rnnt_beam_lm_cases as K
import rnnt_beam_reference as RB
from nntoolkitcore_amd import capi, layers as NL
from rnnt_beam_cases import ml as _ml, score_tol as _acoustic_score_tol
from rnnt_beam_device import assert_equals_reference, decoder as _decoder, host as _host, lattice_losses as _lattice_losses, same as _same, \
    to_device as _t

pytestmark = pytest.mark.gpu


def _lm(name):
    t, alpha, beta = K.table(name)
    return NL.NgramLm.from_arrays(alpha=alpha, beta=beta, **t)


def _unit_lm(c):
    """alpha = beta = 0, no final_logp: every term is +0.0"""
    t = dict(K.table("awkward" if c["m"]["V"] == 5 else "wide_identity")[0], final_logp=None)
    return NL.NgramLm.from_arrays(alpha=0.0, beta=0.0, **t)


def _decode(gpu, dec, c, lm, enc=None, n=None, W=None, nbest=None):
    return _host(dec.beam_decode(_t(gpu, c["enc"] if enc is None else enc), c["n"] if n is None else n, W or c["W"], nbest or c["nbest"],
                                 _ml(c), lm=lm))


def _check(gpu, name):
    c = K.case(name)
    dec, lm = _decoder(gpu, c), _lm(name)
    got = _decode(gpu, dec, c, lm)
    dec.destroy(); lm.close()
    assert_equals_reference(name, got, K.reference(name)[0], c["nbest"], K.score_tol)
    return c, got


@pytest.mark.parametrize("name", K.PARITY + ("stream",))
def test_equals_the_float64_reference(gpu, name):
    K.assert_premise(name)
    c, (labels, lengths, scores) = _check(gpu, name)
    if name.startswith("awkward"):                   # the row without frames: the empty hypothesis with ln E(start_state)
        ref = RB.Lm(*K.table(name))
        assert lengths[2, 0] == 0 and scores[2, 0] == np.float32(ref.final_ln[ref.start]) and (lengths[2, 1:] == -1).all()
    if name == "big_v":                              # the scatter over state 0's arcs strides the workgroup more than once
        t = K.table(name)[0]
        assert t["arc_begin"][1] - t["arc_begin"][0] > 1024 and c["m"]["V"] > 1024


@pytest.mark.parametrize("W", [1, 8])
def test_a_unit_model_and_no_model_give_the_acoustic_bits(gpu, W):
    L = capi.load()
    for name in ("awkward", "wide_identity"):
        c = K.case(name)
        nb = min(W, c["nbest"])
        dec, unit = _decoder(gpu, c), _unit_lm(c)
        want = _host(dec.beam_decode(_t(gpu, c["enc"]), c["n"], W, nb, _ml(c)))
        assert _same(_decode(gpu, dec, c, unit, W=W, nbest=nb), want), (name, W, "unit model")
        # lm == NULL through the _lm entry point, on the acoustic workspace
        enc = _t(gpu, c["enc"])
        B, T, _ = c["enc"].shape
        outs, ws = dec._beam_outputs(enc.device, B, nb, _ml(c)), dec._beam_workspace(enc.device, B, W, _ml(c))
        p = lambda t: C.c_void_p(t.data_ptr())
        n = np.ascontiguousarray(c["n"], np.int32)
        assert L.nntk_rnnt_beam_decode_lm_device(dec.h, None, p(enc), B, T, n.ctypes.data_as(capi.ip), W, nb, _ml(c), None, p(outs[0]),
                                                 p(outs[1]), p(outs[2]), p(ws)) == 0, capi.last_error()
        assert _same(_host(outs), want), (name, W, "no model")
        dec.destroy(); unit.close()


def test_the_model_decides(gpu):
    K.assert_premise("decides")
    a, r = K.acoustic_reference("decides"), K.reference("decides")[0]
    assert any(a["labels"][b][0] != r["labels"][b][0] for b in range(2))
    c, fused = _check(gpu, "decides")
    dec = _decoder(gpu, c)
    plain = _decode(gpu, dec, c, None)
    dec.destroy()
    for b in range(2):
        assert plain[0][b, 0, :plain[1][b, 0]].tolist() == a["labels"][b][0] and fused[0][b, 0, :fused[1][b, 0]].tolist() == r["labels"][b][0]


@pytest.mark.parametrize("name", ["exhaustive3", "exhaustive4"])
def test_exhaustive_search_minus_the_model_is_minus_the_loss(gpu, name):
    c = K.case(name)
    r64 = K.reference(name)[0]
    assert r64["cuts"].sum() == 0
    dec, lm = _decoder(gpu, c), _lm(name)
    labels, lengths, scores = _decode(gpu, dec, c, lm)
    dec.destroy()
    pairs, fused = [], []
    for b in range(len(c["n"])):
        count = len(r64["final"][b])
        got = [labels[b, k, :lengths[b, k]].tolist() for k in range(count)]
        assert got == [r[0] for r in r64["final"][b]] and (lengths[b, count:] == -1).all(), (b, got)
        pairs += [(b, y) for y in got]
        fused += [float(scores[b, k]) - lm.score(y, with_final=True) for k, y in enumerate(got)]
    lm.close()
    loss = _lattice_losses(gpu, c, pairs)
    err = np.abs(loss + np.array(fused)).max()
    tol = _acoustic_score_tol()                     # the existing exhaustive test's (tests/test_gpu_rnnt_beam.py)
    print("largest |score - model + loss| %.3e (tolerance %.3e)" % (err, tol))
    assert err <= tol


def test_a_zero_mass_arc_appears_in_no_hypothesis(gpu):
    K.assert_premise("zero_arc")
    t = K.table("awkward")[0]
    c = K.case("zero_arc")
    dec, lm, full = _decoder(gpu, c), _lm("zero_arc"), _lm("awkward")
    labels, lengths, scores = _decode(gpu, dec, c, lm, nbest=c["W"])
    # the (context label, label) pairs of the zeroed arcs: with blank 0, state s > 0 of the dense bigram is the context (s)
    banned = set()
    for q in K.zero_arcs():
        s = max(i for i in range(len(t["arc_begin"]) - 1) if t["arc_begin"][i] <= q)
        assert s > 0
        banned.add((s, t["arc_label"][q]))
    seen_with = _decode(gpu, dec, c, full, nbest=c["W"])
    hit = lambda lab, ln: any((y[i], y[i + 1]) in banned for b in range(2) for k in range(c["W"]) if ln[b, k] > 0
                              for y in [lab[b, k, :ln[b, k]].tolist()] for i in range(len(y) - 1))
    assert hit(seen_with[0], seen_with[1]) and not hit(labels, lengths) and np.isfinite(scores[lengths >= 0]).all()
    dec.destroy(); lm.close(); full.close()
    _check(gpu, "zero_arc")


def test_the_end_of_sentence_term_drops_reorders_and_leaves_the_beam(gpu):
    K.assert_premise("final_drop")
    best = K.reference("awkward")[0]["labels"][0][0]
    c, (labels, lengths, _) = _check(gpu, "final_drop")
    assert all(labels[0, k, :lengths[0, k]].tolist() != best for k in range(c["nbest"]))
    # a reordering with an exact tie: [1] and [3] stay in the order of A behind the empty hypothesis, with equal scores
    r = K.reference("final_tie")[0]
    assert r["labels"][0] == [[], [1], [3]] and [y for y, _, _ in r["carried"][0]] == [[1], [3], []]
    _, (_, _, scores) = _check(gpu, "final_tie")
    assert scores[0, 1] == scores[0, 2]
    # the carried beam is A, not the report: pushes with the dropping table give the one-shot call's bits
    for name in ("final_drop", "final_tie"):
        c = K.case(name)
        B, T, _ = c["enc"].shape
        dec, lm = _decoder(gpu, c), _lm(name)
        s = NL.RnntBeamStream(dec, B, c["W"], c["nbest"], _ml(c), lm=lm)
        for lo, hi in ((0, 2), (2, T)):
            split = [max(0, min(n, hi) - lo) for n in c["n"]]
            got = _host(s.push(_t(gpu, c["enc"][:, lo:hi]), split))
            assert _same(got, _decode(gpu, dec, c, lm, n=[min(n, hi) for n in c["n"]])), (name, hi)
        s.close(); dec.destroy(); lm.close()


def test_streaming_equals_the_one_shot_call_after_every_push(gpu):
    c = K.case("stream")
    B, T, J = c["enc"].shape
    dec, lm = _decoder(gpu, c), _lm("stream")
    singles = [[1, 1, 1 if i < 7 else 0] for i in range(12)]
    ragged = [[5, 3, 0], [0, 0, 0], [7, 9, 7]]
    for splits in (singles, ragged):
        s = NL.RnntBeamStream(dec, B, c["W"], c["nbest"], _ml(c), lm=lm)
        seen = [0] * B
        for split in splits:
            w = max(max(split), 1)
            chunk = np.full((B, w, J), np.nan, np.float32)
            for b in range(B):
                chunk[b, :split[b]] = c["enc"][b, seen[b]:seen[b] + split[b]]
                seen[b] += split[b]
            got = _host(s.push(_t(gpu, chunk), split))
            assert _same(got, _decode(gpu, dec, c, lm, n=seen)), (splits, seen)          # the one-shot call on the frames so far
        assert seen == c["n"]
        one = _decode(gpu, dec, c, lm)
        s.reset([1])                                                                 # row 1 restarts, the others stay
        chunk = np.full((B, 12, J), np.nan, np.float32)
        chunk[1] = c["enc"][1]
        assert _same(_host(s.push(_t(gpu, chunk), [0, 12, 0])), one)
        s.reset()
        assert _same(_host(s.push(_t(gpu, c["enc"]), c["n"])), one)
        s.close()
    # another row's chunking changes nothing: row 0 in one push, rows 1 and 2 frame by frame
    s = NL.RnntBeamStream(dec, B, c["W"], c["nbest"], _ml(c), lm=lm)
    one = _decode(gpu, dec, c, lm)
    for i in range(12):
        chunk = np.full((B, 12 if i == 0 else 1, J), np.nan, np.float32)
        split = [12 if i == 0 else 0, 1, 1 if i < 7 else 0]
        chunk[0, :split[0]] = c["enc"][0, :split[0]]
        for b in (1, 2):
            chunk[b, :split[b]] = c["enc"][b, i:i + split[b]]
        got = _host(s.push(_t(gpu, chunk), split))
        assert all(np.array_equal(g[0].view(np.int32), o[0].view(np.int32)) for g, o in zip(got, one)), i
    assert _same(got, one)
    s.close(); dec.destroy(); lm.close()


def test_group_of_four_and_one_by_one_give_the_same_bits(gpu):
    L = capi.load()
    c = K.case("awkward")
    m = c["m"]
    dec, lm = _decoder(gpu, c), _lm("awkward")
    try:
        for W in (3, 5, 8):
            assert L.nntk_shim_rnnt_beam_group(W, m["H"], m["J"], m["V"]) == 4
            auto = _decode(gpu, dec, c, lm, W=W, nbest=min(3, W))
            L.nntk_shim_rnnt_beam_set_group(1)
            assert L.nntk_shim_rnnt_beam_group(W, m["H"], m["J"], m["V"]) == 1
            single = _decode(gpu, dec, c, lm, W=W, nbest=min(3, W))
            L.nntk_shim_rnnt_beam_set_group(0)
            assert _same(auto, single), W
    finally:
        L.nntk_shim_rnnt_beam_set_group(0)
        dec.destroy(); lm.close()


def test_padding_neighbours_and_repetition_change_no_bit(gpu):
    c = K.case("awkward")
    dec, lm = _decoder(gpu, c), _lm("awkward")
    base = _decode(gpu, dec, c, lm)
    assert _same(base, _decode(gpu, dec, c, lm))                                     # two calls
    enc = c["enc"].copy()
    for b, n in enumerate(c["n"]):
        enc[b, n:] = np.nan
    dirty = _decode(gpu, dec, c, lm, enc=enc)
    assert _same(base, dirty) and not np.isnan(dirty[2]).any()                       # NaN in the padded frames
    rng = np.random.default_rng(11)
    for B in (1, 4):                                                                 # another batch position, other neighbours, no T padding
        for b in range(3):
            T = 9 if B > 1 else max(c["n"][b], 1)
            enc = rng.uniform(-1.5, 1.5, (B, T, 22)).astype(np.float32)
            n = rng.integers(0, T + 1, B).astype(np.int32)
            at = (B - 1 - b) if B > 1 else 0
            enc[at, :T] = c["enc"][b, :T]
            n[at] = c["n"][b]
            got = _decode(gpu, dec, c, lm, enc=enc, n=n)
            assert all(np.array_equal(g[at].view(np.int32), ref[b].view(np.int32)) for g, ref in zip(got, base)), (B, b)
    dec.destroy(); lm.close()


def test_host_form_equals_the_device_form(gpu):
    c = K.case("awkward")
    m = c["m"]
    dec, lm = _decoder(gpu, c), _lm("awkward")
    dev = _decode(gpu, dec, c, lm)
    dec.destroy()
    got = NL.rnnt_beam_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], c["n"], beam_width=c["W"], nbest=c["nbest"],
                              max_labels=_ml(c), blank=m["blank"], joint_activation=c["act"], max_symbols_per_frame=c["ms"], lm=lm)
    lm.close()
    assert _same(got, dev)


def test_sizes_and_refusals_write_nothing(gpu):
    L = capi.load()
    c = K.case("stream")
    dec, lm, other_lm = _decoder(gpu, c), _lm("stream"), _lm("stream")
    wrong_v, t6 = _lm("awkward"), K.table("stream")[0]                                # V 5 against the decoder's 6
    wrong_blank = NL.NgramLm.from_arrays(**dict(K.table("exhaustive4")[0], n_classes=6))      # blank 1 against the decoder's 2
    assert t6["n_classes"] == 6 and t6["blank"] == 2
    B, T, J = c["enc"].shape
    W, NB, ML = c["W"], c["nbest"], _ml(c)
    need, plain = L.nntk_rnnt_beam_lm_workspace_floats(dec.h, B, W, ML), L.nntk_rnnt_beam_workspace_floats(dec.h, B, W, ML)
    pad = lambda x: (x + 3) & ~3
    assert need == plain + B * (pad((min(c["ms"], ML) + 2) * W) + pad(2 * W * 6))
    assert L.nntk_rnnt_beam_state_bytes_lm(dec.h, B, W, ML) == L.nntk_rnnt_beam_state_bytes(dec.h, B, W, ML) + 4 * B * W
    assert L.nntk_rnnt_beam_lm_workspace_floats(dec.h, 0, W, ML) == 0 and L.nntk_rnnt_beam_state_bytes_lm(dec.h, B, 33, ML) == 0
    enc = _t(gpu, c["enc"])
    one = _decode(gpu, dec, c, lm)
    st = NL.RnntBeamStream(dec, B, W, NB, ML, lm=lm)
    st.push(enc[:, :5].contiguous(), [5, 5, 5])
    st_plain = NL.RnntBeamStream(dec, B, W, NB, ML)
    buf = torch.full((B * NB * ML + 2 * B * NB + 8,), 7, dtype=torch.int32, device=gpu)
    lab, ln = buf[:B * NB * ML], buf[B * NB * ML:B * NB * ML + B * NB]
    sc = torch.full((B * NB,), 7.0, device=gpu)
    ws = torch.full((need + 8,), 7.0, device=gpu)
    p = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())
    ip = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(capi.ip)
    good = dict(d=dec.h, s=None, enc=enc, B=B, T=T, n=c["n"], W=W, NB=NB, ML=ML, lm=lm.h, lab=lab, ln=ln, sc=sc, ws=ws)
    bad = [("NULL decoder", dict(d=None), "NULL"), ("NULL enc", dict(enc=None), "NULL"), ("NULL labels", dict(lab=None), "NULL"),
           ("NULL workspace", dict(ws=None), "NULL"), ("beam_width 33", dict(W=33), "beam_width"), ("nbest 0", dict(NB=0), "nbest"),
           ("max_labels 0", dict(ML=0), "max_labels"), ("n_frames > T", dict(n=[12, 13, 7]), "n_frames"),
           ("beam_width differs from the state's", dict(s=st.h, W=W + 1), "state"), ("misaligned workspace", dict(ws=ws.data_ptr() + 4), "16-byte"),
           ("scores overlap the workspace", dict(sc=ws.data_ptr() + 32), "overlaps"),
           ("labels overlap the model's part of the workspace", dict(lab=ws.data_ptr() + 4 * (need - 1)), "overlaps"),
           ("a model for another class count", dict(lm=wrong_v.h), "class count"), ("a model for another blank", dict(lm=wrong_blank.h), "blank"),
           ("a state without a model", dict(s=st_plain.h), "without a language model"),
           ("a state with a model, the call without", dict(s=st.h, lm=None), "with a language model"),
           ("a state with another model", dict(s=st.h, lm=other_lm.h), "another language model")]
    for name, change, word in bad:
        a = dict(good, **change)
        rc = L.nntk_rnnt_beam_decode_lm_device(a["d"], a["s"], p(a["enc"]), a["B"], a["T"], ip(a["n"]), a["W"], a["NB"], a["ML"], a["lm"],
                                               p(a["lab"]), p(a["ln"]), p(a["sc"]), p(a["ws"]))
        torch.cuda.synchronize()
        assert rc == -1 and word in capi.last_error(), (name, capi.last_error())
        assert (buf == 7).all() and (sc == 7.0).all() and (ws == 7.0).all(), name
    # the acoustic entry point refuses a state that carries a model, and the state constructor a model that does not fit
    assert L.nntk_rnnt_beam_decode_device(dec.h, st.h, p(enc), B, T, ip(c["n"]), W, NB, ML, p(lab), p(ln), p(sc), p(ws)) == -1
    assert "with a language model" in capi.last_error()
    assert not L.nntk_rnnt_beam_state_create_lm(dec.h, B, W, ML, wrong_v.h) and "class count" in capi.last_error()
    torch.cuda.synchronize()
    assert (buf == 7).all() and (sc == 7.0).all() and (ws == 7.0).all()
    rest = _host(st.push(enc[:, 5:].contiguous(), [7, 7, 2]))                        # the state is where the first push left it
    assert _same(rest, one)
    for o in (st, st_plain, lm, other_lm, wrong_v, wrong_blank):
        o.close()
    dec.destroy()
