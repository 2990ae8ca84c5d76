"""RNN-Transducer beam search on the device (csrc/hip/rnnt_beam.hip) against tests/rnnt_beam_reference.py.

Labels and lengths are compared for EQUALITY with the float64 reference, so every case uses inputs on which the reference itself is
unambiguous: its smallest gap at a top-W cut of C or B (cut_gap) and between consecutive scores of the first nbest + 1 final
hypotheses (order_gap) are asserted to be at least GAP = 1e-3, and its float32 restatement must return the same labels
(rnnt_beam_cases.assert_premise; the seeds were chosen on the CPU for that, nothing about them comes from a device).  The tie case is the exception
by construction: exact ties, decided by the lower index in the reference and on the device.

Score tolerance, from the CPU alone: 4 x the largest |float32 restatement - float64| score over every case of tests/rnnt_beam_cases.py (score_tol; 4
because the device's summation order differs).  Measured: largest float32 error 3.383e-6 (the stream case: scores around -5), so the
tolerance is 1.353e-5; the device's largest error on these cases is 7.842e-7 (the awkward case), and 4.768e-7 against the device's own
transducer loss in the exhaustive case; both are printed by every test that compares scores."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from nntoolkitcore_amd import capi, layers as NL
from rnnt_beam_cases import assert_premise as _assert_premise, case as _case, ml as _ml, model as _model, reference as _reference, \
    score_tol as _score_tol
from rnnt_beam_device import assert_equals_reference, decoder as _decoder, host as _host, lattice_losses as _lattice_losses, same as _same, \
    to_device as _t

pytestmark = pytest.mark.gpu


def _decode(gpu, dec, c, enc=None, n=None, W=None, nbest=None):
    return _host(dec.beam_decode(_t(gpu, c["enc"] if enc is None else enc), c["n"] if n is None else n, W or c["W"], nbest or c["nbest"],
                                 _ml(c)))


def _check(gpu, name):
    _assert_premise(name)
    c = _case(name)
    dec = _decoder(gpu, c)
    got = _decode(gpu, dec, c)
    dec.destroy()
    assert_equals_reference(name, got, _reference(name)[0], c["nbest"], _score_tol)
    return c, got


@pytest.mark.parametrize("blank", [0, 2])
def test_exhaustive_search_equals_the_loss(gpu, blank):
    """V 3, at most 2 labels, S 2, W = nbest = 8: nothing is pruned, the 7 sequences come back with 1 empty slot, each score is minus
    the device's own transducer loss on that sequence's lattice, and the masses sum to at most 1"""
    m = _model(3 + blank, 3, 7, 13, 22, True, blank=blank)
    c = dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, (3, 4, 22)).astype(np.float32), n=[4, 2, 3], act="tanh", ms=2, W=8, nbest=8, max_labels=2)
    dec = _decoder(gpu, c)
    labels, lengths, scores = _decode(gpu, dec, c)
    dec.destroy()
    lab = [v for v in range(3) if v != blank]
    want = sorted([()] + [(a,) for a in lab] + list(itertools.product(lab, lab)))
    pairs = []
    for b in range(3):
        got = [tuple(labels[b, k, :lengths[b, k]].tolist()) for k in range(7)]
        assert sorted(got) == want and lengths[b, 7] == -1 and scores[b, 7] == -np.inf and (labels[b, 7] == -1).all(), (b, got)
        assert all(scores[b, k] >= scores[b, k + 1] for k in range(6))
        pairs += [(b, y) for y in got]
    loss = _lattice_losses(gpu, c, pairs)
    err = np.abs(loss + scores[:, :7].reshape(-1)).max()
    print("largest |score + loss| %.3e (tolerance %.3e)" % (err, _score_tol()))
    assert err <= _score_tol()
    for b in range(3):
        assert np.exp(scores[b, :7].astype(np.float64)).sum() <= 1.0 + _score_tol()


@pytest.mark.parametrize("name", ["awkward", "awkward_w3", "awkward_w1", "big_v", "wide_identity", "stream"])
def test_equals_the_float64_reference(gpu, name):
    c, (labels, lengths, scores) = _check(gpu, name)
    if name.startswith("awkward"):
        assert lengths[2, 0] == 0 and scores[2, 0] == 0.0 and (lengths[2, 1:] == -1).all()      # the row without frames
        assert c["m"]["E"] % 4 and c["m"]["H"] % 4 and c["m"]["J"] % 4 and c["m"]["V"] % 64
    if name == "big_v":
        assert c["m"]["V"] > 1024 and c["m"]["proj"] is None and c["m"]["H"] == c["m"]["J"]


def test_merges_cuts_and_the_label_limit(gpu):
    r64 = _reference("pruned")[0]
    assert r64["merges"].sum() > 0 and r64["cuts"].sum() > 0 and r64["at_max"].sum() > 0, (r64["merges"], r64["cuts"], r64["at_max"])
    assert any(len(y) == 3 for y in r64["labels"][0])
    _check(gpu, "pruned")


def test_exact_ties_go_to_the_lower_index(gpu):
    r64 = _reference("tie")[0]
    assert r64["cut_gap"][0] == 0.0 and r64["order_gap"][0] == 0.0                   # ties at a cut and in the final order
    assert r64["labels"][0] == [[1], [3], []] and r64["scores"][0][0] == r64["scores"][0][1]      # equal mass: (1,) was inserted first
    c = _case("tie")
    dec = _decoder(gpu, c)
    got = _decode(gpu, dec, c)
    dec.destroy()
    assert_equals_reference("tie", got, r64, c["nbest"], _score_tol)
    assert got[2][0, 0] == got[2][0, 1]


def test_group_of_four_and_one_by_one_give_the_same_bits(gpu):
    L = capi.load()
    c = _case("awkward")
    m = c["m"]
    dec = _decoder(gpu, c)
    try:
        for W in (3, 5, 8):                                                          # W no multiple of the group, and one that is
            assert L.nntk_shim_rnnt_beam_group(W, m["H"], m["J"], m["V"]) == 4
            auto = _decode(gpu, dec, c, W=W, nbest=min(3, W))
            L.nntk_shim_rnnt_beam_set_group(1)
            assert L.nntk_shim_rnnt_beam_group(W, m["H"], m["J"], m["V"]) == 1
            single = _decode(gpu, dec, c, W=W, nbest=min(3, W))
            L.nntk_shim_rnnt_beam_set_group(0)
            assert _same(auto, single), W
    finally:
        L.nntk_shim_rnnt_beam_set_group(0)
        dec.destroy()


def test_nan_in_the_padding_changes_no_bit(gpu):
    c = _case("awkward")
    dec = _decoder(gpu, c)
    clean = _decode(gpu, dec, c)
    enc = c["enc"].copy()
    for b, n in enumerate(c["n"]):
        enc[b, n:] = np.nan
    dirty = _decode(gpu, dec, c, enc=enc)
    dec.destroy()
    assert _same(clean, dirty) and not np.isnan(dirty[2]).any()


def test_rows_are_independent_of_batch_position_and_neighbours(gpu):
    c = _case("awkward")
    dec = _decoder(gpu, c)
    base = _decode(gpu, dec, c)
    rng = np.random.default_rng(11)
    for B in (1, 4):
        for b in range(3):
            T = 9 if B > 1 else max(c["n"][b], 1)                                    # alone: without the T padding as well
            enc = rng.uniform(-1.5, 1.5, (B, T, 22)).astype(np.float32)
            n = rng.integers(0, T + 1, B).astype(np.int32)
            at = (B - 1 - b) if B > 1 else 0
            enc[at, :T] = c["enc"][b, :T]
            n[at] = c["n"][b]
            got = _decode(gpu, dec, c, enc=enc, n=n)
            assert all(np.array_equal(g[at].view(np.int32), ref[b].view(np.int32)) for g, ref in zip(got, base)), (B, b)
    dec.destroy()


def test_two_calls_return_the_same_bits(gpu):
    c = _case("wide_identity")
    dec = _decoder(gpu, c)
    a, b = _decode(gpu, dec, c), _decode(gpu, dec, c)
    dec.destroy()
    assert _same(a, b)


def test_streaming_equals_the_one_shot_call_after_every_push(gpu):
    c = _case("stream")
    B, T, J = c["enc"].shape
    dec = _decoder(gpu, c)
    singles = [[1, 1, 1 if i < 7 else 0] for i in range(12)]
    ragged = [[5, 3, 0], [0, 0, 0], [7, 9, 7]]
    for splits in (singles, ragged):
        s = NL.RnntBeamStream(dec, B, c["W"], c["nbest"], _ml(c))
        seen = [0] * B
        for split in splits:
            w = max(max(split), 1)
            chunk = np.full((B, w, J), np.nan, np.float32)
            for b in range(B):
                chunk[b, :split[b]] = c["enc"][b, seen[b]:seen[b] + split[b]]
                seen[b] += split[b]
            got = _host(s.push(_t(gpu, chunk), split))
            assert _same(got, _decode(gpu, dec, c, n=seen)), (splits, seen)           # the one-shot call on the frames so far
        assert seen == c["n"]
        one = _decode(gpu, dec, c)
        s.reset([1])                                                                 # row 1 restarts, the others stay
        chunk = np.full((B, 12, J), np.nan, np.float32)
        chunk[1] = c["enc"][1]
        assert _same(_host(s.push(_t(gpu, chunk), [0, 12, 0])), one)
        s.reset()
        assert _same(_host(s.push(_t(gpu, c["enc"]), c["n"])), one)
        s.close()
    dec.destroy()


def test_host_form_equals_the_device_form(gpu):
    c = _case("awkward")
    m = c["m"]
    dec = _decoder(gpu, c)
    dev = _decode(gpu, dec, c)
    dec.destroy()
    got = NL.rnnt_beam_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], c["n"], beam_width=c["W"], nbest=c["nbest"],
                              max_labels=_ml(c), blank=m["blank"], joint_activation=c["act"], max_symbols_per_frame=c["ms"])
    assert _same(got, dev)


def test_sizes_are_monotone_and_refusals_write_nothing(gpu):
    """the size functions on a live decoder, then every refusal of the decode call and of the state: -1 / NULL, a message, outputs,
    workspace and state untouched"""
    L = capi.load()
    c = _case("stream")
    dec = _decoder(gpu, c)
    for f in (L.nntk_rnnt_beam_workspace_floats, L.nntk_rnnt_beam_state_bytes):
        base = (3, 4, 6)
        v0 = f(dec.h, *base)
        assert v0 > 0 and f(dec.h, 0, 4, 6) == 0 and f(dec.h, -1, 4, 6) == 0
        for i in range(3):
            prev = v0
            for step in (1, 2):
                v = f(dec.h, *[x + (step if j == i else 0) for j, x in enumerate(base)])
                assert v >= prev
                prev = v
            assert prev > v0 or (f is L.nntk_rnnt_beam_workspace_floats and i == 2 and c["ms"] < 6)
    B, T, J = c["enc"].shape
    W, NB, ML = c["W"], c["nbest"], _ml(c)
    enc = _t(gpu, c["enc"])
    one = _decode(gpu, dec, c)
    st = NL.RnntBeamStream(dec, B, W, NB, ML)
    st.push(enc[:, :5].contiguous(), [5, 5, 5])
    need = L.nntk_rnnt_beam_workspace_floats(dec.h, B, W, ML)
    buf = torch.full((B * NB * ML + 2 * B * NB + 8,), 7, dtype=torch.int32, device=gpu)
    lab, ln = buf[:B * NB * ML], buf[B * NB * ML:B * NB * ML + B * NB]
    sc = torch.full((B * NB,), 7.0, device=gpu)
    ws = torch.full((need + 8,), 7.0, device=gpu)
    assert ws.data_ptr() % 16 == 0
    p = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())
    ip = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(capi.ip)
    good = dict(d=dec.h, s=None, enc=enc, B=B, T=T, n=c["n"], W=W, NB=NB, ML=ML, lab=lab, ln=ln, sc=sc, ws=ws)
    bad = [("NULL decoder", dict(d=None), "NULL"), ("NULL enc", dict(enc=None), "NULL"), ("NULL labels", dict(lab=None), "NULL"),
           ("NULL lengths", dict(ln=None), "NULL"), ("NULL scores", dict(sc=None), "NULL"), ("NULL workspace", dict(ws=None), "NULL"),
           ("beam_width 0", dict(W=0), "beam_width"), ("beam_width 33", dict(W=33), "beam_width"), ("nbest 0", dict(NB=0), "nbest"),
           ("nbest > beam_width", dict(NB=W + 1), "nbest"), ("max_labels 0", dict(ML=0), "max_labels"),
           ("n_frames > T", dict(n=[12, 13, 7]), "n_frames"), ("n_frames < 0", dict(n=[12, -1, 7]), "n_frames"),
           ("batch differs from the state's", dict(s=st.h, B=B - 1, n=[12, 12]), "state"),
           ("beam_width differs from the state's", dict(s=st.h, W=W + 1), "state"),
           ("max_labels differs from the state's", dict(s=st.h, ML=ML + 1), "state"),
           ("misaligned enc", dict(enc=enc.data_ptr() + 2), "aligned"), ("misaligned labels", dict(lab=lab.data_ptr() + 1), "aligned"),
           ("misaligned workspace", dict(ws=ws.data_ptr() + 4), "16-byte"),
           ("lengths overlap labels", dict(ln=lab.data_ptr() + 8), "overlaps"), ("scores overlap enc", dict(sc=enc.data_ptr() + 16), "overlaps"),
           ("labels overlap enc", dict(lab=enc.data_ptr()), "overlaps"), ("scores overlap the workspace", dict(sc=ws.data_ptr() + 32), "overlaps"),
           ("labels overlap the workspace's end", dict(lab=ws.data_ptr() + 4 * (need - 1)), "overlaps")]
    for name, change, word in bad:
        a = dict(good, **change)
        rc = L.nntk_rnnt_beam_decode_device(a["d"], a["s"], p(a["enc"]), a["B"], a["T"], ip(a["n"]), a["W"], a["NB"], a["ML"], p(a["lab"]),
                                            p(a["ln"]), p(a["sc"]), p(a["ws"]))
        torch.cuda.synchronize()
        assert rc == -1 and word in capi.last_error(), (name, capi.last_error())
        assert (buf == 7).all() and (sc == 7.0).all() and (ws == 7.0).all() and torch.equal(enc.cpu(), torch.from_numpy(c["enc"])), name
    other = _decoder(gpu, c)
    assert L.nntk_rnnt_beam_decode_device(other.h, st.h, p(enc), B, T, ip(c["n"]), W, NB, ML, p(lab), p(ln), p(sc), p(ws)) == -1
    assert "another decoder" in capi.last_error()
    other.destroy()
    assert not L.nntk_rnnt_beam_state_create(dec.h, 0, W, ML) and "batch" in capi.last_error()
    assert not L.nntk_rnnt_beam_state_create(dec.h, B, 33, ML) and "beam_width" in capi.last_error()
    assert not L.nntk_rnnt_beam_state_create(dec.h, B, W, 0) and "max_labels" in capi.last_error()
    assert L.nntk_rnnt_beam_state_reset(st.h, ip([3]), 1) == -1 and "rows" in capi.last_error()
    assert L.nntk_rnnt_beam_state_reset(st.h, None, 2) == -1 and "NULL" in capi.last_error()
    torch.cuda.synchronize()
    assert (buf == 7).all() and (sc == 7.0).all() and (ws == 7.0).all()
    # ... and the state is where the first push left it: the rest of the stream gives the one-shot result
    rest = _host(st.push(enc[:, 5:].contiguous(), [7, 7, 2]))
    assert _same(rest, one)
    st.close(); dec.destroy()
