"""Label timestamps, confidences and length normalisation of the transducer beam search on the device (csrc/hip/rnnt_beam.hip, the
DETAIL instantiations) against tests/rnnt_beam_reference.py.

Labels, lengths and FRAMES are compared for equality with the float64 reference, so every case is one on which the reference is
unambiguous (tests/rnnt_beam_detail_cases.py, checked without a device by tests/test_rnnt_beam_detail_host.py and again here): cut,
order, lead and key gaps of at least GAP = 1e-3 and a float32 restatement with the same labels and frames; the tie case by its rule.
Labels, lengths and scores with detail on are compared BIT FOR BIT with the calls that existed before.

Confidences: label_logps[j] against log_softmax(lattice_logits(labels)[frames[j]][j])[labels[j]] in float64, whatever the merge rule
chose.  Tolerance, from the CPU alone: 4 x the largest |float32 restatement - float64| over the lps of all cases (4: the device's
summation order differs).  Measured on the CPU: largest float32 error 1.038e-06 (big_v), so the tolerance is 4.151e-06; the device's
largest error on these cases is 2.466e-07, printed by every test that compares them.  Scores keep the tolerance the existing beam
tests form the same way over these cases (1.353e-05; the device's largest error 1.024e-06)."""
import ctypes as C

import numpy as np
import pytest
import torch

import rnnt_beam_detail_cases as DC
import rnnt_beam_reference as RB
from nntoolkitcore_amd import capi, layers as NL
from rnnt_beam_cases import ml as _ml
from rnnt_beam_device import assert_equals_reference, decoder as _decoder, host as _host, same as _same, to_device as _t

pytestmark = pytest.mark.gpu


def _lm(name):
    t = DC.lm_table(name)
    return NL.NgramLm.from_arrays(alpha=t[1], beta=t[2], **t[0]) if t else None


def _decode(gpu, dec, c, lm=None, detail=True, length_norm=False, enc=None, n=None, nbest=None):
    return _host(dec.beam_decode(_t(gpu, c["enc"] if enc is None else enc), c["n"] if n is None else n, c["W"], nbest or c["nbest"], _ml(c),
                                 lm=lm, detail=detail, length_norm=length_norm))


def _entries(got, b):
    """row b's reported hypotheses as (labels, score bits, frames, log-probability bits)"""
    labels, lengths, scores, frames, logps = got
    return [(tuple(labels[b, k, :lengths[b, k]].tolist()), int(scores[b, k].view(np.int32)), tuple(frames[b, k, :lengths[b, k]].tolist()),
             tuple(logps[b, k, :lengths[b, k]].view(np.int32).tolist())) for k in range(labels.shape[1]) if lengths[b, k] >= 0]


def _log_softmax(x):
    x = x - x.max()
    return x - np.log(np.exp(x).sum())


def _assert_structure(name, c, got, n=None, t0=None):
    """independent of the reference: padding, order, range and multiplicity of the frames, the sign of the confidences"""
    labels, lengths, scores, frames, logps = got
    n = c["n"] if n is None else n
    for b in range(labels.shape[0]):
        lo = 0 if t0 is None else t0[b]
        for k in range(labels.shape[1]):
            L = max(int(lengths[b, k]), 0)
            fr, lp = frames[b, k], logps[b, k]
            assert (fr[L:] == -1).all() and (lp[L:] == 0.0).all() and (lp[L:].view(np.int32) == 0).all(), (name, b, k)
            assert (labels[b, k, L:] == -1).all()
            assert (np.diff(fr[:L]) >= 0).all() and (fr[:L] >= lo).all() and (fr[:L] < lo + n[b]).all(), (name, b, k, fr[:L], n[b])
            assert all((fr[:L] == t).sum() <= c["ms"] for t in fr[:L]), (name, b, k, fr[:L])
            assert float(lp[:L].astype(np.float64).sum()) <= 0.0
        if n[b] == 0 and t0 is None:                 # the row without frames: the empty hypothesis, nothing else
            assert lengths[b, 0] == 0 and (lengths[b, 1:] == -1).all() and (frames[b] == -1).all() and (logps[b] == 0.0).all(), (name, b)


def _assert_confidences(name, c, got):
    """label_logps against the float64 lattice of the hypothesis's own labels, at its own frames -> the largest error"""
    labels, lengths, scores, frames, logps = got
    m = c["m"]
    worst = 0.0
    for b in range(labels.shape[0]):
        for k in range(labels.shape[1]):
            L = int(lengths[b, k])
            if L <= 0:
                continue
            y = labels[b, k, :L].tolist()
            lat = RB.lattice_logits(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"][b], y, blank=m["blank"], activation=c["act"])
            for j in range(L):
                want = _log_softmax(lat[frames[b, k, j], j])[y[j]]
                worst = max(worst, abs(float(logps[b, k, j]) - want))
    print("%s: largest device error of a label's log-probability %.3e (tolerance %.3e)" % (name, worst, DC.lps_tol()))
    assert worst <= DC.lps_tol(), (name, worst, DC.lps_tol())
    return worst


@pytest.mark.parametrize("group", [0, 1])
@pytest.mark.parametrize("name", DC.ALL_CASES)
def test_equals_the_reference_and_moves_nothing(gpu, name, group):
    """assertions 1 to 4 and 7 on every case, with the automatic group (four where it fits) and one by one"""
    r64 = DC.assert_premise(name)
    c = DC.case(name)
    L = capi.load()
    dec, lm = _decoder(gpu, c), _lm(name)
    try:
        L.nntk_shim_rnnt_beam_set_group(group)
        if group == 0 and c["W"] > 1:
            assert L.nntk_shim_rnnt_beam_group(c["W"], c["m"]["H"], c["m"]["J"], c["m"]["V"]) == 4
        plain = _decode(gpu, dec, c, lm, detail=False)                               # the call that existed before
        got = _decode(gpu, dec, c, lm, length_norm=DC.length_norm(name))
        off = _decode(gpu, dec, c, lm, length_norm=False)
        whole = [_decode(gpu, dec, c, lm, length_norm=ln, nbest=c["W"]) for ln in (False, True)] if DC.length_norm(name) else None
    finally:
        L.nntk_shim_rnnt_beam_set_group(0)
        dec.destroy()
        if lm:
            lm.close()
    assert _same(off[:3], plain), name                                               # 1: detail on moves no bit
    _assert_structure(name, c, got)
    _assert_structure(name, c, off)
    assert_equals_reference(name, got, r64, c["nbest"], DC.score_tol)
    _assert_confidences(name, c, got)
    if DC.length_norm(name):                                                         # 7: the same final A, the plain call's bits
        assert any(_entries(got, b) != _entries(off, b) for b in range(got[0].shape[0])), (name, "nothing was reordered")
        for b in range(got[0].shape[0]):
            plain_all, norm_all = _entries(whole[0], b), _entries(whole[1], b)
            assert sorted(plain_all) == sorted(norm_all), (name, b)                  # nbest = W: the whole report, in another order
            assert _entries(got, b) == norm_all[:c["nbest"]], (name, b)
            assert len(norm_all) == len(r64["final"][b]), (name, b)                  # with a model: the -inf entries are still dropped


def test_null_options_and_an_all_off_struct_are_the_existing_calls(gpu):
    L = capi.load()
    for name in ("awkward", "lm_stream"):
        c = DC.case(name)
        dec, lm = _decoder(gpu, c), _lm(name)
        B, T, J = c["enc"].shape
        W, NB, ML = c["W"], c["nbest"], _ml(c)
        enc = _t(gpu, c["enc"])
        n = np.asarray(c["n"], np.int32)
        plain = _decode(gpu, dec, c, lm, detail=False)
        opts = [C.byref(capi.NntkRnntBeamOptions(lm.h if lm else None, 0, None, None))] + ([None] if lm is None else [])
        for o in opts:
            outs = dec._beam_outputs(gpu, B, NB, ML)
            ws = dec._beam_workspace(gpu, B, W, ML, lm)
            need = L.nntk_rnnt_beam_opt_workspace_floats(dec.h, B, W, ML, o)
            assert need == (L.nntk_rnnt_beam_lm_workspace_floats if lm else L.nntk_rnnt_beam_workspace_floats)(dec.h, B, W, ML)
            rc = L.nntk_rnnt_beam_decode_opt_device(dec.h, None, enc.data_ptr(), B, T, n.ctypes.data_as(capi.ip), W, NB, ML, o,
                                                    outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), ws.data_ptr())
            assert rc == 0, capi.last_error()
            assert _same(_host(outs), plain), name
        dec.destroy()
        if lm:
            lm.close()


def test_an_unpruned_path_does_not_exceed_the_mass(gpu):
    """sum(lps) + the blanks along the frames is one alignment's log-probability: at most the hypothesis's score, which is their sum"""
    c = DC.case("exhaustive")
    m = c["m"]
    dec = _decoder(gpu, c)
    labels, lengths, scores, frames, logps = _decode(gpu, dec, c)
    dec.destroy()
    for b, n in enumerate(c["n"]):
        for k in range(c["nbest"]):
            L = int(lengths[b, k])
            if L < 0:
                continue
            y, fr = labels[b, k, :L].tolist(), frames[b, k, :L]
            lat = RB.lattice_logits(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"][b], y, blank=m["blank"], activation=c["act"])
            blanks = sum(_log_softmax(lat[t, int((fr <= t).sum())])[m["blank"]] for t in range(n))
            path = float(logps[b, k, :L].astype(np.float64).sum()) + blanks
            assert path <= float(scores[b, k]) + DC.score_tol(), (b, k, path, scores[b, k])


@pytest.mark.parametrize("name", DC.STREAM_CASES)
def test_streaming_equals_the_one_shot_call_after_every_push(gpu, name):
    c = DC.case(name)
    B, T, J = c["enc"].shape
    dec, lm = _decoder(gpu, c), _lm(name)
    ln = DC.length_norm(name)
    singles = [[1, 1, 1 if i < 7 else 0] for i in range(12)]
    ragged = [[5, 3, 0], [0, 0, 0], [7, 9, 7]]                                       # with a push of zero frames
    for splits in (singles, ragged):
        s = NL.RnntBeamStream(dec, B, c["W"], c["nbest"], _ml(c), lm=lm, detail=True, length_norm=ln)
        seen = [0] * B
        for split in splits:
            chunk = np.full((B, max(max(split), 1), J), np.nan, np.float32)
            for b in range(B):
                chunk[b, :split[b]] = c["enc"][b, seen[b]:seen[b] + split[b]]
                seen[b] += split[b]
            got = _host(s.push(_t(gpu, chunk), split))
            assert _same(got, _decode(gpu, dec, c, lm, length_norm=ln, n=seen)), (splits, seen)
        assert seen == c["n"]
        one = _decode(gpu, dec, c, lm, length_norm=ln)
        s.reset([1])                                                                 # row 1 counts its frames from 0 again
        chunk = np.full((B, 12, J), np.nan, np.float32)
        chunk[1] = c["enc"][1]
        assert _same(_host(s.push(_t(gpu, chunk), [0, 12, 0])), one)
        s.reset()
        assert _same(_host(s.push(_t(gpu, c["enc"]), c["n"])), one)
        s.close()
    dec.destroy()
    if lm:
        lm.close()


def test_two_calls_position_neighbours_padding_and_nan_change_no_bit(gpu):
    c = DC.case("awkward")
    dec = _decoder(gpu, c)
    base = _decode(gpu, dec, c)
    assert _same(base, _decode(gpu, dec, c))
    enc = c["enc"].copy()
    for b, n in enumerate(c["n"]):
        enc[b, n:] = np.nan
    dirty = _decode(gpu, dec, c, enc=enc)
    assert _same(base, dirty) and not np.isnan(dirty[4]).any()
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


def test_host_form_equals_the_device_form(gpu):
    for name in ("awkward", "lm_norm"):
        c = DC.case(name)
        m = c["m"]
        dec, lm = _decoder(gpu, c), _lm(name)
        dev = _decode(gpu, dec, c, lm, length_norm=DC.length_norm(name))
        dec.destroy()
        got = NL.rnnt_beam_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], c["n"], beam_width=c["W"], nbest=c["nbest"],
                                  max_labels=_ml(c), blank=m["blank"], joint_activation=c["act"], max_symbols_per_frame=c["ms"], lm=lm,
                                  detail=True, length_norm=DC.length_norm(name))
        if lm:
            lm.close()
        assert _same(got, dev), name


def test_sizes_and_refusals_write_nothing(gpu):
    """the size functions, then every refusal the options add: -1 / NULL, a message, the five outputs and the workspace untouched"""
    L = capi.load()
    c = DC.case("stream")
    dec = _decoder(gpu, c)
    other = _lm("lm_wide_identity")                 # V 70: no model for the stream case's 6 classes
    B, T, J = c["enc"].shape
    W, NB, ML = c["W"], c["nbest"], _ml(c)
    plain_b, lm_b = L.nntk_rnnt_beam_state_bytes(dec.h, B, W, ML), L.nntk_rnnt_beam_state_bytes_lm(dec.h, B, W, ML)
    assert L.nntk_rnnt_beam_state_bytes_opt(dec.h, B, W, ML, 0, 0) == plain_b and L.nntk_rnnt_beam_state_bytes_opt(dec.h, B, W, ML, 1, 0) == lm_b
    assert L.nntk_rnnt_beam_state_bytes_opt(dec.h, B, W, ML, 0, 1) == plain_b + B * W * ML * 8
    assert L.nntk_rnnt_beam_state_bytes_opt(dec.h, B, W, ML, 1, 1) == lm_b + B * W * ML * 8
    assert L.nntk_rnnt_beam_state_bytes_opt(dec.h, 0, W, ML, 0, 1) == 0
    enc = _t(gpu, c["enc"])
    buf = torch.full((3 * B * NB * ML + 2 * B * NB + 8,), 7, dtype=torch.int32, device=gpu)
    nl, nh = B * NB * ML, B * NB
    lab, ln, fr = buf[:nl], buf[nl:nl + nh], buf[nl + nh:2 * nl + nh]
    fbuf = torch.full((nl + nh + 8,), 7.0, device=gpu)
    sc, lp = fbuf[:nh], fbuf[nh:nh + nl]
    full = capi.NntkRnntBeamOptions(None, 0, fr.data_ptr(), lp.data_ptr())
    need = L.nntk_rnnt_beam_opt_workspace_floats(dec.h, B, W, ML, C.byref(full))
    assert need > L.nntk_rnnt_beam_workspace_floats(dec.h, B, W, ML)
    ws = torch.full((need + 8,), 7.0, device=gpu)
    st_plain = NL.RnntBeamStream(dec, B, W, NB, ML)
    st_detail = NL.RnntBeamStream(dec, B, W, NB, ML, detail=True)
    st_detail.push(enc[:, :5].contiguous(), [5, 5, 5])
    n = np.asarray(c["n"], np.int32)

    def call(state=None, length_norm=0, frames=fr.data_ptr(), logps=lp.data_ptr(), model=None, scores=sc.data_ptr()):
        o = capi.NntkRnntBeamOptions(model, length_norm, frames, logps)
        return L.nntk_rnnt_beam_decode_opt_device(dec.h, state, enc.data_ptr(), B, T, n.ctypes.data_as(capi.ip), W, NB, ML, C.byref(o),
                                                  lab.data_ptr(), ln.data_ptr(), scores, ws.data_ptr())

    bad = [("length_norm 2", dict(length_norm=2), "length_norm"), ("length_norm -1", dict(length_norm=-1), "length_norm"),
           ("misaligned label_frames", dict(frames=fr.data_ptr() + 2), "aligned"),
           ("misaligned label_logps", dict(logps=lp.data_ptr() + 1), "aligned"),
           ("label_frames overlap labels", dict(frames=lab.data_ptr() + 8), "overlaps"),
           ("label_logps overlap label_frames", dict(logps=fr.data_ptr() + 4), "overlaps"),
           ("label_logps overlap scores", dict(logps=sc.data_ptr()), "overlaps"),
           ("label_frames overlap enc", dict(frames=enc.data_ptr()), "overlaps"),
           ("label_logps overlap the workspace's end", dict(logps=ws.data_ptr() + 4 * (need - 1)), "overlaps"),
           ("a state without detail in a call with detail", dict(state=st_plain.h), "without detail"),
           ("a state with detail in a call without", dict(state=st_detail.h, frames=None, logps=None), "with detail"),
           ("what the existing calls refuse: NULL scores", dict(scores=None), "NULL"),
           ("a model for another vocabulary", dict(model=other.h), "language model")]
    for name, change, word in bad:
        rc = call(**change)
        torch.cuda.synchronize()
        assert rc == -1 and word in capi.last_error(), (name, capi.last_error())
        assert (buf == 7).all() and (fbuf == 7.0).all() and (ws == 7.0).all(), name
    # a state created with detail is refused by the calls that existed before
    args = (dec.h, st_detail.h, enc.data_ptr(), B, T, n.ctypes.data_as(capi.ip), W, NB, ML)
    assert L.nntk_rnnt_beam_decode_device(*args, lab.data_ptr(), ln.data_ptr(), sc.data_ptr(), ws.data_ptr()) == -1
    assert "with detail" in capi.last_error()
    torch.cuda.synchronize()
    assert (buf == 7).all() and (fbuf == 7.0).all() and (ws == 7.0).all()
    # ... and the state is where its first push left it
    one = _decode(gpu, dec, c)
    assert _same(_host(st_detail.push(enc[:, 5:].contiguous(), [7, 7, 2])), one)
    assert call() == 0
    torch.cuda.synchronize()
    assert _same((lab.cpu().numpy().reshape(B, NB, ML), ln.cpu().numpy().reshape(B, NB), sc.cpu().numpy().reshape(B, NB),
                  fr.cpu().numpy().reshape(B, NB, ML), lp.cpu().numpy().reshape(B, NB, ML)), one)
    st_plain.close(); st_detail.close(); dec.destroy(); other.close()
