"""The options of the token-and-duration beam search on the device (csrc/hip/rnnt_tdt_beam.hip, the LM and DETAIL instantiations)
against tests/rnnt_tdt_beam_opt_reference.py.  Labels, lengths, frames and durations are compared for EQUALITY with the float64
reference on the cases whose premises tests/test_rnnt_tdt_beam_opt_host.py checks on the CPU; scores and logps within its score_tol(),
4 x the largest float32-restatement error, computed there.  Measured: largest float32 error 1.354e-06, so the tolerance is 5.417e-06;
the device's largest error is 5.531e-07 on the cases (awkward, lm and length_norm on) and 6.904e-07 against tdt_path_mass plus the
model's score in the exhaustive case.  Every comparison prints its measured error next to the tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import rnnt_beam_lm_cases as LC
import test_rnnt_tdt_beam_host as H
from nntoolkitcore_amd import capi, layers as NL
from rnnt_beam_device import host as _host, same as _same, to_device as _t
from test_gpu_rnnt_tdt_beam import _decoder
from test_rnnt_tdt_beam_opt_host import ALPHA, BETA, MODES, VARIANT, case as _case, reference as _reference, score_tol, table as _table

pytestmark = pytest.mark.gpu
_p = lambda t: C.c_void_p(t if isinstance(t, int) else t.data_ptr())


def _lm(t, alpha=ALPHA, beta=BETA):
    return NL.NgramLm.from_arrays(alpha=alpha, beta=beta, **t)


def _decode(gpu, dec, c, **kw):
    enc, W, nbest = kw.pop("enc", c["enc"]), kw.pop("W", c["W"]), kw.pop("nbest", c["nbest"])
    return _host(dec.tdt_beam_decode(_t(gpu, enc), c["n"], W, nbest, c["max_labels"], **kw))


@pytest.mark.parametrize("detail", (False, True))
@pytest.mark.parametrize("lm,length_norm", MODES)
@pytest.mark.parametrize("name", list(VARIANT))
def test_equals_the_float64_reference(gpu, name, lm, length_norm, detail):
    c, r64 = _case(name), _reference(name, lm, length_norm)[0]
    dec, model = _decoder(gpu, c), _lm(_table(name)) if lm else None
    got = _decode(gpu, dec, c, lm=model, detail=detail, length_norm=length_norm)
    dec.destroy()
    worst = 0.0
    for b, k in np.ndindex(got[0].shape[:2]):
        have = k < len(r64["labels"][b])
        y = r64["labels"][b][k] if have else []
        want = [y, r64["frames"][b][k], r64["durs"][b][k]] if have else [[], [], []]
        assert got[1][b, k] == (len(y) if have else -1) and (have or got[2][b, k] == -np.inf), (name, b, k)
        for g, w in zip((got[0], *got[3:5]), want):                                  # labels (frames, durations), then -1
            assert g[b, k].tolist() == w + [-1] * (c["max_labels"] - len(y)), (name, b, k, g[b, k], w)
        if have:
            worst = max(worst, abs(float(got[2][b, k]) - float(r64["scores"][b][k])))
        if detail:
            assert (got[5][b, k, len(y):] == 0.0).all()
            worst = max([worst] + [abs(float(x) - float(z)) for x, z in zip(got[5][b, k], r64["lps"][b][k] if have else [])])
    print("%s lm %d norm %d detail %d: largest device error, scores and logps %.3e (tolerance %.3e)" % (name, lm, length_norm, detail, worst,
                                                                                                        score_tol()))
    assert worst <= score_tol()
    assert got[1][2, 0] == 0 and (got[1][2, 1:] == -1).all()                         # the row without frames: ln E(start_state)
    assert got[2][2, 0] == np.float32(r64["scores"][2][0]) and (lm or got[2][2, 0] == 0.0)


def test_everything_off_is_the_plain_call_and_detail_changes_no_bit(gpu):
    L = capi.load()
    c = _case("awkward")
    dec, model = _decoder(gpu, c), _lm(_table("awkward"))
    unit = _lm(dict(_table("awkward"), final_logp=None), 0.0, 0.0)
    plain = _decode(gpu, dec, c)
    B, T, _ = c["enc"].shape
    need = L.nntk_rnnt_tdt_beam_workspace_floats(dec.h, B, c["W"], c["max_labels"])
    for o in (None, C.byref(capi.NntkRnntTdtBeamOptions(None, 0, None, None, None))):        # o == NULL, everything off: raw calls
        assert L.nntk_rnnt_tdt_beam_opt_workspace_floats(dec.h, B, c["W"], c["max_labels"], o) == need
        outs, ws = dec._beam_outputs(gpu, B, c["nbest"], c["max_labels"]), torch.empty(need, device=gpu)
        assert L.nntk_rnnt_tdt_beam_decode_opt_device(dec.h, _p(_t(gpu, c["enc"])), B, T, np.asarray(c["n"], np.int32).ctypes.data_as(capi.ip),
                                                      c["W"], c["nbest"], c["max_labels"], o, *(_p(x) for x in outs), _p(ws)) == 0
        assert _same(_host(outs), plain)
    assert _same(_decode(gpu, dec, c, lm=unit), plain)
    for kw in (dict(), dict(lm=model), dict(lm=model, length_norm=True)):
        assert _same(_decode(gpu, dec, c, detail=True, **kw)[:3], _decode(gpu, dec, c, **kw) if kw else plain), kw
    dec.destroy()


def test_groups_calls_and_nan_frames_change_no_bit(gpu):
    L = capi.load()
    c = _case("awkward")
    dec, model = _decoder(gpu, c), _lm(_table("awkward"))
    try:
        for W in (3, 8):
            runs = []
            for pin in (0, 1, 1):                                                    # the group of four, one by one, and once more
                L.nntk_shim_rnnt_tdt_beam_set_group(pin)
                runs.append(_decode(gpu, dec, c, W=W, nbest=3, lm=model, detail=True, length_norm=True))
            assert len(runs[0]) == 6 and _same(runs[0], runs[1]) and _same(runs[1], runs[2]), W
    finally:
        L.nntk_shim_rnnt_tdt_beam_set_group(0)
        dec.destroy()
    c = H.case("skip")                                                               # durations (0, 2, 4): odd frames are never landed on
    t, alpha, beta = LC.table("stream")                                              # V 6, blank 2, as the case
    dec, model, enc = _decoder(gpu, c), _lm(t, alpha, beta), c["enc"].copy()
    for b, n in enumerate(c["n"]):
        enc[b, list(range(n, enc.shape[1])) + list(range(1, n, 2))] = np.nan
    clean, dirty = (_decode(gpu, dec, c, enc=e, lm=model, detail=True) for e in (c["enc"], enc))
    dec.destroy()
    assert _same(clean, dirty) and not np.isnan(dirty[2]).any() and (dirty[3][dirty[3] >= 0] % 2 == 0).all()


def test_fused_score_minus_the_model_is_the_path_mass(gpu):
    c = H.exhaustive_case((0, 1, 2, 4), 1)                                           # V 3, blank 1: nothing is pruned
    t, alpha, beta = LC.table("exhaustive3")
    model = _lm(t, alpha, beta)
    labels, lengths, scores = _decode(gpu, _decoder(gpu, c), c, lm=model)
    worst = 0.0
    for b, k in np.ndindex(3, 7):
        y = labels[b, k, :lengths[b, k]].tolist()
        worst = max(worst, abs(float(scores[b, k]) - model.score(y, with_final=True) - H.path_mass(c, b, tuple(y))))
    print("largest |score - lm - path mass| %.3e (tolerance %.3e)" % (worst, score_tol()))
    assert worst <= score_tol() and (lengths[:, 7] == -1).all()


def test_host_pointer_form_gives_the_device_forms_bits(gpu):
    c = _case("awkward_w3")
    m, kw = c["m"], dict(lm=_lm(_table("awkward_w3")), detail=True, length_norm=True)
    dec = _decoder(gpu, c)
    assert _same(_decode(gpu, dec, c, **kw), NL.rnnt_tdt_beam_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], m["durs"], c["n"], c["W"],
                                                                      c["nbest"], c["max_labels"], m["blank"], c["act"], c["ms"], **kw))
    dec.destroy()


def test_refusals_write_nothing(gpu):
    L = capi.load()
    c = _case("awkward_w3")
    m, (B, T, _), W, NB, ML = c["m"], c["enc"].shape, c["W"], c["nbest"], c["max_labels"]
    tdt, lm = _decoder(gpu, c), _lm(_table("awkward_w3"))
    classic = NL.RnntDecoder(_t(gpu, m["embed"]), _t(gpu, m["lstm"]), _t(gpu, m["proj"]), _t(gpu, m["out"][:23 * 5]), blank=0)
    other = _lm(LC.table("stream")[0])                                               # built for V 6, blank 2
    nl, enc = B * NB * ML, _t(gpu, c["enc"])
    buf = torch.full((4 * nl + 2 * B * NB + 8,), 7, dtype=torch.int32, device=gpu)
    lab, fr, du, lp, ln = [buf[i * nl:(i + 1) * nl] for i in range(4)] + [buf[4 * nl:4 * nl + B * NB]]
    sc = torch.full((B * NB,), 7.0, device=gpu)
    o = lambda **kw: capi.NntkRnntTdtBeamOptions(*(kw.get(k, d) for k, d in (("lm", lm.h), ("norm", 1), ("fr", fr.data_ptr()), ("du", du.data_ptr()),
                                                                               ("lp", lp.data_ptr()))))
    ws = torch.full((L.nntk_rnnt_tdt_beam_opt_workspace_floats(tdt.h, B, W, ML, C.byref(o())) + 8,), 7.0, device=gpu)
    bad = [(tdt, o(lm=other.h), "language model"), (tdt, o(norm=2), "length_norm"), (tdt, o(du=du.data_ptr() + 2), "4-byte"),
           (tdt, o(fr=lab.data_ptr()), "overlaps"), (tdt, o(lp=du.data_ptr() + 8), "overlaps"), (tdt, o(du=enc.data_ptr()), "overlaps"),
           (tdt, o(lp=ws.data_ptr() + 64), "overlaps"), (classic, o(lm=None), "nntk_rnnt_beam_decode_device")]
    for dec, opt, word in bad:
        rc = L.nntk_rnnt_tdt_beam_decode_opt_device(dec.h, _p(enc), B, T, np.asarray(c["n"], np.int32).ctypes.data_as(capi.ip), W, NB, ML,
                                                    C.byref(opt), _p(lab), _p(ln), _p(sc), _p(ws))
        torch.cuda.synchronize()
        assert rc == -1 and word in capi.last_error() and (buf == 7).all() and (sc == 7.0).all() and (ws == 7.0).all(), (word, capi.last_error())
    tdt.destroy(); classic.destroy()
