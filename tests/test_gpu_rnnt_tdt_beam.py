"""Token-and-duration beam search on the device (csrc/hip/rnnt_tdt_beam.hip) against tests/rnnt_tdt_beam_reference.py.

Labels and lengths are compared for EQUALITY with the float64 reference, on the cases whose premises tests/test_rnnt_tdt_beam_host.py
checks on the CPU (cut and order gaps of at least 1e-3, the float32 restatement returning the same labels); the tie case is the
exception by construction.  Score tolerance, from the CPU alone: 4 x the largest |float32 restatement - float64| score over the named
cases and the tie case (score_tol; 4 because the device's summation order differs).  Measured: largest float32 error 1.354e-06, so the
tolerance is 5.416e-06; the device's largest error is 5.165e-07 on the named cases (the skip case) and 6.197e-07 against
tdt_path_mass in the exhaustive cases; every test that compares scores prints both."""
import ctypes as C

import numpy as np
import pytest
import torch

from nntoolkitcore_amd import capi, layers as NL
from rnnt_beam_device import assert_equals_reference, host as _host, same as _same, to_device as _t
from test_rnnt_tdt_beam_host import CASES, EXHAUSTIVE, case as _case, exhaustive_case, path_mass, reference as _reference, score_tol

pytestmark = pytest.mark.gpu


def _decoder(gpu, c):
    m = c["m"]
    return NL.RnntDecoder(_t(gpu, m["embed"]), _t(gpu, m["lstm"]), _t(gpu, m["proj"]), _t(gpu, m["out"]), blank=m["blank"],
                          joint_activation=c["act"], max_symbols_per_frame=c["ms"], durations=m["durs"])


def _decode(gpu, dec, c, enc=None, n=None, W=None, nbest=None, once=False):
    got = _host(dec.tdt_beam_decode(_t(gpu, c["enc"] if enc is None else enc), c["n"] if n is None else n, W or c["W"], nbest or c["nbest"],
                                    c["max_labels"]))
    if once:
        dec.destroy()
    return got


@pytest.mark.parametrize("durs,blank", EXHAUSTIVE)
def test_exhaustive_search_gives_the_path_masses(gpu, durs, blank):
    """nothing pruned: the 7 sequences come back with 1 empty slot, in descending order, each with the mass of its paths"""
    c = exhaustive_case(durs, blank)
    labels, lengths, scores = _decode(gpu, _decoder(gpu, c), c, once=True)
    worst = 0.0
    for b in range(3):
        got = [tuple(labels[b, k, :lengths[b, k]].tolist()) for k in range(7)]
        assert len(set(got)) == 7 and lengths[b, 7] == -1 and scores[b, 7] == -np.inf and (labels[b, 7] == -1).all(), (b, got)
        assert all(scores[b, k] >= scores[b, k + 1] for k in range(6))
        worst = max([worst] + [abs(float(scores[b, k]) - path_mass(c, b, got[k])) for k in range(7)])
    print("largest |score - path mass| %.3e (tolerance %.3e)" % (worst, score_tol()))
    assert worst <= score_tol()


@pytest.mark.parametrize("name", list(CASES) + ["tie"])
def test_equals_the_float64_reference(gpu, name):
    """the named cases; tie: exact ties at a cut and in the final order go to the lower index, in the reference and on the device"""
    c = _case(name)
    labels, lengths, scores = got = _decode(gpu, _decoder(gpu, c), c, once=True)
    assert_equals_reference(name, got, _reference(name)[0], c["nbest"], score_tol)
    assert name != "tie" or scores[0, 0] == scores[0, 1]
    if name == "awkward_w3":                         # the host-pointer form gives the device form's bits
        m = c["m"]
        assert _same(got, NL.rnnt_tdt_beam_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], m["durs"], c["n"], c["W"], c["nbest"],
                                                  c["max_labels"], m["blank"], c["act"], c["ms"]))
    if name.startswith("awkward"):
        assert lengths[2, 0] == 0 and scores[2, 0] == 0.0 and (lengths[2, 1:] == -1).all()      # the row without frames
        assert c["m"]["E"] % 4 and c["m"]["H"] % 4 and c["m"]["J"] % 4 and c["m"]["V"] % 64


def test_group_of_four_and_one_by_one_give_the_same_bits(gpu):
    L = capi.load()
    c = _case("awkward")
    dims = (c["m"]["H"], c["m"]["J"], c["m"]["V"], 4)
    dec = _decoder(gpu, c)
    try:
        for W in (3, 5, 8):                                                          # W no multiple of the group, and one that is
            runs = []
            for pin, want in ((0, 4), (1, 1)):
                L.nntk_shim_rnnt_tdt_beam_set_group(pin)
                assert L.nntk_shim_rnnt_tdt_beam_group(W, *dims) == want
                runs.append(_decode(gpu, dec, c, W=W, nbest=min(3, W)))
            assert _same(*runs), W
    finally:
        L.nntk_shim_rnnt_tdt_beam_set_group(0)
        dec.destroy()


def test_nan_in_frames_nobody_lands_on_changes_no_bit(gpu):
    c, r64 = _case("skip"), _reference("skip")[0]
    assert r64["skipped_frames"].min() > 0
    enc = c["enc"].copy()
    for b, n in enumerate(c["n"]):
        enc[b, list(range(n, enc.shape[1])) + r64["skipped"][b]] = np.nan           # at or beyond n, and never landed on
    dec = _decoder(gpu, c)
    clean, dirty = _decode(gpu, dec, c), _decode(gpu, dec, c, enc=enc)
    dec.destroy()
    assert _same(clean, dirty) and not np.isnan(dirty[2]).any()


def test_rows_are_independent_and_two_calls_give_the_same_bits(gpu):
    c = _case("awkward")
    dec = _decoder(gpu, c)
    base = _decode(gpu, dec, c)
    assert _same(base, _decode(gpu, dec, c))
    rng = np.random.default_rng(11)
    for B, b in [(B, b) for B in (1, 4) for b in range(3)]:
        T = 10 if B > 1 else max(c["n"][b], 1)                                       # alone: without the T padding as well
        enc, n = rng.uniform(-1.5, 1.5, (B, T, 22)).astype(np.float32), rng.integers(0, T + 1, B).astype(np.int32)
        at = (B - 1 - b) if B > 1 else 0                                             # another position, other neighbours
        enc[at, :T], n[at] = c["enc"][b, :T], c["n"][b]
        got = _decode(gpu, dec, c, enc=enc, n=n)
        assert all(np.array_equal(g[at].view(np.int32), ref[b].view(np.int32)) for g, ref in zip(got, base)), (B, b)
    dec.destroy()


def test_refusals_write_nothing(gpu):
    """-1 with a message, outputs and workspace untouched; the size query is 0 on a classic handle"""
    L = capi.load()
    c = _case("awkward_w3")
    m = c["m"]
    tdt = _decoder(gpu, c)
    classic = NL.RnntDecoder(_t(gpu, m["embed"]), _t(gpu, m["lstm"]), _t(gpu, m["proj"]), _t(gpu, m["out"][:23 * 5]), blank=0)
    B, T, W, NB, ML = 3, 10, c["W"], c["nbest"], c["max_labels"]
    need = L.nntk_rnnt_tdt_beam_workspace_floats(tdt.h, B, W, ML)
    assert need > 0 and L.nntk_rnnt_tdt_beam_workspace_floats(classic.h, B, W, ML) == 0 and L.nntk_rnnt_beam_workspace_floats(tdt.h, B, W, ML) == 0
    enc = _t(gpu, c["enc"])
    buf = torch.full((B * NB * ML + 2 * B * NB + 8,), 7, dtype=torch.int32, device=gpu)
    lab, ln = buf[:B * NB * ML], buf[B * NB * ML:B * NB * ML + B * NB]
    sc, ws = torch.full((B * NB,), 7.0, device=gpu), torch.full((need + 8,), 7.0, device=gpu)
    p = lambda t: C.c_void_p(t if isinstance(t, int) else t.data_ptr())
    n = np.asarray(c["n"], np.int32).ctypes.data_as(capi.ip)
    bad = [(dict(d=classic.h), "nntk_rnnt_beam_decode_device"), (dict(W=0), "beam_width"), (dict(W=33), "beam_width"), (dict(NB=W + 1), "nbest"),
           (dict(ws=ws.data_ptr() + 4), "16-byte"), (dict(ln=lab.data_ptr() + 8), "overlaps"), (dict(sc=ws.data_ptr() + 32), "overlaps")]
    for change, word in bad:
        a = dict(dict(d=tdt.h, W=W, NB=NB, lab=lab, ln=ln, sc=sc, ws=ws), **change)
        rc = L.nntk_rnnt_tdt_beam_decode_device(a["d"], p(enc), B, T, n, a["W"], a["NB"], ML, p(a["lab"]), p(a["ln"]), p(a["sc"]), p(a["ws"]))
        torch.cuda.synchronize()
        assert rc == -1 and word in capi.last_error() and (buf == 7).all() and (sc == 7.0).all() and (ws == 7.0).all(), (change, capi.last_error())
    for dec, call in ((classic, "tdt_beam_decode"), (tdt, "beam_decode")):           # each kind of handle keeps refusing the other's call
        with pytest.raises(capi.NNTKError):
            getattr(dec, call)(enc, c["n"])
    tdt.destroy(); classic.destroy()
