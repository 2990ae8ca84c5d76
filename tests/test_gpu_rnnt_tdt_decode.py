"""Token-and-duration greedy decoding on the device (csrc/hip/rnnt_tdt_decode.hip) against tests/rnnt_tdt_decode_reference.py.

Labels, frames, durations and lengths are compared for EQUALITY with the float64 reference, so every gap case uses inputs on which the
reference itself is unambiguous: its smallest best-minus-second gap over both heads' decisions is asserted to be at least GAP = 1e-3
(orders above the f32 rounding of O(1) scores at J <= 33), its float32 restatement must decode identically, and the case must hold the
moves it is there for (_assert_premise; the seeds were chosen on the CPU for that).  The tie case is the exception by construction.

Score tolerance, from the CPU alone: 4 x the largest |float32 restatement - float64| score over the cases of this file (_score_tol; 4
because the device's summation order differs), printed with the device's own error by every test that compares scores."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import rnnt_tdt_decode_reference as R
import rnnt_tdt_reference as LOSS
from nntoolkitcore_amd import capi, layers as NL

pytestmark = pytest.mark.gpu

GAP = 1e-3
GROUP, GROUP_BATCH = 4, 512                         # NNTK_RNNT_DEC_GROUP rows share a workgroup above NNTK_RNNT_DEC_GROUP_BATCH rows
KEYS = ("labels", "frames", "durations")


def _model(seed, V, E, H, J, proj, durs, blank=0, label_bias=0.0, dur_bias=None):
    rng = np.random.default_rng(seed)
    u = lambda sc, *s: rng.uniform(-sc, sc, s).astype(np.float32)
    G, D = 4 * H, len(durs)
    bias = u(0.1, V + D)
    bias[:V][np.arange(V) != blank] += np.float32(label_bias)
    bias[V:] += np.float32(dur_bias if dur_bias is not None else 0.0)
    return dict(V=V, E=E, H=H, J=J, blank=blank, durs=durs, embed=u(1.0, V, E),
                lstm=np.concatenate([u(2.0 * E ** -0.5, E * G), u(2.0 * H ** -0.5, H * G), u(0.1, G), u(0.1, G)]),
                proj=np.concatenate([u(2.0 * H ** -0.5, H * J), u(0.1, J)]) if proj else None,
                out=np.concatenate([u(3.0 * J ** -0.5, J * (V + D)), bias]), rng=rng)


# seeds chosen on the CPU so that _assert_premise holds; nothing about them comes from a device
SEEDS = {"awkward": 9, "wide": 0, "straddle": 12, "lattice": 56}
# what each case must hold, as counts of the reference
NEEDS = {"awkward": ("long_blank", "label_zero", "label_pos", "capped", "overshoot", "blank_zero"), "truncated": ("label_zero",),
         "wide": ("label_pos", "skipped"), "straddle": ("label_zero", "label_pos", "skipped"), "lattice": ("ends_exact", "skipped")}


def _case(name):
    """dict(m = the model, enc, n, act, ms = max_symbols_per_frame, max_labels)"""
    if name in ("awkward", "truncated"):            # batch 3, T 11, tanh, with the projection, cap 2
        m = _model(SEEDS["awkward"], 5, 7, 12, 20, True, (0, 1, 2, 3), label_bias=-0.5, dur_bias=[0.3, 0.0, 0.0, 0.0])
        return dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, (3, 11, 20)).astype(np.float32), n=[11, 5, 0], act="tanh", ms=2,
                    max_labels=3 if name == "truncated" else None)
    if name == "wide":                              # the duration columns 70 .. 72 sit in the lanes' second wavefront; no projection
        m = _model(SEEDS["wide"], 70, 5, 33, 33, False, (1, 2, 4), blank=69, label_bias=-2.5)
        return dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, (2, 9, 33)).astype(np.float32), n=[9, 6], act="relu", ms=3, max_labels=None)
    if name == "straddle":                          # columns 1022 .. 1025 cross the RD_THREADS boundary
        m = _model(SEEDS["straddle"], 1022, 5, 8, 8, False, (0, 1, 2, 4), blank=0, label_bias=-5.0)
        return dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, (2, 9, 8)).astype(np.float32), n=[9, 6], act="tanh", ms=3, max_labels=None)
    if name == "lattice":                           # the cap out of reach: every move is a move of the loss's lattice
        m = _model(SEEDS["lattice"], 5, 7, 12, 20, True, (0, 1, 2, 3), label_bias=-1.0)
        return dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, (3, 9, 20)).astype(np.float32), n=[9, 4, 1], act="tanh", ms=9, max_labels=None)
    if name == "tie":                               # W_out = 0: the scores are the bias; ties in both heads, the blank's among the positive
        m = _model(5, 5, 7, 12, 20, True, (0, 1, 2, 3), blank=3)
        m["out"][:20 * 9] = 0.0
        m["out"][20 * 9:] = np.float32([-0.5, 0.375, -0.75, 0.375, -1.5, 0.25, -1.0, 0.25, 0.25])
        return dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, (2, 6, 20)).astype(np.float32), n=[6, 3], act="tanh", ms=2, max_labels=None)
    raise KeyError(name)


GAP_CASES = ("awkward", "truncated", "wide", "straddle", "lattice")


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = _case(name)
    m = c["m"]
    kw = dict(n_frames=c["n"], blank=m["blank"], activation=c["act"], max_symbols_per_frame=c["ms"], max_labels=c["max_labels"])
    return tuple(R.greedy_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], m["durs"], dtype=dt, **kw)
                 for dt in (np.float64, np.float32))


@functools.lru_cache(maxsize=None)
def _score_tol():
    err = max(float(np.abs(_reference(nm)[1]["scores"].astype(np.float64) - _reference(nm)[0]["scores"]).max()) for nm in GAP_CASES + ("tie",))
    print("largest float32-restatement score error over the cases: %.3e -> tolerance %.3e" % (err, 4 * err))
    assert err > 0
    return 4 * err


def _assert_premise(name):
    r64, r32 = _reference(name)
    c = _case(name)
    live = [b for b, n in enumerate(c["n"]) if n > 0]
    print("%s: smallest gap %.3e; labels %s durations %s cells %s" % (name, min(r64["gaps"][b] for b in live), r64["labels"],
                                                                      r64["durations"], r64["cells"]))
    assert min(r64["gaps"][b] for b in live) >= GAP, (name, r64["gaps"])
    assert all(r32[k] == r64[k] for k in KEYS + ("cells",)), name
    durs = [d for row in r64["durations"] for d in row]
    jumps = [t1 - t0 for cells in r64["cells"] for (t0, u0), (t1, u1) in zip(cells, cells[1:]) if u1 == u0]      # blanks but each row's last
    have = dict(long_blank=any(j > 1 for j in jumps), label_pos=any(d > 0 for d in durs), ends_exact=r64["ends_exact"].any(),
                **{k: r64[k].sum() > 0 for k in ("label_zero", "capped", "overshoot", "blank_zero", "skipped")})
    assert all(have[k] for k in NEEDS[name]), (name, have)


def _t(gpu, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _decoder(gpu, c):
    m = c["m"]
    return NL.RnntDecoder(_t(gpu, m["embed"]), _t(gpu, m["lstm"]), _t(gpu, m["proj"]), _t(gpu, m["out"]), blank=m["blank"],
                          joint_activation=c["act"], max_symbols_per_frame=c["ms"], durations=m["durs"])


def _host(outs):
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in outs)


def _decode(gpu, dec, enc, n, max_labels=None):
    return _host(dec.decode(_t(gpu, enc), n, max_labels))


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _assert_equals_reference(name, got, r64):
    lengths, scores = got[3], got[4]
    for b in range(len(lengths)):
        k = len(r64["labels"][b])
        assert lengths[b] == k, (name, b, lengths[b], k)
        for out, key in zip(got[:3], KEYS):
            assert out[b, :k].tolist() == r64[key][b] and (out[b, k:] == -1).all(), (name, key, b, out[b], r64[key][b])
    err = np.abs(scores.astype(np.float64) - r64["scores"]).max()
    print("%s: largest device score error %.3e (tolerance %.3e); scores %s" % (name, err, _score_tol(), r64["scores"]))
    assert err <= _score_tol(), (name, err, _score_tol())


@pytest.mark.parametrize("name", GAP_CASES)
def test_equals_the_reference(gpu, name):
    _assert_premise(name)
    c = _case(name)
    dec = _decoder(gpu, c)
    got = _decode(gpu, dec, c["enc"], c["n"], c["max_labels"])
    dec.destroy()
    _assert_equals_reference(name, got, _reference(name)[0])
    if name == "awkward":
        assert got[3][2] == 0 and got[4][2] == 0.0 and (got[0][2] == -1).all()        # the row without frames
    if name == "truncated":
        full = _reference("awkward")[0]
        assert len(full["labels"][0]) > 3 and got[0].shape == (3, 3) and got[0][0].tolist() == full["labels"][0][:3]


def test_exact_ties_go_to_the_lowest_index_in_both_heads(gpu):
    c = _case("tie")
    r64 = _reference("tie")[0]
    assert all(g == 0.0 for g in r64["gaps"])
    # tokens 1 and 3 (the blank) tie: label 1; durations 0, 2 and 3 tie: 0, so the cap moves on; nothing but labels
    assert r64["labels"] == [[1] * 12, [1] * 6] and r64["durations"] == [[0] * 12, [0] * 6] and r64["capped"].tolist() == [6, 3]
    dec = _decoder(gpu, c)
    _assert_equals_reference("tie", _decode(gpu, dec, c["enc"], c["n"]), r64)
    # the blank ahead of the label: it cannot take duration 0 (the first of the tie); durations 2 and 3 tie among the positive: 2
    m = dict(c["m"], blank=1)
    rb = R.greedy_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], m["durs"], n_frames=c["n"], blank=1, max_symbols_per_frame=2)
    assert rb["labels"] == [[], []] and rb["cells"] == [[(0, 0), (2, 0), (4, 0)], [(0, 0), (2, 0)]] and rb["blank_zero"].tolist() == [3, 2]
    decb = _decoder(gpu, dict(c, m=m))
    got = _decode(gpu, decb, c["enc"], c["n"])
    assert got[3].tolist() == [0, 0] and np.abs(got[4] - rb["scores"]).max() <= _score_tol()
    dec.destroy(); decb.destroy()


def _push_all(gpu, dec, c, splits, max_labels, stream=None):
    """splits: per push the frames each row brings; the chunk tensor holds NaN behind a row's frames"""
    B, T, J = c["enc"].shape
    s = stream or NL.RnntGreedyStream(dec, B, max_labels)
    seen = [0] * B
    out = None
    for split in splits:
        chunk = np.full((B, max(max(split), 1), J), np.nan, np.float32)
        for b in range(B):
            chunk[b, :split[b]] = c["enc"][b, seen[b]:seen[b] + split[b]]
            seen[b] += split[b]
        out = s.push(_t(gpu, chunk), split)
    assert seen == list(c["n"])
    return s, _host(out)


def test_streaming_equals_the_one_shot_call_bit_for_bit(gpu):
    _assert_premise("awkward")                                                       # jumps of 2 and 3 frames, and one past the end
    c = _case("awkward")
    dec = _decoder(gpu, c)
    one = _decode(gpu, dec, c["enc"], c["n"], 22)
    singles = [[1, 1 if i < 5 else 0, 0] for i in range(11)]                         # a jump crosses whole pushes
    ragged = [[4, 2, 0], [0, 0, 0], [7, 3, 0]]
    for splits in (singles, ragged):
        s, got = _push_all(gpu, dec, c, splits, 22)
        assert _same(got, one), splits
        s.reset([1])                                                                 # restarts row 1, frames owed included
        chunk = np.full((3, 11, 20), np.nan, np.float32)
        chunk[1] = c["enc"][1]
        assert _same(_host(s.push(_t(gpu, chunk), [0, 5, 0])), one)
        s.reset()
        assert _same(_push_all(gpu, dec, c, ragged, 22, stream=s)[1], one)
        s.close()
    dec.destroy()


def test_rows_are_independent_of_position_neighbours_grouping_and_unread_frames(gpu):
    rpg = capi.load().nntk_shim_rnnt_tdt_dec_rows_per_group
    c = _case("awkward")
    r64 = _reference("awkward")[0]
    assert rpg(GROUP_BATCH, 12, 20, 5, 4) == 1 and rpg(GROUP_BATCH + 1, 12, 20, 5, 4) == GROUP
    dec = _decoder(gpu, c)
    base = _decode(gpu, dec, c["enc"], c["n"], 22)
    dirty = c["enc"].copy()                                                          # NaN in the padding and in every frame jumped over
    for b, n in enumerate(c["n"]):
        dirty[b, [t for t in range(11) if t >= n or t not in {cell[0] for cell in r64["cells"][b]}]] = np.nan
    assert r64["skipped"].sum() > 0 and _same(_decode(gpu, dec, dirty, c["n"], 22), base) and np.isfinite(base[4]).all()
    rng = np.random.default_rng(11)
    for B in (1, GROUP_BATCH + GROUP + 2):                                           # alone; grouped, with a ragged last group
        for b in range(3):
            T = 11 if B > 1 else max(c["n"][b], 1)                                   # alone: without the T padding as well
            enc = rng.uniform(-1.5, 1.5, (B, T, 20)).astype(np.float32)
            n = rng.integers(0, T + 1, B).astype(np.int32)
            at = (B - 1 - b) if B > 1 else 0                                         # another position, other neighbours
            enc[at, :T] = dirty[b, :T]
            n[at] = c["n"][b]
            got = _decode(gpu, dec, enc, n, 22)
            assert all(np.array_equal(g[at], ref[b]) for g, ref in zip(got, base)), (B, b)
    dec.destroy()


def test_the_greedy_path_is_a_path_of_the_loss_lattice(gpu):
    """rows that end on a blank landing exactly on n: the loss of the decoded labels on the reference-built lattice is at most -score"""
    _assert_premise("lattice")
    c = _case("lattice")
    m, r64 = c["m"], _reference("lattice")[0]
    assert r64["capped"].sum() == 0
    x = R.lattice_scores(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], 4, r64["labels"], blank=m["blank"], activation=c["act"])
    rows = [b for b in range(3) if r64["ends_exact"][b]]
    for b in rows:                                                                   # the margin in float64: other alignments carry mass
        loss64 = LOSS.tdt_row(x[b, :c["n"][b], :len(r64["labels"][b]) + 1], r64["labels"][b], m["blank"], m["durs"])[0]
        print("row %d: float64 loss %.6f, -score %.6f" % (b, loss64, -r64["scores"][b]))
        assert -r64["scores"][b] - loss64 >= 1e-2, b
    dec = _decoder(gpu, c)
    got = _decode(gpu, dec, c["enc"], c["n"])
    dec.destroy()
    _assert_equals_reference("lattice", got, r64)
    loss, _ = NL.rnnt_tdt_loss_device(_t(gpu, x.astype(np.float32)), r64["labels"], m["durs"], input_lengths=c["n"], blank=m["blank"],
                                      want_grad=False)
    torch.cuda.synchronize()
    loss = loss.cpu().numpy()
    for b in rows:
        print("row %d: device loss %.6f, device -score %.6f" % (b, loss[b], -got[4][b]))
        assert loss[b] <= -got[4][b], b


def test_host_form_equals_the_device_form(gpu):
    c = _case("awkward")
    m = c["m"]
    dec = _decoder(gpu, c)
    dev = _decode(gpu, dec, c["enc"], c["n"])
    dec.destroy()
    got = NL.rnnt_tdt_greedy_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], m["durs"], c["n"], blank=m["blank"],
                                    joint_activation=c["act"], max_symbols_per_frame=c["ms"])
    assert _same(got, dev)


def test_cross_refusals_write_nothing(gpu):
    """each kind of handle refuses the other kind's calls: -1 / NULL / 0, a message, outputs and state untouched"""
    L = capi.load()
    c = _case("awkward")
    m = c["m"]
    tdt = _decoder(gpu, c)
    classic = NL.RnntDecoder(_t(gpu, m["embed"]), _t(gpu, m["lstm"]), _t(gpu, m["proj"]), _t(gpu, m["out"][:21 * 5]), blank=0)
    enc = _t(gpu, c["enc"])
    one = _decode(gpu, tdt, c["enc"], c["n"], 22)
    st = NL.RnntGreedyStream(tdt, 3, 22)
    st.push(enc[:, :4].contiguous(), [4, 4, 0])
    buf = torch.full((4 * 3 * 22 + 16,), 7, dtype=torch.int32, device=gpu)
    lab, fr, du, ln = (C.c_void_p(buf[i * 66:].data_ptr()) for i in range(4))
    sc = torch.full((3,), 7.0, device=gpu)
    n = np.asarray(c["n"], np.int32).ctypes.data_as(capi.ip)
    pe, ps = C.c_void_p(enc.data_ptr()), C.c_void_p(sc.data_ptr())
    calls = [("tdt call, classic handle", lambda: L.nntk_rnnt_tdt_greedy_decode_device(classic.h, None, pe, 3, 11, n, 22, lab, fr, du, ln, ps), -1),
             ("classic call, tdt handle", lambda: L.nntk_rnnt_greedy_decode_device(tdt.h, None, pe, 3, 11, n, 22, lab, fr, ln, ps), -1),
             ("classic call, tdt state", lambda: L.nntk_rnnt_greedy_decode_device(tdt.h, st.h, pe, 3, 11, n, 22, lab, fr, ln, ps), -1),
             ("beam call", lambda: L.nntk_rnnt_beam_decode_device(tdt.h, None, pe, 3, 11, n, 2, 1, 22, lab, ln, ps, fr), -1),
             ("beam state", lambda: L.nntk_rnnt_beam_state_create(tdt.h, 3, 2, 22) or 0, 0),
             ("beam state, opt", lambda: L.nntk_rnnt_beam_state_create_opt(tdt.h, 3, 2, 22, None, 1) or 0, 0)]
    for name, call, want in calls:
        rc = call()
        torch.cuda.synchronize()
        assert rc == want and "durations" in capi.last_error(), (name, rc, capi.last_error())
        assert (buf == 7).all() and (sc == 7.0).all(), name
    assert L.nntk_rnnt_beam_workspace_floats(tdt.h, 3, 2, 22) == 0 and L.nntk_rnnt_beam_state_bytes(tdt.h, 3, 2, 22) == 0
    assert L.nntk_rnnt_beam_workspace_floats(classic.h, 3, 2, 22) > 0                # a classic handle is served as before
    with pytest.raises(capi.NNTKError):
        tdt.beam_decode(enc, c["n"])
    assert len(classic.decode(enc, c["n"])) == 4
    assert _same(_host(st.push(enc[:, 4:].contiguous(), [7, 1, 0])), one)            # the stream is where the first push left it
    st.close(); tdt.destroy(); classic.destroy()
