"""Greedy RNN-Transducer decoding on the device (csrc/hip/rnnt_decode.hip) against tests/rnnt_decode_reference.py.

Labels, frames and lengths are compared for EQUALITY with the float64 reference, so every case uses inputs on which the reference itself
is unambiguous: its smallest gap between the best and the second-best logit over all decisions is asserted to be at least GAP = 1e-3
(orders above the f32 rounding of O(1) logits at J <= 70), its float32 restatement must decode identically, and the case must hold
blanks, labels, a frame with two or more labels and a row that ends on a label (_assert_premise).  The tie cases are the exception by
construction: exact ties, decided by the lowest index in the reference and on the device.

Score tolerance, from the CPU alone: SCORE_TOL = 4 x the largest |float32 restatement - float64| score over every case of this file
(_score_tol; 4 because the device's summation order differs).  Measured: largest float32 error 1.095e-4 (the moderate shape: some 200 decisions
a row, scores of a few hundred), so the tolerance is 4.38e-4; the device's largest error on these cases is printed by every test that compares scores.

The refusals that need a live decoder or state (they cannot exist without a device) are here as well: test_refusals_write_nothing."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import rnnt_decode_reference as R
from nntoolkitcore_amd import capi, layers as NL

pytestmark = pytest.mark.gpu

GAP = 1e-3
GROUP, GROUP_BATCH = 4, 512                         # NNTK_RNNT_DEC_GROUP rows share a workgroup above NNTK_RNNT_DEC_GROUP_BATCH rows


def _model(seed, V, E, H, J, proj, blank=0, scale=2.0, out_scale=3.0, label_bias=0.0):
    rng = np.random.default_rng(seed)
    u = lambda sc, *s: rng.uniform(-sc, sc, s).astype(np.float32)
    G = 4 * H
    bias = u(0.1, V)
    bias[np.arange(V) != blank] += np.float32(label_bias)
    return dict(V=V, E=E, H=H, J=J, blank=blank, embed=u(1.0, V, E),
                lstm=np.concatenate([u(scale * E ** -0.5, E * G), u(scale * H ** -0.5, H * G), u(0.1, G), u(0.1, G)]),
                proj=np.concatenate([u(scale * H ** -0.5, H * J), u(0.1, J)]) if proj else None,
                out=np.concatenate([u(out_scale * J ** -0.5, J * V), bias]), rng=rng)


def _case(name):
    """dict(m = the model, enc, n, act, ms = max_symbols_per_frame, max_labels)"""
    if name in ("awkward", "cap1", "cap2", "truncated", "lattice"):
        # batch 3, T 9, n_frames (9, 4, 0), E 7, H 12, J 20, V 5, tanh, with the projection
        ms = {"awkward": 3, "cap1": 1, "cap2": 2, "truncated": 3, "lattice": 4}[name]
        key = "awkward" if name == "truncated" else name
        seed, lb = SEEDS[key], LABEL_BIAS[key]
        m = _model(seed, 5, 7, 12, 20, True, label_bias=lb)
        n = [9, 4, 0] if name != "lattice" else [9, 4, 1]
        return dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, (3, 9, 20)).astype(np.float32), n=n, act="tanh", ms=ms,
                    max_labels=3 if name == "truncated" else None)
    if name in ("wide_relu", "wide_identity"):      # more classes than a wavefront, no projection
        m = _model(SEEDS[name], 70, 5, 33, 33, False, blank=69, label_bias=LABEL_BIAS["wide"])
        return dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, (2, 8, 33)).astype(np.float32), n=[8, 5], act=name.split("_")[1], ms=3,
                    max_labels=None)
    if name in ("tie_blank", "tie_label"):          # W_out = 0: the logits are the bias; two classes share the maximum
        blank, pair = (0, (0, 2)) if name == "tie_blank" else (3, (1, 3))
        m = _model(5, 5, 7, 12, 20, True, blank=blank)
        m["out"][:20 * 5] = 0.0
        m["out"][20 * 5:] = np.float32([-0.5, -0.25, -0.75, -1.0, -1.5])
        m["out"][20 * 5 + pair[0]] = m["out"][20 * 5 + pair[1]] = np.float32(0.375)
        return dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, (2, 6, 20)).astype(np.float32), n=[6, 3], act="tanh", ms=2, max_labels=None)
    if name == "stream":                            # T 12
        m = _model(SEEDS["stream"], 6, 5, 16, 16, False, blank=2, label_bias=LABEL_BIAS["stream"])
        return dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, (3, 12, 16)).astype(np.float32), n=[12, 12, 7], act="tanh", ms=3, max_labels=None)
    if name == "stream_w2":                         # the stream case's shapes with other weights
        m = _model(SEEDS["stream"] + 1000, 6, 5, 16, 16, False, blank=2, label_bias=LABEL_BIAS["stream"])
        return dict(_case("stream"), m=m)
    if name == "moderate":                          # batch 4, T 64, E = H = J = 64, V 40
        m = _model(SEEDS["moderate"], 40, 64, 64, 64, True, blank=0, label_bias=LABEL_BIAS["moderate"])
        return dict(m=m, enc=m["rng"].uniform(-1.5, 1.5, (4, 64, 64)).astype(np.float32), n=[64, 50, 64, 1], act="tanh", ms=4,
                    max_labels=None)
    raise KeyError(name)


# seeds chosen on the CPU so that _assert_premise holds (the reference's decision gap, the float32 restatement's agreement, no
# degenerate output); nothing about them comes from a device
SEEDS = {"awkward": 38, "cap1": 2, "cap2": 2, "lattice": 77, "wide_relu": 3, "wide_identity": 3, "stream": 0, "moderate": 2}
# added to every label's output bias: how often a row emits (the cap cases favour labels so that the cap fires)
LABEL_BIAS = {"awkward": -1.0, "cap1": 1.5, "cap2": 1.5, "lattice": -1.5, "wide": -2.5, "stream": -1.0, "moderate": -2.2}
GAP_CASES = ("awkward", "cap1", "cap2", "truncated", "lattice", "wide_relu", "wide_identity", "stream", "stream_w2", "moderate")
ALL_CASES = GAP_CASES + ("tie_blank", "tie_label")


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = _case(name)
    m = c["m"]
    kw = dict(n_frames=c["n"], blank=m["blank"], activation=c["act"], max_symbols_per_frame=c["ms"], max_labels=c["max_labels"])
    r64 = R.greedy_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], **kw)
    r32 = R.greedy_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], dtype=np.float32, **kw)
    return r64, r32


@functools.lru_cache(maxsize=None)
def _score_tol():
    err = max(float(np.abs(_reference(nm)[1]["scores"].astype(np.float64) - _reference(nm)[0]["scores"]).max()) for nm in ALL_CASES)
    print("largest float32-restatement score error over the cases: %.3e -> tolerance %.3e" % (err, 4 * err))
    assert err > 0
    return 4 * err


def _assert_premise(name, ends_on_label=True):
    r64, r32 = _reference(name)
    c = _case(name)
    live = [b for b, n in enumerate(c["n"]) if n > 0]
    print("%s: smallest decision gap %.3e; labels %s" % (name, min(r64["gaps"][b] for b in live), r64["labels"]))
    assert min(r64["gaps"][b] for b in live) >= GAP, (name, r64["gaps"])
    assert r32["labels"] == r64["labels"] and r32["frames"] == r64["frames"], name
    decisions = sum(len(x) for x in r64["cells"])
    n_labels = sum(len(x) for x in r64["labels"])
    assert 0 < n_labels < decisions + int(r64["capped"].sum()), (name, "needs blanks and labels")
    assert n_labels < decisions, (name, "needs a blank")
    assert any(np.bincount(f).max() >= 2 for f in r64["frames"] if f) or c["ms"] == 1, (name, "needs a frame with two labels")
    if ends_on_label:
        assert r64["ends_on_label"].any(), (name, "needs a row that ends on a label")


def _t(gpu, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _decoder(gpu, c):
    m = c["m"]
    return NL.RnntDecoder(_t(gpu, m["embed"]), _t(gpu, m["lstm"]), _t(gpu, m["proj"]), _t(gpu, m["out"]), blank=m["blank"],
                          joint_activation=c["act"], max_symbols_per_frame=c["ms"])


def _host(outs):
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in outs)


def _decode(gpu, dec, enc, n, max_labels=None):
    return _host(dec.decode(_t(gpu, enc), n, max_labels))


def _assert_equals_reference(name, got, r64):
    labels, frames, lengths, scores = got
    B, ML = labels.shape
    for b in range(B):
        k = len(r64["labels"][b])
        assert lengths[b] == k, (name, b, lengths[b], k)
        assert labels[b, :k].tolist() == r64["labels"][b] and (labels[b, k:] == -1).all(), (name, b, labels[b], r64["labels"][b])
        assert frames[b, :k].tolist() == r64["frames"][b] and (frames[b, k:] == -1).all(), (name, b)
    err = np.abs(scores.astype(np.float64) - r64["scores"]).max()
    print("%s: largest device score error %.3e (tolerance %.3e); scores %s" % (name, err, _score_tol(), r64["scores"]))
    assert err <= _score_tol(), (name, err, _score_tol())


def _check(gpu, name, ends_on_label=True):
    _assert_premise(name, ends_on_label)
    c = _case(name)
    dec = _decoder(gpu, c)
    got = _decode(gpu, dec, c["enc"], c["n"], c["max_labels"])
    dec.destroy()
    _assert_equals_reference(name, got, _reference(name)[0])
    return c, got


def test_awkward_widths(gpu):
    c, (labels, frames, lengths, scores) = _check(gpu, "awkward")
    assert lengths[2] == 0 and scores[2] == 0.0 and (labels[2] == -1).all()           # the row without frames
    assert labels.shape == (3, 27)                                                  # max_symbols_per_frame * T: never truncates


@pytest.mark.parametrize("name", ["wide_relu", "wide_identity"])
def test_more_classes_than_a_wavefront_without_projection(gpu, name):
    c, _ = _check(gpu, name, ends_on_label=False)
    assert c["m"]["proj"] is None and c["m"]["V"] > 64 and c["m"]["H"] == c["m"]["J"] == 33
    assert max(max(l) for l in _reference(name)[0]["labels"] if l) >= 64              # a winner in the second pass of the lanes' scan


@pytest.mark.parametrize("name,ms", [("cap1", 1), ("cap2", 2)])
def test_symbol_cap(gpu, name, ms):
    r64 = _reference(name)[0]
    assert r64["capped"].sum() >= 2 and _case(name)["ms"] == ms                      # the cap fires in the reference
    assert all(np.bincount(f).max() <= ms for f in r64["frames"] if f)
    # the unscored moves: every decision is scored once, and there are fewer blanks than frames consumed
    blanks = sum(len(cl) for cl in r64["cells"]) - sum(len(l) for l in r64["labels"])
    assert blanks + r64["capped"].sum() == sum(_case(name)["n"])
    _check(gpu, name)


def test_truncation(gpu):
    full = _reference("awkward")[0]
    assert len(full["labels"][0]) > 3 and _case("truncated")["max_labels"] == 3
    c, (labels, frames, lengths, scores) = _check(gpu, "truncated", ends_on_label=False)
    assert labels.shape == (3, 3) and lengths[0] == 3 and labels[0].tolist() == full["labels"][0][:3]
    assert len(full["labels"][1]) < 3 and (labels[1, lengths[1]:] == -1).all()       # a row below the cap keeps its -1 tail


@pytest.mark.parametrize("name", ["tie_blank", "tie_label"])
def test_exact_ties_go_to_the_lowest_index(gpu, name):
    c = _case(name)
    r64 = _reference(name)[0]
    assert all(g == 0.0 for g in r64["gaps"])
    if name == "tie_blank":
        assert all(l == [] for l in r64["labels"])
    else:
        assert r64["labels"] == [[1] * 12, [1] * 6] and r64["capped"].tolist() == [6, 3]
    dec = _decoder(gpu, c)
    got = _decode(gpu, dec, c["enc"], c["n"])
    dec.destroy()
    _assert_equals_reference(name, got, r64)


def test_nan_in_the_padding_changes_no_bit(gpu):
    c = _case("awkward")
    dec = _decoder(gpu, c)
    clean = _decode(gpu, dec, c["enc"], c["n"])
    enc = c["enc"].copy()
    for b, n in enumerate(c["n"]):
        enc[b, n:] = np.nan
    dirty = _decode(gpu, dec, enc, c["n"])
    dec.destroy()
    assert all(np.array_equal(a, b) for a, b in zip(clean, dirty))
    assert np.isfinite(dirty[3]).all()


def test_rows_are_independent_of_batch_position_neighbours_and_grouping(gpu):
    rpg = capi.load().nntk_shim_rnnt_dec_rows_per_group
    c = _case("awkward")
    m = c["m"]
    assert rpg(3, m["H"], m["J"], m["V"]) == 1 and rpg(GROUP_BATCH, m["H"], m["J"], m["V"]) == 1
    assert rpg(GROUP_BATCH + 1, m["H"], m["J"], m["V"]) == GROUP
    dec = _decoder(gpu, c)
    base = _decode(gpu, dec, c["enc"], c["n"], 27)
    rng = np.random.default_rng(11)
    for B in (1, GROUP_BATCH, GROUP_BATCH + 1, GROUP_BATCH + GROUP + 2):             # alone; one row a workgroup; grouped, with a ragged last group
        for b in range(3):
            T = 9 if B > 1 else max(c["n"][b], 1)                                    # alone: without the T padding as well
            enc = rng.uniform(-1.5, 1.5, (B, T, 20)).astype(np.float32)
            n = rng.integers(0, T + 1, B).astype(np.int32)
            at = (B - 1 - b) if B > 1 else 0                                         # another position, other neighbours
            enc[at, :T] = c["enc"][b, :T]
            n[at] = c["n"][b]
            got = _decode(gpu, dec, enc, n, 27)
            for g, ref in zip(got, base):
                assert np.array_equal(g[at], ref[b]), (B, b)
    dec.destroy()


def test_two_calls_return_the_same_bits(gpu):
    c = _case("moderate")
    dec = _decoder(gpu, c)
    a, b = _decode(gpu, dec, c["enc"], c["n"]), _decode(gpu, dec, c["enc"], c["n"])
    dec.destroy()
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def _push_all(gpu, dec, c, splits, max_labels, stream=None):
    """splits: per push the frames each row brings; the chunk tensor holds NaN behind a row's frames"""
    B, T, J = c["enc"].shape
    s = stream or NL.RnntGreedyStream(dec, B, max_labels)
    seen = [0] * B
    out = None
    for split in splits:
        w = max(max(split), 1)
        chunk = np.full((B, w, J), np.nan, np.float32)
        for b in range(B):
            chunk[b, :split[b]] = c["enc"][b, seen[b]:seen[b] + split[b]]
            seen[b] += split[b]
        out = s.push(_t(gpu, chunk), split)
    assert seen == list(c["n"])
    return s, _host(out)


def test_streaming_equals_the_one_shot_call_bit_for_bit(gpu):
    _assert_premise("stream", ends_on_label=False)
    c = _case("stream")
    assert c["enc"].shape[1] == 12 and c["n"] == [12, 12, 7]
    dec = _decoder(gpu, c)
    one = _decode(gpu, dec, c["enc"], c["n"], 36)
    _assert_equals_reference("stream", one, _reference("stream")[0])
    singles = [[1, 1, 1 if i < 7 else 0] for i in range(12)]
    ragged = [[5, 3, 0], [0, 0, 0], [7, 9, 7]]                                       # [5, 0, 7] for row 0, other cuts for the others
    for splits in (singles, ragged):
        s, got = _push_all(gpu, dec, c, splits, 36)
        assert all(np.array_equal(x, y) for x, y in zip(got, one)), splits
        # reset of row 1 restarts it and leaves the others alone
        s.reset([1])
        chunk = np.full((3, 12, 16), np.nan, np.float32)
        chunk[1] = c["enc"][1]
        again = _host(s.push(_t(gpu, chunk), [0, 12, 0]))
        assert all(np.array_equal(x, y) for x, y in zip(again, one))
        s.reset()                                                                    # every row
        _, got = _push_all(gpu, dec, c, ragged, 36, stream=s)
        assert all(np.array_equal(x, y) for x, y in zip(got, one))
        s.close()
    # other weights change the result; the first weights again restore the first bits
    m2 = _case("stream_w2")["m"]
    _assert_premise("stream_w2", ends_on_label=False)
    dec.load_weights(_t(gpu, m2["embed"]), _t(gpu, m2["lstm"]), None, _t(gpu, m2["out"]))
    two = _decode(gpu, dec, c["enc"], c["n"], 36)
    _assert_equals_reference("stream_w2", two, _reference("stream_w2")[0])
    assert not np.array_equal(two[0], one[0])
    m = c["m"]
    dec.load_weights(_t(gpu, m["embed"]), _t(gpu, m["lstm"]), None, _t(gpu, m["out"]))
    assert all(np.array_equal(x, y) for x, y in zip(_decode(gpu, dec, c["enc"], c["n"], 36), one))
    dec.destroy()


def test_agrees_with_the_training_path_on_the_device(gpu):
    """decode; build the lattice for the decoded labels with the library's own calls; the argmax walk from (0, 0) visits the decoder's
    cells and emits its labels, and the loss of those labels is at most -score (the greedy path is one of the alignments)"""
    _assert_premise("lattice", ends_on_label=False)                                  # (without the cap a row leaves its last frame by a blank)
    c = _case("lattice")
    m, r64 = c["m"], _reference("lattice")[0]
    assert r64["capped"].sum() == 0 and min(c["n"]) >= 1                             # every move is a lattice move
    dec = _decoder(gpu, c)
    labels, frames, lengths, scores = _decode(gpu, dec, c["enc"], c["n"])
    dec.destroy()
    _assert_equals_reference("lattice", (labels, frames, lengths, scores), r64)
    B, T, J = c["enc"].shape
    V, E, H, blank = m["V"], m["E"], m["H"], m["blank"]
    U1 = int(lengths.max()) + 1
    x = np.zeros((B, U1, E), np.float32)
    for b in range(B):
        x[b] = m["embed"][[blank] + labels[b, :lengths[b]].tolist() + [blank] * (U1 - 1 - lengths[b])]
    W, U, b_i, b_h = R.split_lstm(m["lstm"], E, H)
    lstm = NL.LSTM(E, H, True, U1)
    lstm.set_weights(W, U, b_i, b_h)
    h = lstm.apply_device_varlen(_t(gpu, x), lengths=lengths + 1)
    Wp, bp = R.split_dense(m["proj"], H, J)
    tdd = NL.TimeDistributedDense(U1, H, J)
    tdd.set_weights(Wp, bp)
    pred = tdd.apply_device(h)
    joint = NL.rnnt_joint_device(_t(gpu, c["enc"]), pred, c["act"])
    Wo, bo = R.split_dense(m["out"], J, V)
    voc = NL.TimeDistributedDense(T * U1, J, V)
    voc.set_weights(Wo, bo)
    logits = voc.apply_device(joint.reshape(B, T * U1, J)).reshape(B, T, U1, V)
    loss, _ = NL.rnnt_loss_device(logits, [labels[b, :lengths[b]].tolist() for b in range(B)], input_lengths=c["n"], blank=blank,
                                  want_grad=False)
    torch.cuda.synchronize()
    lg, loss = logits.cpu().numpy(), loss.cpu().numpy()
    for b in range(B):
        t = u = s = 0
        cells, walked = [], []
        while t < c["n"][b]:
            row = lg[b, t, u]
            top = np.sort(row)[-2:]
            assert top[1] - top[0] >= GAP / 2, (b, t, u)                             # the lattice's f32 logits: the same decision, half the gap
            k = int(np.argmax(row))
            cells.append((t, u))
            if k == blank:
                t, s = t + 1, 0
            else:
                walked.append(k); u += 1; s += 1
                if s == c["ms"]:
                    t, s = t + 1, 0
        assert cells == r64["cells"][b] and walked == r64["labels"][b], b
        print("row %d: loss %.6f, -score %.6f" % (b, loss[b], -scores[b]))
        assert loss[b] <= -float(scores[b]) + _score_tol(), (b, loss[b], scores[b])
    for o in (lstm, tdd, voc):
        o.destroy()


def test_moderate_shape(gpu):
    c, (labels, frames, lengths, scores) = _check(gpu, "moderate", ends_on_label=False)
    assert lengths.max() > 20                                                        # loop counts beyond the tiny cases


def test_host_form_equals_the_device_form(gpu):
    c = _case("awkward")
    m = c["m"]
    dec = _decoder(gpu, c)
    dev = _decode(gpu, dec, c["enc"], c["n"])
    dec.destroy()
    got = NL.rnnt_greedy_decode(m["embed"], m["lstm"], m["proj"], m["out"], c["enc"], c["n"], blank=m["blank"], joint_activation=c["act"],
                                max_symbols_per_frame=c["ms"])
    assert all(np.array_equal(x, y) for x, y in zip(got, dev))


def test_refusals_write_nothing(gpu):
    """the refusals of the decode call and of the handles that need a live decoder: -1, a message, outputs and state untouched"""
    L = capi.load()
    c = _case("stream")
    dec = _decoder(gpu, c)
    B, T, J = c["enc"].shape
    ML = 36
    enc = _t(gpu, c["enc"])
    one = _decode(gpu, dec, c["enc"], c["n"], ML)
    st = NL.RnntGreedyStream(dec, B, ML)
    first = _host(st.push(enc[:, :5].contiguous(), [5, 5, 5]))
    buf = torch.full((2 * B * ML + 2 * B + 8,), 7, dtype=torch.int32, device=gpu)
    lab, fr, ln = buf[:B * ML], buf[B * ML:2 * B * ML], buf[2 * B * ML:2 * B * ML + B]
    sc = torch.full((B,), 7.0, device=gpu)
    p = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())
    ip = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(capi.ip)
    good = dict(d=dec.h, s=None, enc=enc, B=B, T=T, n=c["n"], ML=ML, lab=lab, fr=fr, ln=ln, sc=sc)
    bad = [("NULL decoder", dict(d=None), "NULL"), ("NULL enc", dict(enc=None), "NULL"), ("NULL labels", dict(lab=None), "NULL"),
           ("NULL lengths", dict(ln=None), "NULL"), ("max_labels 0", dict(ML=0), "max_labels"), ("n_frames > T", dict(n=[12, 13, 7]), "n_frames"),
           ("n_frames < 0", dict(n=[12, -1, 7]), "n_frames"), ("batch differs from the state's", dict(s=st.h, B=B - 1, n=[12, 12]), "state"),
           ("misaligned enc", dict(enc=enc.data_ptr() + 2), "aligned"), ("misaligned labels", dict(lab=lab.data_ptr() + 1), "aligned"),
           ("labels overlap frames", dict(fr=lab.data_ptr() + 4 * (B * ML - 1)), "overlaps"),
           ("lengths overlap labels", dict(ln=lab.data_ptr() + 8), "overlaps"), ("scores overlap enc", dict(sc=enc.data_ptr() + 16), "overlaps"),
           ("labels overlap enc", dict(lab=enc.data_ptr()), "overlaps")]
    for name, change, word in bad:
        a = dict(good, **change)
        rc = L.nntk_rnnt_greedy_decode_device(a["d"], a["s"], p(a["enc"]), a["B"], a["T"], ip(a["n"]), a["ML"], p(a["lab"]), p(a["fr"]),
                                              p(a["ln"]), p(a["sc"]))
        torch.cuda.synchronize()
        assert rc == -1 and word in capi.last_error(), (name, capi.last_error())
        assert (buf == 7).all() and (sc == 7.0).all() and torch.equal(enc.cpu(), torch.from_numpy(c["enc"])), name
    assert not L.nntk_rnnt_decode_state_create(dec.h, 0) and "batch" in capi.last_error()
    assert L.nntk_rnnt_decode_state_reset(st.h, ip([3]), 1) == -1 and "rows" in capi.last_error()
    assert L.nntk_rnnt_decode_state_reset(st.h, None, 2) == -1 and "NULL" in capi.last_error()
    m = c["m"]
    assert L.nntk_rnnt_decoder_load_weights_device(dec.h, p(_t(gpu, m["embed"])), None, None, p(_t(gpu, m["out"]))) == -1
    assert "NULL" in capi.last_error()
    # ... and the state is where the first push left it: the rest of the stream gives the one-shot result
    rest = _host(st.push(enc[:, 5:].contiguous(), [7, 7, 2]))
    assert all(np.array_equal(x, y) for x, y in zip(rest, one))
    st.close(); dec.destroy()
