"""The predictor handle (csrc/host/rnnt_pred.c): the decoder's prediction network in training.

References: (1) the composed recipe a caller had to write before -- the lookup in numpy, then LSTMApplyTrainingBatchDeviceVarLen /
LSTMCalculateGradientDeviceVarLen and TimeDistributedDense training, the recipe of
tests/test_gpu_rnnt_decode.py::test_agrees_with_the_training_path_on_the_device -- whose bits pred, d_dlstm and d_dproj must equal;
(2) torch float64 autograd on the CPU over nn.Embedding, an LSTM written in rnnt_decode_reference.split_lstm's gate order (i, f, g, o)
and a linear layer.  The scalar of (2) is sum(pred G) over the LIVE cells u <= U_b: the handle ignores d_dpred in the padding.

Tolerances against float64 are those of the ragged LSTM training comparison, tests/test_gpu_train_varlen.py:343 and :347 with
check_grads at :160-167: forward rtol 2e-5 / atol 2e-6, gradients 2e-7 sqrt(B T) max(1, |ref|max), T = U1 here.  The embedding gradient
against the float64 scatter of the recipe's d_dX has the derived bound of tests/test_gpu_embedding.py: (n - 1) 2^-24 sum |terms|."""
import ctypes as C

import numpy as np
import pytest
import torch

import rnnt_decode_reference as R
from nntoolkitcore_amd import capi, layers as NL

pytestmark = pytest.mark.gpu
DP = lambda t: C.c_void_p(t.data_ptr())
IP = lambda a: a.ctypes.data_as(capi.ip)

# B, max_label_len, V, E, H, J, projection, label rows
CASES = {
    "proj": (3, 4, 6, 5, 8, 7, True, [[2, 2, 5, 1], [], [3, 3]]),
    "identity": (3, 4, 6, 5, 8, 8, False, [[2, 2, 5, 1], [], [3, 3]]),
    "start-symbol-70": (70, 3, 9, 16, 32, 16, True, None),
}


def _t(gpu, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _case(name):
    B, maxL, V, E, H, J, proj, labels = CASES[name]
    rng = np.random.default_rng(len(name) + B)
    if labels is None:                                                      # lengths 0 .. maxL, repeated labels among them
        labels = [rng.integers(1, V, b % (maxL + 1)).tolist() for b in range(B)]
        labels[5] = [4, 4, 4]
    u = lambda sc, *s: rng.uniform(-sc, sc, s).astype(np.float32)
    m = dict(B=B, maxL=maxL, U1=maxL + 1, V=V, E=E, H=H, J=J, blank=0, labels=labels, lens=np.array([len(r) for r in labels], np.int32),
             embed=u(1.0, V, E), lstm=u(0.4, 4 * H * (E + H + 2)), proj=u(0.4, (H + 1) * J) if proj else None)
    assert {0, maxL} <= set(m["lens"].tolist()) and any(len(r) != len(set(r)) for r in labels)
    m["G"] = u(1.0, B, m["U1"], J)
    return m


def _ids(m):
    ids = np.full((m["B"], m["U1"]), -1, np.int32)
    for b, r in enumerate(m["labels"]):
        ids[b, :len(r) + 1] = [m["blank"]] + r
    return ids


def _predictor(gpu, m):
    p = NL.RnntPredictor(m["V"], m["E"], m["H"], m["J"], m["B"], m["maxL"], blank=m["blank"], proj=m["proj"] is not None)
    p.load_weights(_t(gpu, m["embed"]), _t(gpu, m["lstm"]), None if m["proj"] is None else _t(gpu, m["proj"]))
    return p


def _run(gpu, m, dpred, prefill=None):
    """forward and backward through the handle -> pred, dembed, dlstm, dproj (host arrays)"""
    p = _predictor(gpu, m)
    pred = p.forward(m["labels"])
    mk = lambda *s: None if prefill is None else torch.full(s, prefill, device=gpu)
    g = p.backward(_t(gpu, dpred), dembed=mk(m["V"], m["E"]), dlstm=mk(m["lstm"].size), dproj=None if m["proj"] is None else mk(m["proj"].size))
    torch.cuda.synchronize()
    p.destroy()
    return (pred.cpu().numpy(),) + tuple(None if x is None else x.cpu().numpy() for x in g)


def _recipe(gpu, m, dpred_masked):
    """the composed recipe: numpy lookup, the ragged LSTM training calls, TimeDistributedDense training and gradient -> pred, dX, dlstm, dproj"""
    L = capi.load()
    B, U1, E, H, J = m["B"], m["U1"], m["E"], m["H"], m["J"]
    ids = _ids(m)
    x = _t(gpu, np.where((ids >= 0)[..., None], m["embed"][np.maximum(ids, 0)], np.float32(0)))
    lens = (m["lens"] + 1).astype(np.int32)
    lstm = NL.LSTM(E, H, True, U1, mini_batch=B)
    assert L.LSTMLoadWeightsDevice(lstm.h, DP(_t(gpu, m["lstm"]))) == 0, capi.last_error()
    h = torch.empty((B, U1, H), device=gpu)
    assert L.LSTMApplyTrainingBatchDeviceVarLen(lstm.h, DP(x), DP(h), IP(lens), None, None, None, None) == 0, capi.last_error()
    dlstm, dX = torch.zeros(m["lstm"].size, device=gpu), torch.empty((B, U1, E), device=gpu)
    if m["proj"] is None:
        pred, dproj, dh = h, None, _t(gpu, dpred_masked)
        tdd = None
    else:
        tdd = L.TimeDistributedDenseCreateForTraining(L.TimeDistributedDenseConfigCreate(U1, L.DenseConfigCreate(H, J, None)), capi.ConvTrainingConfig(B))
        assert tdd, capi.last_error()
        assert L.TimeDistributedDenseLoadWeightsDevice(tdd, DP(_t(gpu, m["proj"]))) == 0, capi.last_error()
        pred = torch.empty((B, U1, J), device=gpu)
        assert L.TimeDistributedDenseApplyTrainingBatchDevice(tdd, DP(h), DP(pred)) == 0, capi.last_error()
        dproj, dh = torch.zeros(m["proj"].size, device=gpu), torch.empty((B, U1, H), device=gpu)
        assert L.TimeDistributedDenseCalculateGradientDevice(tdd, DP(dproj), DP(dh), DP(_t(gpu, dpred_masked))) == 0, capi.last_error()
    assert L.LSTMCalculateGradientDeviceVarLen(lstm.h, DP(dlstm), DP(dX), DP(dh), None, None, None, None) == 0, capi.last_error()
    torch.cuda.synchronize()
    out = (pred.cpu().numpy(), dX.cpu().numpy(), dlstm.cpu().numpy(), None if dproj is None else dproj.cpu().numpy())
    lstm.destroy()
    if tdd:
        L.TimeDistributedDenseDestroy(tdd)
    return out


def _masked(m, a, fill=0.0):
    a = a.copy()
    for b, n in enumerate(m["lens"]):
        a[b, n + 1:] = fill
    return a


@pytest.mark.parametrize("name", list(CASES))
def test_bits_of_the_composed_recipe(gpu, name):
    m = _case(name)
    pred, dembed, dlstm, dproj = _run(gpu, m, m["G"])
    r_pred, r_dX, r_dlstm, r_dproj = _recipe(gpu, m, _masked(m, m["G"]))
    assert np.array_equal(pred.view(np.int32), r_pred.view(np.int32))
    assert np.array_equal(dlstm.view(np.int32), r_dlstm.view(np.int32))
    assert (dproj is None and r_dproj is None) or np.array_equal(dproj.view(np.int32), r_dproj.view(np.int32))
    # padding: h is zeros, pred the projection's bias (zeros without one)
    bias = np.zeros(m["J"], np.float32) if m["proj"] is None else R.split_dense(m["proj"], m["H"], m["J"])[1]
    for b, n in enumerate(m["lens"]):
        assert (pred[b, n + 1:] == bias).all()
    ids, dX = _ids(m).reshape(-1), r_dX.reshape(-1, m["E"]).astype(np.float64)
    worst = 0.0
    for v in range(m["V"]):
        r = np.flatnonzero(ids == v)
        if r.size == 0:
            assert (dembed[v] == 0).all()
            continue
        err = np.abs(dembed[v] - dX[r].sum(0))
        bound = (r.size - 1) * 2.0 ** -24 * np.abs(dX[r]).sum(0)
        assert (err <= bound).all(), (v, r.size, err.max())
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print("%s: the start symbol occurs %d times; d embed: largest error / bound %.4f" % (name, (ids == m["blank"]).sum(), worst))


def _torch64(m):
    """nn.Embedding -> LSTM (gates i, f, g, o as split_lstm lays them out) -> linear, float64 autograd on the CPU; the scalar is
    sum(pred G) over the live cells"""
    B, U1, E, H, J = m["B"], m["U1"], m["E"], m["H"], m["J"]
    emb = torch.nn.Embedding(m["V"], E).double()
    emb.weight.data = torch.from_numpy(m["embed"].astype(np.float64))
    lstm = torch.from_numpy(m["lstm"].astype(np.float64)).requires_grad_(True)
    G4 = 4 * H
    W, U, b_i, b_h = lstm[:E * G4].view(E, G4), lstm[E * G4:(E + H) * G4].view(H, G4), lstm[(E + H) * G4:(E + H + 1) * G4], lstm[(E + H + 1) * G4:]
    proj = None if m["proj"] is None else torch.from_numpy(m["proj"].astype(np.float64)).requires_grad_(True)
    ids = _ids(m)
    rows, scalar = [], 0.0
    Gt = torch.from_numpy(m["G"].astype(np.float64))
    for b in range(B):
        h, c = torch.zeros(H, dtype=torch.float64), torch.zeros(H, dtype=torch.float64)
        out = []
        for u in range(U1):
            if ids[b, u] < 0:
                h = torch.zeros(H, dtype=torch.float64)
            else:
                z = emb(torch.tensor(int(ids[b, u]))) @ W + b_i + h @ U + b_h
                i, f, g, o = torch.sigmoid(z[:H]), torch.sigmoid(z[H:2 * H]), torch.tanh(z[2 * H:3 * H]), torch.sigmoid(z[3 * H:])
                c = f * c + i * g
                h = o * torch.tanh(c)
            p = h if proj is None else h @ proj[:H * J].view(H, J) + proj[H * J:]
            out.append(p)
            if ids[b, u] >= 0:
                scalar = scalar + (p * Gt[b, u]).sum()
        rows.append(torch.stack(out))
    scalar.backward()
    return (torch.stack(rows).detach().numpy(), emb.weight.grad.numpy(), lstm.grad.numpy(), None if proj is None else proj.grad.numpy())


@pytest.mark.parametrize("name", list(CASES))
def test_against_torch_float64_autograd(gpu, name):
    m = _case(name)
    pred, dembed, dlstm, dproj = _run(gpu, m, m["G"])
    r_pred, r_dembed, r_dlstm, r_dproj = _torch64(m)
    print("%s pred: largest error %.2e" % (name, np.abs(pred - r_pred).max()))
    np.testing.assert_allclose(pred, r_pred, rtol=2e-5, atol=2e-6)                   # tests/test_gpu_train_varlen.py:343
    tol = 2e-7 * np.sqrt(m["B"] * m["U1"])                                           # tests/test_gpu_train_varlen.py:347, :160-167
    for part, a, b_ in (("d embed", dembed, r_dembed), ("d lstm", dlstm, r_dlstm), ("d proj", dproj, r_dproj)):
        if a is None:
            continue
        sc = max(1.0, float(np.abs(b_).max()))
        err = float(np.abs(a.reshape(-1) - b_.reshape(-1)).max())
        print("%s %s: %.2e (scale %.1f, bound %.2e)" % (name, part, err, sc, tol * sc))
        assert np.isfinite(a).all() and err <= tol * sc, (name, part, err, tol * sc)


@pytest.mark.parametrize("name", ["proj", "identity"])
def test_nan_in_the_padding_of_dpred_reaches_nothing(gpu, name):
    m = _case(name)
    zeros = _run(gpu, m, _masked(m, m["G"], 0.0))
    nans = _run(gpu, m, _masked(m, m["G"], np.nan))
    assert np.isnan(_masked(m, m["G"], np.nan)).any()
    for a, b_ in zip(zeros[1:], nans[1:]):
        assert (a is None and b_ is None) or (np.isfinite(b_).all() and np.array_equal(a.view(np.int32), b_.view(np.int32)))


def test_labels_beyond_a_rows_length_are_neither_checked_nor_read(gpu):
    """the header's choice: labels[b][i >= U_b] may hold anything"""
    m = _case("proj")
    p = _predictor(gpu, m)
    want = p.forward(m["labels"]).clone()
    lab = np.full((m["B"], m["maxL"]), 10 ** 6, np.int32)
    for b, r in enumerate(m["labels"]):
        lab[b, :len(r)] = r
    got = p.forward(lab, m["lens"])
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    p.destroy()


def test_gradient_blocks_are_overwritten(gpu):
    for name in ("proj", "identity"):
        m = _case(name)
        fresh, filled = _run(gpu, m, m["G"], prefill=0.0), _run(gpu, m, m["G"], prefill=7.0)
        for a, b_ in zip(fresh[1:], filled[1:]):
            assert (a is None and b_ is None) or np.array_equal(a.view(np.int32), b_.view(np.int32))


def test_refusals_of_a_live_handle_enqueue_nothing(gpu):
    m = _case("proj")
    L = capi.load()
    p = NL.RnntPredictor(m["V"], m["E"], m["H"], m["J"], m["B"], m["maxL"])
    assert p.device_bytes() > 0
    pred = torch.full((m["B"], m["U1"], m["J"]), 7.0, device=gpu)
    g = [torch.full((n,), 7.0, device=gpu) for n in (m["V"] * m["E"], m["lstm"].size, m["proj"].size)]
    with pytest.raises(capi.NNTKError, match="no weights"):
        p.forward(m["labels"], pred=pred)
    embed, lstm, proj = _t(gpu, m["embed"]), _t(gpu, m["lstm"]), _t(gpu, m["proj"])
    with pytest.raises(capi.NNTKError, match="exactly when"):
        p.load_weights(embed, lstm, None)
    p.load_weights(embed, lstm, proj)
    with pytest.raises(capi.NNTKError, match="no forward"):
        p.backward(pred, *g)
    for labels, word in (([[2, 6], [], []], "not a class"), ([[2, 0], [], []], "is the blank"), ([[-1], [], []], "not a class")):
        with pytest.raises(capi.NNTKError, match=word):
            p.forward(labels, pred=pred)
    lab = np.ones((m["B"], m["maxL"]), np.int32)
    for lens in ([5, 0, 0], [0, -1, 0]):
        with pytest.raises(capi.NNTKError, match="label_lengths"):
            p.forward(lab, np.array(lens, np.int32), pred=pred)
    assert L.nntk_rnnt_predictor_forward_device(p.h, IP(lab), None, None) == -1 and "d_pred is NULL" in capi.last_error()
    assert L.nntk_rnnt_predictor_forward_device(p.h, None, None, DP(pred)) == -1 and "labels is NULL" in capi.last_error()
    with pytest.raises(capi.NNTKError, match="no forward"):                          # a refused forward is no forward
        p.backward(pred, *g)
    p.forward(m["labels"])
    assert L.nntk_rnnt_predictor_backward_device(p.h, DP(pred), DP(g[0]), DP(g[1]), None) == -1 and "exactly when" in capi.last_error()
    assert L.nntk_rnnt_predictor_backward_device(p.h, DP(pred), None, DP(g[1]), DP(g[2])) == -1 and "d_dembed is NULL" in capi.last_error()
    torch.cuda.synchronize()
    assert all(bool((x == 7.0).all()) for x in g) and bool((pred == 7.0).all())
    p.destroy()
    q = NL.RnntPredictor(m["V"], m["E"], m["H"], m["H"], m["B"], m["maxL"], proj=False)
    with pytest.raises(capi.NNTKError, match="exactly when"):
        q.load_weights(embed, lstm, proj)
    q.destroy()


def _path_score(enc, pred, out_block, J, V, labels, frames, n_frames, blank, max_symbols):
    """the score of the decoder's own path, recomputed in float64 from pred [U1, J], enc [T, J] and the vocabulary block"""
    Wo, bo = R.split_dense(out_block.astype(np.float64), J, V)
    t = u = s = 0
    score = 0.0
    while t < n_frames:
        logits = np.tanh(enc[t].astype(np.float64) + pred[u].astype(np.float64)) @ Wo + bo
        lp = logits - logits.max() - np.log(np.exp(logits - logits.max()).sum())
        if u < len(labels) and frames[u] == t:
            score += lp[labels[u]]
            u, s = u + 1, s + 1
            if s == max_symbols:
                t, s = t + 1, 0
        else:
            score += lp[blank]
            t, s = t + 1, 0
    assert u == len(labels)
    return score


def test_one_whole_training_step_on_the_device(gpu):
    """predictor forward -> fused loss -> predictor backward -> one SGD step of the device optimizer on enc, embed, lstm, proj and out ->
    load_weights: the loss on the same batch goes down, only the embedding rows in use move, and the decoder takes the four updated
    blocks.  Then the decoder's greedy path is scored again from the predictor's teacher-forced pred in float64.  Its tolerance restates
    tests/test_gpu_rnnt_decode.py::_score_tol: four times the largest score difference between the float64 reference decoder and its
    sequential float32 restatement (rnnt_decode_reference.greedy_decode, dtype float32), here on this test's own model and batch."""
    rng = np.random.default_rng(12)
    B, T, J, V, E, H, blank, ms = 2, 5, 16, 8, 6, 12, 0, 10
    labels, lens = [[3, 3, 5], [1, 7]], [5, 4]
    maxL = 3
    u = lambda sc, *s: torch.from_numpy(rng.uniform(-sc, sc, s).astype(np.float32)).to(gpu)
    enc, embed, lstm, proj, out = u(1.0, B, T, J), u(1.0, V, E), u(0.4, 4 * H * (E + H + 2)), u(0.4, (H + 1) * J), u(0.5, J * V + V)
    embed0 = embed.clone()
    grads = [torch.zeros_like(w) for w in (enc, embed, lstm, proj, out)]
    denc, dembed, dlstm, dproj, dout = grads
    opt = NL.Optimizer("sgd", list(zip((enc, embed, lstm, proj, out), grads)), learning_rate=0.05, zero_gradients=1)
    p = NL.RnntPredictor(V, E, H, J, B, maxL, blank=blank)
    losses = []
    for step in range(2):
        p.load_weights(embed, lstm, proj)
        pred = p.forward(labels)
        if step == 0:
            loss, _, dpred, _ = NL.rnnt_fused_loss_device(enc, pred, out, labels, input_lengths=lens, blank=blank, denc=denc, dout=dout)
            p.backward(dpred, dembed=dembed, dlstm=dlstm, dproj=dproj)
            assert all(float(g.abs().sum()) > 0 for g in grads)
            used = sorted({blank} | {k for r in labels for k in r})
            assert all(float(dembed[v].abs().sum()) > 0 for v in used)
            opt.step()
        else:
            loss = NL.rnnt_fused_loss_device(enc, pred, out, labels, input_lengths=lens, blank=blank, want_grad=False)[0]
        losses.append(float(loss.sum()))
    torch.cuda.synchronize()
    print("summed transducer loss: %.5f before the step, %.5f after" % (losses[0], losses[1]))
    assert np.isfinite(losses).all() and losses[1] < losses[0]
    for v in range(V):
        assert torch.equal(embed[v], embed0[v]) == (v not in used), v
    dec = NL.RnntDecoder(embed, lstm, proj, out, blank=blank, joint_activation="tanh", max_symbols_per_frame=ms)
    dec.load_weights(embed, lstm, proj, out)
    got, frames, lengths, scores = (o.cpu().numpy() for o in dec.decode(enc, lens))
    dec.destroy()
    assert np.isfinite(scores).all()
    h = lambda t: t.cpu().numpy()
    r64 = R.greedy_decode(h(embed), h(lstm), h(proj), h(out), h(enc), lens, blank=blank, activation="tanh", max_symbols_per_frame=ms)
    r32 = R.greedy_decode(h(embed), h(lstm), h(proj), h(out), h(enc), lens, blank=blank, activation="tanh", max_symbols_per_frame=ms,
                          dtype=np.float32)
    tol = 4 * float(np.abs(r32["scores"].astype(np.float64) - r64["scores"]).max())
    assert tol > 0
    q = NL.RnntPredictor(V, E, H, J, B, int(lengths.max()), blank=blank)
    q.load_weights(embed, lstm, proj)
    tf = q.forward([got[b, :lengths[b]].tolist() for b in range(B)]).cpu().numpy()
    for b in range(B):
        s = _path_score(h(enc)[b], tf[b], h(out), J, V, got[b, :lengths[b]].tolist(), frames[b], lens[b], blank, ms)
        print("row %d: decoder score %.6f, teacher-forced float64 score %.6f (tolerance %.2e)" % (b, scores[b], s, tol))
        assert abs(float(scores[b]) - s) <= tol, (b, scores[b], s, tol)
    for o in (p, q, opt):
        o.destroy()
