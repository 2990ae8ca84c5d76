"""Ragged batches with carried state: the *ApplyDeviceVarLen / *ApplyInferenceBatchVarLen calls and the ragged
bidirectional helpers, on every kernel family a batch call takes: the register-resident split-K kernels (gru_rr_kernel /
lstm_rr_kernel, both hand-off protocols), the full-K kernels (*_fk_kernel), rec_persistent_kernel, rec_step_kernel, RNN.

Row b with L = lengths[b] must equal the reference's stateful single-sequence recurrence on x[b, :L] from h0[b] (c0[b]);
sequence outputs past L are exactly 0; for every step a row runs the bits equal the zero-state *ApplyDevice call's.
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from nntoolkitcore_amd import capi, layers as NL

pytestmark = pytest.mark.gpu

ATOL, RTOL = 1e-5, 1e-5      # the single-layer tolerance of tests/test_gpu_parity.py, tests/test_gpu_lstm_rr.py, tests/test_gpu_fk.py


def u(r, *shape, sc=1.0):
    return r.uniform(-sc, sc, shape).astype(np.float32)


def close(a, b, atol=ATOL, rtol=RTOL):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.isfinite(a).all()
    err = np.abs(a - b)
    bad = err > atol + rtol * np.abs(b)
    assert not bad.any(), "max abs err %.3e at %d/%d elements" % (err.max(), bad.sum(), bad.size)


def ragged_lengths(r, B, T):
    """0, 1 and T mixed with random lengths; one long row in a tile of short rows; a whole tile of zeros next to full tiles"""
    lens = r.integers(0, T + 1, B)
    lens[:4] = [0, 1, T, 0]
    lens[4:64] = r.integers(0, 3, 60)            # tile 0: short rows ...
    lens[37] = T                                 # ... and one long one
    if B > 128:
        lens[64:128] = 0                         # tile 1: empty
        lens[128:] = T                           # tile 2: full
    return lens.astype(np.int32)


def last_kernel():
    return capi.load().nntk_hip_last_recurrent_kernel().decode()


# (kind, I, H, acts, options, family): every route a batch call takes
CASES = [
    ("gru", 16, 128, None, {}, "gru_rr_kernel<4,1>"),                       # pending-pattern hand-off, f32 x
    ("lstm", 96, 256, None, {}, "lstm_rr_kernel<4,2>"),                     # pending-pattern hand-off
    ("lstm", 128, 512, None, {}, "lstm_rr_kernel<8,2>"),                    # flag protocol
    ("gru", 256, 256, None, {}, "gru_fk_kernel<16,16,4>"),                  # full-K
    ("lstm", 256, 256, None, {}, "lstm_fk_kernel<16,16,4>"),
    ("gru", 12, 40, "nondefault", {}, "rec_persistent_kernel<3,GRU>"),
    ("lstm", 20, 72, None, {}, "rec_persistent_kernel<4,LSTM>"),              # H % 16 != 0: not the register-resident family
    ("lstm", 16, 64, None, {"rec_rr": "0"}, "rec_persistent_kernel<4,LSTM>"),
    ("lstm", 16, 64, None, {"rec_rr": "0", "rec_persistent": "0"}, "rec_step_kernel<4,LSTM>"),
    ("gru", 12, 33, None, {"rec_persistent": "0"}, "rec_step_kernel<3,GRU>"),
    ("rnn", 10, 48, None, {}, "rec_persistent_kernel<1,RNN>"),
    ("rnn", 10, 48, None, {"rec_persistent": "0"}, "rec_step_kernel<1,RNN>"),
]
IDS = ["gru-rr4", "lstm-rr4", "lstm-rr8-H512", "gru-fk", "lstm-fk", "gru-acts", "lstm-H72", "lstm-rr0", "lstm-step", "gru-step-H33", "rnn", "rnn-step"]


class Layer:
    """one handle plus its weights and the oracle call for one sequence"""

    def __init__(self, kind, I, H, acts, T, seq, seed=0, weights=None):
        L = capi.load()
        self.kind, self.I, self.H, self.T = kind, I, H, T
        r = np.random.default_rng(seed + 1000 * I + H)
        G = {"gru": 3, "lstm": 4, "rnn": 1}[kind]
        self.w = weights if weights is not None else (u(r, I, G * H, sc=I ** -0.5), u(r, H, G * H, sc=H ** -0.5),
                                                      u(r, G * H, sc=0.1), u(r, G * H, sc=0.1))
        self.oacts = None
        if kind == "gru":
            a = None
            if acts == "nondefault":     # (z, h, r)
                a = L.GRUActivationsCreate(L.ActivationFunctionCreateTanh(H), L.ActivationFunctionCreateReLU(H, 1.0),
                                           L.ActivationFunctionCreateSigmoid(H))
                self.oacts = (O.ACT_TANH, O.ACT_RELU, O.ACT_SIGMOID)
            self.layer = NL.GRU(I, H, seq, T, acts=a)
        elif kind == "lstm":
            self.layer = NL.LSTM(I, H, seq, T, v2=True)
        else:
            self.layer = NL.RNN(I, H, seq, T, v2=True)
        self.layer.set_weights(*self.w)
        self.seq = seq

    def oracle(self, x, h0, c0):
        """single sequence x [L, in] from (h0, c0): (out, h, c)"""
        kw = {} if self.oacts is None else {"acts": self.oacts}
        if self.kind == "gru":
            out, h = O.gru(x, *self.w, h0=h0, return_sequences=self.seq, **kw)
            return out, h, None
        if self.kind == "lstm":
            return O.lstm(x, *self.w, h0=h0, c0=c0, return_sequences=self.seq, v2=True)
        out, h = O.rnn(x, *self.w, h0=h0, return_sequences=self.seq, v2=True)
        return out, h, None

    def destroy(self):
        self.layer.destroy()


def set_options(opts):
    for k, v in opts.items():
        capi.set_option(k, v)


def run_vl(lay, x, lens, h0, c0):
    res = lay.layer.apply_device_varlen(x, lengths=lens, h0=h0, c0=c0 if lay.kind == "lstm" else None, return_state=True)
    return res if lay.kind == "lstm" else res + (None,)


@pytest.mark.parametrize("kind,I,H,acts,opts,family", CASES, ids=IDS)
@pytest.mark.parametrize("seq", [True, False])
def test_varlen_against_oracle(gpu, kind, I, H, acts, opts, family, seq):
    import torch
    set_options(opts)
    B, T = 130, 9
    r = np.random.default_rng(H + 7 * I + seq)
    lay = Layer(kind, I, H, acts, T, seq)
    xs, h0s, c0s = u(r, B, T, I), u(r, B, H, sc=0.5), u(r, B, H, sc=0.5)
    lens = ragged_lengths(r, B, T)
    x, h0, c0 = (torch.from_numpy(a).cuda() for a in (xs, h0s, c0s))
    out, hT, cT = run_vl(lay, x, lens, h0, c0)
    torch.cuda.synchronize()
    assert last_kernel() == family
    out, hT = out.cpu().numpy(), hT.cpu().numpy()
    cT = cT.cpu().numpy() if cT is not None else None
    for b in range(B):
        L = int(lens[b])
        if L == 0:                      # the state passes through untouched
            assert np.array_equal(hT[b], h0s[b])
            if cT is not None:
                assert np.array_equal(cT[b], c0s[b])
            if seq:
                assert not out[b].any()
            else:
                assert np.array_equal(out[b], h0s[b])
            continue
        ro, rh, rc = lay.oracle(xs[b, :L], h0s[b], c0s[b])
        close(hT[b], rh)
        if rc is not None:
            close(cT[b], rc, atol=2 * ATOL)      # (the cell state: tests/test_gpu_lstm_rr.py)
        if seq:
            close(out[b, :L], ro)
            assert not out[b, L:].any(), "padding must be exactly zero"
        else:
            close(out[b], ro)
    lay.destroy()


@pytest.mark.parametrize("kind,I,H,acts,opts,family", CASES, ids=IDS)
def test_varlen_same_bits_as_apply_device(gpu, kind, I, H, acts, opts, family):
    import torch
    set_options(opts)
    B, T = 67, 11
    r = np.random.default_rng(H + I)
    lay = Layer(kind, I, H, acts, T, True)
    x = torch.from_numpy(u(r, B, T, I)).cuda()
    full = lay.layer.apply_device(x).clone()
    assert last_kernel() == family
    assert torch.equal(lay.layer.apply_device_varlen(x, lengths=[T] * B), full)
    assert last_kernel() == family
    assert torch.equal(lay.layer.apply_device_varlen(x), full)
    lens = ragged_lengths(r, B, T)
    out, hT, _ = run_vl(lay, x, lens, None, None)
    for b in range(B):
        L = int(lens[b])
        assert torch.equal(out[b, :L], full[b, :L])
        if L:
            assert torch.equal(hT[b], full[b, L - 1])
        else:
            assert not hT[b].any()
    lay.destroy()


@pytest.mark.parametrize("kind,I,H,acts,opts,family", CASES, ids=IDS)
@pytest.mark.parametrize("ragged", [False, True])
def test_chunked_streaming_equals_one_call(gpu, kind, I, H, acts, opts, family, ragged):
    """two calls on a T = tau handle, state carried, give the bits of one call on a T = 2 tau handle"""
    import torch
    set_options(opts)
    B, tau = 130, 6
    r = np.random.default_rng(3 * H + I)
    one = Layer(kind, I, H, acts, 2 * tau, True)
    half = Layer(kind, I, H, acts, tau, True, weights=one.w)
    x = torch.from_numpy(u(r, B, 2 * tau, I)).cuda()
    h0 = torch.from_numpy(u(r, B, H, sc=0.5)).cuda()
    c0 = torch.from_numpy(u(r, B, H, sc=0.5)).cuda()
    lens = ragged_lengths(r, B, 2 * tau) if ragged else np.full(B, 2 * tau, np.int32)
    l1, l2 = np.minimum(lens, tau), np.maximum(lens - tau, 0)
    out, hT, cT = run_vl(one, x, lens, h0, c0)
    o1, h1, c1 = run_vl(half, x[:, :tau].contiguous(), l1, h0, c0)
    o2, h2, c2 = run_vl(half, x[:, tau:].contiguous(), l2, h1, c1)
    assert last_kernel() == family
    assert torch.equal(torch.cat([o1, o2], 1), out)
    assert torch.equal(h2, hT)
    if cT is not None:
        assert torch.equal(c2, cT)
    one.destroy()
    half.destroy()


@pytest.mark.parametrize("kind,I,H,acts,opts,family", [CASES[0], CASES[2], CASES[3], CASES[5], CASES[6], CASES[10]],
                         ids=["gru-rr", "lstm-rr8", "gru-fk", "gru-acts", "lstm-H72", "rnn"])
@pytest.mark.parametrize("merge", ["concat", "sum"])
def test_bidirectional_ragged(gpu, kind, I, H, acts, opts, family, merge):
    import torch
    B, T = 130, 8
    r = np.random.default_rng(11 * H)
    fwd, bwd = Layer(kind, I, H, acts, T, True, seed=1), Layer(kind, I, H, acts, T, True, seed=2)
    xs = u(r, B, T, I)
    lens = ragged_lengths(r, B, T)
    x = torch.from_numpy(xs).cuda()
    of = fwd.layer.apply_device_varlen(x, lengths=lens)
    ob = bwd.layer.apply_device_varlen(NL.bd_reverse_device(x, "input", lengths=lens), lengths=lens)
    ob = NL.bd_reverse_device(ob, "backward", lengths=lens)
    got = NL.bd_merge_device(of, ob, merge).cpu().numpy()
    for b in range(B):
        L = int(lens[b])
        assert not got[b, L:].any()
        if not L:
            continue
        rf = fwd.oracle(xs[b, :L], None, None)[0]
        rb = bwd.oracle(xs[b, :L][::-1].copy(), None, None)[0][::-1]
        close(got[b, :L], np.concatenate([rf, rb], -1) if merge == "concat" else rf + rb, atol=2 * ATOL)
    fwd.destroy()
    bwd.destroy()


def test_varlen_errors_leave_output_untouched(gpu):
    import torch
    L = capi.load()
    B, T, I, H = 5, 6, 4, 8
    lay = Layer("lstm", I, H, None, T, True)
    x = torch.zeros(B, T, I, device="cuda")
    out = torch.full((B, T, H), 7.0, device="cuda")
    nul = C.c_void_p(None)
    for bad in ([0, 1, -1, 2, 3], [0, 1, T + 1, 2, 3]):
        arr = (C.c_int * B)(*bad)
        rc = L.LSTMApplyDeviceVarLen(lay.layer.h, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), B, arr, nul, nul, nul, nul)
        assert rc == -1 and b"outside" in L.nntk_last_error()
    rc = L.LSTMApplyDeviceVarLen(lay.layer.h, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), -1, None, nul, nul, nul, nul)
    assert rc == -1 and b"batch" in L.nntk_last_error()
    arr = (C.c_int * B)(0, 1, -1, 2, 3)
    cfg = capi.RecurrentConfig(I, H, True, T)
    assert L.bd_reverse_input_batch_varlen_device(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), cfg, B, arr) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    lay.destroy()


@pytest.mark.parametrize("kind,I,H,acts,opts,family", [CASES[0], CASES[1], CASES[4], CASES[5], CASES[6], CASES[11]],
                         ids=["gru-rr", "lstm-rr", "lstm-fk", "gru-acts", "lstm-H72", "rnn-step"])
def test_host_forms_equal_device_forms(gpu, kind, I, H, acts, opts, family):
    import torch
    set_options(opts)
    L = capi.load()
    B, T = 67, 7
    r = np.random.default_rng(5 * H)
    lay = Layer(kind, I, H, acts, T, True)
    xs, h0s, c0s = u(r, B, T, I), u(r, B, H, sc=0.5), u(r, B, H, sc=0.5)
    lens = ragged_lengths(r, B, T)
    dout, dh, dc = run_vl(lay, torch.from_numpy(xs).cuda(), lens, torch.from_numpy(h0s).cuda(), torch.from_numpy(c0s).cuda())
    out, hT, cT = np.empty((B, T, H), np.float32), np.empty((B, H), np.float32), np.empty((B, H), np.float32)
    p = lambda a: a.ctypes.data_as(capi.fp)
    lp = lens.ctypes.data_as(capi.ip)
    if kind == "lstm":
        rc = L.LSTMApplyInferenceBatchVarLen(lay.layer.h, p(xs), p(out), B, lp, p(h0s), p(c0s), p(hT), p(cT))
        assert np.array_equal(cT, dc.cpu().numpy())
    elif kind == "gru":
        rc = L.GRUApplyInferenceBatchVarLen(lay.layer.h, p(xs), p(out), B, lp, p(h0s), p(hT))
    else:
        rc = L.RNNApplyInferenceBatchVarLen(lay.layer.h, p(xs), p(out), B, lp, p(h0s), p(hT))
    assert rc == 0, L.nntk_last_error()
    assert np.array_equal(out, dout.cpu().numpy())
    assert np.array_equal(hT, dh.cpu().numpy())
    lay.destroy()
