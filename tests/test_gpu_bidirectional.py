"""Bidirectional layers in one call: *BidirectionalApplyDevice / *BidirectionalApplyInferenceBatch.

The result must equal, bit for bit, the composed recipe built from the existing calls (bd_reverse_*[_varlen]_device, *ApplyDevice[VarLen]
twice, bd_reverse of the backward sequence output, bd_merge_*_device) on every route: the fused one (both directions in ONE launch of the
BD instantiations of gru_rr_kernel / lstm_rr_kernel / *_fk_kernel) and the composed one (everything those kernels do not take).
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from nntoolkitcore_amd import capi, layers as NL

pytestmark = pytest.mark.gpu

ATOL, RTOL = 1e-5, 1e-5      # the single-layer tolerance of tests/test_gpu_varlen.py


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


def set_options(opts):
    for k, v in opts.items():
        capi.set_option(k, v)


@pytest.fixture(autouse=True)
def _restore_rec_bd():
    """(the session's option reset predates rec_bd)"""
    yield
    if capi._lib is not None:
        capi.set_option("rec_bd", "auto")


# (kind, I, H, acts, options, kernel the call must report): the fused route on both hand-off protocols of the split-K family and on the
# full-K family; the composed route (its last launch is the backward direction's own call) for what those kernels do not take
CASES = [
    ("gru", 16, 128, None, {}, "gru_rr_kernel<4,1,bd>"),                     # pending-pattern hand-off
    ("lstm", 96, 256, None, {}, "lstm_rr_kernel<4,2,bd>"),                   # pending-pattern hand-off
    ("lstm", 128, 512, None, {}, "lstm_rr_kernel<8,2,bd>"),                  # flag protocol
    ("gru", 256, 256, None, {}, "gru_fk_kernel<16,16,4,bd>"),                # full-K
    ("lstm", 256, 256, None, {}, "lstm_fk_kernel<16,16,4,bd>"),
    ("gru", 12, 40, "nondefault", {}, "rec_persistent_kernel<3,GRU>"),      # composed: non-default activations
    ("lstm", 20, 72, None, {}, "rec_persistent_kernel<4,LSTM>"),            # composed: H % 16 != 0
    ("lstm", 16, 64, None, {"rec_rr": "0"}, "rec_persistent_kernel<4,LSTM>"),
    ("gru", 16, 128, None, {"rec_bd": "0"}, "gru_rr_kernel<4,1>"),           # composed on the register-resident kernels (A/B switch)
    ("rnn", 10, 48, None, {}, "rec_persistent_kernel<1,RNN>"),
]
IDS = ["gru-rr4", "lstm-rr4", "lstm-rr8-H512", "gru-fk", "lstm-fk", "gru-acts", "lstm-H72", "lstm-rr0", "gru-bd0", "rnn"]


class Layer:
    def __init__(self, kind, I, H, acts, T, seq, seed=0):
        L = capi.load()
        self.kind, self.I, self.H, self.T, self.seq = kind, I, H, T, seq
        r = np.random.default_rng(seed + 1000 * I + H)
        G = {"gru": 3, "lstm": 4, "rnn": 1}[kind]
        self.w = [u(r, I, G * H, sc=I ** -0.5), u(r, H, G * H, sc=H ** -0.5), u(r, G * H, sc=0.1), u(r, G * H, sc=0.1)]
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

    def oracle(self, x):
        """one sequence x [L, in] from zero state: (sequence output or final h, final h)"""
        kw = {} if self.oacts is None else {"acts": self.oacts}
        if self.kind == "gru":
            return O.gru(x, *self.w, return_sequences=self.seq, **kw)
        if self.kind == "lstm":
            out, h, _ = O.lstm(x, *self.w, return_sequences=self.seq, v2=True)
            return out, h
        return O.rnn(x, *self.w, return_sequences=self.seq, v2=True)

    def destroy(self):
        self.layer.destroy()


def composed(fwd, bwd, x, lens, merge):
    """the recipe from the existing calls"""
    xr = NL.bd_reverse_device(x, "input", lens)
    if lens is None:
        of, obr = fwd.layer.apply_device(x), bwd.layer.apply_device(xr)
    else:
        of, obr = fwd.layer.apply_device_varlen(x, lengths=lens), bwd.layer.apply_device_varlen(xr, lengths=lens)
    ob = NL.bd_reverse_device(obr, "backward", lens) if fwd.seq else obr
    return NL.bd_merge_device(of, ob, merge)


def oracle_bd(fwd, bwd, xs, lens, merge):
    B, T = xs.shape[:2]
    H = fwd.H
    W = 2 * H if merge == "concat" else H
    out = np.zeros((B, T, W) if fwd.seq else (B, W), np.float32)
    for b in range(B):
        L = T if lens is None else int(lens[b])
        if L == 0:
            continue
        xb = xs[b:b + 1, :L]
        of, hf = fwd.oracle(xb[0])
        ob, hb = bwd.oracle(O.bd_reverse(xb)[0])
        if fwd.seq:
            out[b, :L] = O.bd_merge(of[None], O.bd_reverse(ob[None]), merge)[0]
        else:
            out[b] = O.bd_merge(hf[None, None], hb[None, None], merge)[0, 0]
    return out


@pytest.mark.parametrize("kind,I,H,acts,opts,family", CASES, ids=IDS)
@pytest.mark.parametrize("seq", [True, False], ids=["seq", "final"])
@pytest.mark.parametrize("merge", ["concat", "sum"])
@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
def test_bidirectional_route_table(gpu, kind, I, H, acts, opts, family, seq, merge, ragged):
    import torch
    set_options(opts)
    B, T = 130, 9
    r = np.random.default_rng(H + 7 * I + seq)
    fwd = Layer(kind, I, H, acts, T, seq, seed=1)
    bwd = Layer(kind, I, H, acts, T, seq, seed=2)
    xs = u(r, B, T, I)
    lens = ragged_lengths(r, B, T) if ragged else None
    x = torch.from_numpy(xs).cuda()
    ref = composed(fwd, bwd, x, lens, merge)
    out = NL.bidirectional_apply_device(fwd.layer, bwd.layer, x, lengths=lens, merge=merge)
    torch.cuda.synchronize()
    assert last_kernel() == family
    assert torch.equal(out, ref), "fused and composed differ: max %.3e" % (out - ref).abs().max().item()
    got = out.cpu().numpy()
    close(got, oracle_bd(fwd, bwd, xs, lens, merge))
    if seq and lens is not None:
        for b in range(B):
            assert not got[b, int(lens[b]):].any(), "rows past the length must be exactly zero in both halves"
    fwd.destroy()
    bwd.destroy()


@pytest.mark.parametrize("B", [1, 63, 65])
@pytest.mark.parametrize("merge", ["concat", "sum"])
def test_batch_edges(gpu, B, merge):
    import torch
    T = 7
    r = np.random.default_rng(B)
    fwd, bwd = Layer("gru", 16, 128, None, T, True, seed=3), Layer("gru", 16, 128, None, T, True, seed=4)
    x = torch.from_numpy(u(r, B, T, 16)).cuda()
    for lens in (None, r.integers(0, T + 1, B).astype(np.int32)):
        ref = composed(fwd, bwd, x, lens, merge)
        out = NL.bidirectional_apply_device(fwd.layer, bwd.layer, x, lengths=lens, merge=merge)
        assert last_kernel() == "gru_rr_kernel<4,1,bd>"
        assert torch.equal(out, ref)
    fwd.destroy()
    bwd.destroy()


def test_three_launches_one_straddling_the_directions(gpu):
    """GRU 128 -> 256 at B = 1536: 2 x 24 virtual tiles of 16 workgroups, 16 tiles per launch on a 256-CU chip -> three launches, the second
    holding tiles of both directions"""
    import torch
    L = capi.load()
    B, T = 1536, 200
    r = np.random.default_rng(11)
    fwd, bwd = Layer("gru", 128, 256, None, T, True, seed=5), Layer("gru", 128, 256, None, T, True, seed=6)
    x = torch.from_numpy(u(r, B, T, 128, sc=0.5)).cuda()
    lens = r.integers(0, T + 1, B).astype(np.int32)
    ref = composed(fwd, bwd, x, lens, "concat")
    torch.cuda.synchronize()
    ms, launches, steps = C.c_double(), C.c_long(), C.c_long()
    L.nntk_hip_profile_enable(1)
    try:
        L.nntk_hip_profile_get(b"rec_step", C.byref(ms), C.byref(launches), C.byref(steps))      # (clears)
        out = NL.bidirectional_apply_device(fwd.layer, bwd.layer, x, lengths=lens)
        torch.cuda.synchronize()
        L.nntk_hip_profile_get(b"rec_step", C.byref(ms), C.byref(launches), C.byref(steps))
    finally:
        L.nntk_hip_profile_enable(0)
    assert last_kernel() == "gru_rr_kernel<4,2,bd>"
    if torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert launches.value == 3
    else:
        assert launches.value >= 1
    assert torch.equal(out, ref)
    fwd.destroy()
    bwd.destroy()


def test_concat_tile_past_32bit_offsets_takes_the_composed_route(gpu):
    """LSTM 128 -> 512 at T = 8193, B = 64: a 64-row tile of one direction's rows (64 T H floats) fits the kernels' 32-bit buffer offsets, a
    tile of the concat merge's 2H-wide rows does not.  The concat call must run the composed route (its high rows would otherwise fall
    outside the output descriptor and keep what the buffer held); the sum merge, H wide, still runs fused.  Both equal the recipe."""
    import torch
    B, T = 64, 8193
    r = np.random.default_rng(19)
    fwd, bwd = Layer("lstm", 128, 512, None, T, True, seed=14), Layer("lstm", 128, 512, None, T, True, seed=15)
    x = torch.from_numpy(u(r, B, T, 128, sc=0.5)).cuda()
    lens = r.integers(T // 2, T + 1, B).astype(np.int32)
    lens[-8:] = T                                # the tile's high rows run every step
    for merge, family in (("concat", "lstm_rr_kernel<8,2>"), ("sum", "lstm_rr_kernel<8,2,bd>")):
        ref = composed(fwd, bwd, x, lens, merge)
        out = torch.full_like(ref, float("nan"))
        NL.bidirectional_apply_device(fwd.layer, bwd.layer, x, lengths=lens, merge=merge, out=out)
        torch.cuda.synchronize()
        assert last_kernel() == family
        assert torch.equal(out, ref)
        del ref, out
    fwd.destroy()
    bwd.destroy()


@pytest.mark.parametrize("kind,I,H,family", [("gru", 16, 128, "gru_rr_kernel<4,1,bd>"), ("lstm", 256, 256, "lstm_fk_kernel<16,16,4,bd>")])
def test_same_handle_both_directions(gpu, kind, I, H, family):
    import torch
    B, T = 70, 8
    r = np.random.default_rng(5)
    lay = Layer(kind, I, H, None, T, True, seed=7)
    x = torch.from_numpy(u(r, B, T, I)).cuda()
    lens = ragged_lengths(r, B, T)
    for merge in ("concat", "sum"):
        ref = composed(lay, lay, x, lens, merge)
        out = NL.bidirectional_apply_device(lay.layer, lay.layer, x, lengths=lens, merge=merge)
        assert last_kernel() == family
        assert torch.equal(out, ref)
    lay.destroy()


def test_errors_leave_the_output_untouched(gpu):
    import torch
    L = capi.load()
    B, T, I, H = 4, 5, 16, 64
    g1, g2 = NL.GRU(I, H, True, T), NL.GRU(I, H, True, T)
    other_T, other_H, other_seq = NL.GRU(I, H, True, T + 1), NL.GRU(I, H + 16, True, T), NL.GRU(I, H, False, T)
    other_in = NL.GRU(I + 1, H, True, T)
    x = torch.zeros(B, T, I, device="cuda")
    out = torch.full((B, T, 2 * H), 7.25, device="cuda")
    lens = np.array([1, 2, 3, 4], np.int32)
    lp = lens.ctypes.data_as(capi.ip)

    def call(f, b, xp, op, batch, lp_, merge):
        rc = L.GRUBidirectionalApplyDevice(f.h, b.h, xp, op, batch, lp_, merge)
        torch.cuda.synchronize()
        assert rc == -1
        assert capi.last_error()
        assert (out == 7.25).all(), "the output must be left untouched"

    xp, op = NL._dp(x), NL._dp(out)
    for bad in (other_T, other_H, other_seq, other_in):
        call(g1, bad, xp, op, B, lp, 0)
    for bad_len in ([1, 2, 3, T + 1], [1, -1, 3, 4]):
        bl = np.array(bad_len, np.int32)
        call(g1, g2, xp, op, B, bl.ctypes.data_as(capi.ip), 0)
    call(g1, g2, xp, op, B, lp, 2)
    call(g1, g2, xp, op, -1, lp, 0)
    call(g1, g2, xp, C.c_void_p(x.data_ptr() + 64), B, None, 0)          # the output overlaps the input
    assert not x.any()
    # the host form checks the same things
    xs, os_ = np.zeros((B, T, I), np.float32), np.full((B, T, 2 * H), 7.25, np.float32)
    assert L.GRUBidirectionalApplyInferenceBatch(g1.h, other_T.h, NL._p(xs), NL._p(os_), B, lp, 0) == -1 and capi.last_error()
    assert L.GRUBidirectionalApplyInferenceBatch(g1.h, g2.h, NL._p(xs), NL._p(os_), B, lp, 5) == -1
    assert (os_ == 7.25).all()
    for lay in (g1, g2, other_T, other_H, other_seq, other_in):
        lay.destroy()


@pytest.mark.parametrize("kind,I,H,family", [("gru", 16, 128, "gru_rr_kernel<4,1,bd>"), ("lstm", 96, 256, "lstm_rr_kernel<4,2,bd>")])
def test_sync_weights_reaches_the_backward_direction(gpu, kind, I, H, family):
    """a host edit of the backward handle's weights reaches the fused call after *SyncWeights, not before (the device-call contract)"""
    import torch
    B, T = 40, 6
    r = np.random.default_rng(9)
    fwd, bwd = Layer(kind, I, H, None, T, True, seed=8), Layer(kind, I, H, None, T, True, seed=9)
    x = torch.from_numpy(u(r, B, T, I)).cuda()
    before = NL.bidirectional_apply_device(fwd.layer, bwd.layer, x).clone()
    new_w = [w * np.float32(0.5) for w in bwd.w]
    bwd.layer.set_weights(*new_w)
    stale = NL.bidirectional_apply_device(fwd.layer, bwd.layer, x)
    assert last_kernel() == family
    assert torch.equal(stale, before), "without SyncWeights the call keeps the uploaded weights"
    bwd.layer.sync_weights()
    bwd.w = new_w
    synced = NL.bidirectional_apply_device(fwd.layer, bwd.layer, x)
    assert not torch.equal(synced[..., H:], before[..., H:])
    assert torch.equal(synced[..., :H], before[..., :H])
    assert torch.equal(synced, composed(fwd, bwd, x, None, "concat"))
    close(synced.cpu().numpy(), oracle_bd(fwd, bwd, x.cpu().numpy(), None, "concat"))
    fwd.destroy()
    bwd.destroy()


@pytest.mark.parametrize("kind,I,H", [("gru", 16, 128), ("lstm", 128, 512), ("gru", 256, 256)])
def test_alternating_inputs_leak_nothing(gpu, kind, I, H):
    import torch
    B, T = 100, 10
    r = np.random.default_rng(13)
    fwd, bwd = Layer(kind, I, H, None, T, True, seed=10), Layer(kind, I, H, None, T, True, seed=11)
    xa, xb = (torch.from_numpy(u(r, B, T, I)).cuda() for _ in range(2))
    la, lb = ragged_lengths(r, B, T), np.full(B, T, np.int32)
    out = torch.empty(B, T, 2 * H, device="cuda")
    first = {}
    for i in range(4):
        x, lens = (xa, la) if i % 2 == 0 else (xb, lb)
        NL.bidirectional_apply_device(fwd.layer, bwd.layer, x, lengths=lens, out=out)
        res = out.clone()
        if i < 2:
            first[i % 2] = res
        else:
            assert torch.equal(res, first[i % 2])
    assert not torch.equal(first[0], first[1])
    fwd.destroy()
    bwd.destroy()


@pytest.mark.parametrize("kind,I,H", [("gru", 16, 128), ("lstm", 20, 72), ("rnn", 10, 48)])
def test_host_form_equals_device_form(gpu, kind, I, H):
    import torch
    B, T = 66, 7
    r = np.random.default_rng(17)
    for seq in (True, False):
        fwd, bwd = Layer(kind, I, H, None, T, seq, seed=12), Layer(kind, I, H, None, T, seq, seed=13)
        xs = u(r, B, T, I)
        lens = ragged_lengths(r, B, T)
        for merge in ("concat", "sum"):
            dev = NL.bidirectional_apply_device(fwd.layer, bwd.layer, torch.from_numpy(xs).cuda(), lengths=lens, merge=merge)
            host = NL.bidirectional_apply(fwd.layer, bwd.layer, xs, lengths=lens, merge=merge)
            assert np.array_equal(host, dev.cpu().numpy())
            close(host, oracle_bd(fwd, bwd, xs, lens, merge))
        fwd.destroy()
        bwd.destroy()
