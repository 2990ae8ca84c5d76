"""Training on ragged batches with carried state (the *ApplyTrainingBatch*VarLen / *CalculateGradient*VarLen calls) through the C
boundary: per-row lengths, h0 / c0 in, hT / cT out, d_hT / d_cT in, d_h0 / d_c0 out -- what truncated back-propagation through time
needs.  References: the existing fixed-length calls (bits), the oracle row by row, and a masked torch float64 loop with autograd.

Tolerances are the project's own (tests/test_gpu_training.py): forward rtol 2e-5 / atol 2e-6, gradients 2e-7 sqrt(B T) max(1, |ref|max),
persistent against per-step BPTT 2e-5 max(1, |ref|max)."""
import ctypes as C

import numpy as np
import pytest

from nntoolkitcore_amd import capi
import oracle as O

pytestmark = pytest.mark.gpu
P = lambda a: None if a is None else a.ctypes.data_as(capi.fp)
IP = lambda a: None if a is None else a.ctypes.data_as(capi.ip)
NG = {"gru": 3, "lstm": 4, "rnn": 1}
DEFAULT = {"gru": ("sigmoid", "tanh", "sigmoid"),                       # z, h, r
           "lstm": ("sigmoid", "sigmoid", "tanh", "sigmoid", "tanh"),   # i, f, g, o, out
           "rnn": ("tanh",)}
CREATE = {"sigmoid": "ActivationFunctionCreateSigmoid", "tanh": "ActivationFunctionCreateTanh", "identity": "ActivationFunctionCreateIdentity"}
KIND = {"sigmoid": O.ACT_SIGMOID, "tanh": O.ACT_TANH, "identity": O.ACT_IDENTITY}


def u(r, *shape, sc=1.0):
    return r.uniform(-sc, sc, shape).astype(np.float32)


class Net:
    """one training handle with fixed random weights; forward / backward through the host-memory VarLen forms"""

    def __init__(self, kind, B, T, n_in, H, seq, seed=1, acts=None, v2=True):
        L = self.L = capi.load()
        self.kind, self.B, self.T, self.n_in, self.H, self.seq, self.v2 = kind, B, T, n_in, H, seq, v2
        self.acts = acts or DEFAULT[kind]
        g = NG[kind]
        r = np.random.default_rng(seed)
        self.W, self.U = u(r, n_in, g * H, sc=n_in ** -0.5), u(r, H, g * H, sc=H ** -0.5)
        self.bi, self.bh = u(r, g * H, sc=0.1), u(r, g * H, sc=0.1)
        self.ah = [getattr(L, CREATE[a])(H) for a in self.acts]
        self.tc = capi.ConvTrainingConfig(B)
        if kind == "gru":
            self.cfg = L.GRUConfigCreate(n_in, H, seq, T, L.GRUActivationsCreate(self.ah[0], self.ah[1], self.ah[2]))
        elif kind == "lstm":
            self.cfg = L.LSTMConfigCreate(n_in, H, seq, T, v2, L.LSTMActivationsCreate(*self.ah))
        else:
            self.cfg = L.RNNConfigCreate(n_in, H, seq, T, v2, self.ah[0])
        self.pre = kind.upper()
        self.h = self.f("CreateForTraining")(self.cfg, self.tc)
        w = self.f("GetWeights")(self.h).contents
        for dst, src in ((w.W, self.W), (w.U, self.U), (w.b_i, self.bi), (w.b_h, self.bh)):
            C.memmove(dst, src.ctypes.data, src.nbytes)
        self.out_shape = (B, T, H) if seq else (B, H)
        self.nblk = self.W.size + self.U.size + 2 * g * H

    def f(self, name):
        return getattr(self.L, self.pre + name)

    def forward(self, x, lengths=None, h0=None, c0=None):
        y = np.full(self.out_shape, 7.0, np.float32)
        hT, cT = np.full((self.B, self.H), 7.0, np.float32), np.full((self.B, self.H), 7.0, np.float32)
        if self.kind == "lstm":
            rc = self.f("ApplyTrainingBatchVarLen")(self.h, P(x), P(y), IP(lengths), P(h0), P(c0), P(hT), P(cT))
        else:
            rc = self.f("ApplyTrainingBatchVarLen")(self.h, P(x), P(y), IP(lengths), P(h0), P(hT))
            cT = None
        assert rc == 0, capi.last_error()
        return y, hT, cT

    def backward(self, dout, dhT=None, dcT=None, block=None):
        """(dW, dU, dbi, dbh, dX, dh0, dc0); block: an existing gradient block to accumulate onto"""
        g = block or self.f("GradientCreate")(self.cfg, self.tc)
        dh0, dc0 = np.full((self.B, self.H), 7.0, np.float32), np.full((self.B, self.H), 7.0, np.float32)
        if self.kind == "lstm":
            rc = self.f("CalculateGradientVarLen")(self.h, g, P(dout), P(dhT), P(dcT), P(dh0), P(dc0))
        else:
            rc = self.f("CalculateGradientVarLen")(self.h, g, P(dout), P(dhT), P(dh0))
            dc0 = None
        assert rc == 0, capi.last_error()
        gc = g.contents
        got = [np.ctypeslib.as_array(p_, shape=s).copy() for p_, s in ((gc.d_W, self.W.shape), (gc.d_U, self.U.shape), (gc.d_b_i, self.bi.shape),
                                                                       (gc.d_b_h, self.bh.shape), (gc.d_X, (self.B, self.T, self.n_in)))]
        if block is None:
            self.L.RecurrentGradientDestroy(g)
        return got + [dh0, dc0]

    def last_kernel(self):
        """the recurrent kernel the last call ran (the route)"""
        return self.L.nntk_hip_last_recurrent_kernel().decode()

    def close(self):
        self.f("Destroy")(self.h)
        for a in self.ah:
            self.L.ActivationFunctionDestroy(a)


def lengths_for(B, T, seed):
    """0, 1, T, a 16-row tile whose rows are all shorter than T (mini-batches above 16), the rest a random draw"""
    r = np.random.default_rng(seed)
    ln = r.integers(0, T + 1, B).astype(np.int32)
    ln[:3] = (T, 0, 1)
    if B > 16:
        ln[16:32] = r.integers(0, T, min(16, B - 16))
    if B > 3:
        ln[3] = T
    return ln


def ref64(net, x, lengths, h0, c0, dout, dhT, dcT):
    """masked float64 loop over the cell with autograd: (out, hT, cT), (dW, dU, dbi, dbh, dX, dh0, dc0)"""
    import torch
    B, T, H, kind = net.B, net.T, net.H, net.kind
    fn = {"sigmoid": torch.sigmoid, "tanh": torch.tanh, "identity": lambda v: v}
    a = [fn[n] for n in net.acts]
    ln = torch.tensor(np.full(B, T) if lengths is None else lengths)
    msk = (torch.arange(T)[None, :] < ln[:, None])
    xz = np.where(msk.numpy()[:, :, None], x, 0.0)
    leaf = lambda v, shape: torch.tensor(np.zeros(shape) if v is None else v).double().requires_grad_(True)
    xt, Wt, Ut, bit, bht = (leaf(v, None) for v in (xz, net.W, net.U, net.bi, net.bh))
    h0t, c0t = leaf(h0, (B, H)), leaf(c0, (B, H))
    hp, cp, outs = h0t, c0t, []
    for t in range(T):
        m = msk[:, t:t + 1]
        xw = xt[:, t] @ Wt + bit
        if kind == "gru":
            hu = hp @ Ut + bht
            z, rr = a[0](xw[:, :H] + hu[:, :H]), a[2](xw[:, H:2 * H] + hu[:, H:2 * H])
            hn = (1 - z) * a[1](rr * hu[:, 2 * H:] + xw[:, 2 * H:]) + z * hp
        elif kind == "lstm":
            Z = xw + hp @ Ut + (bht if net.v2 else 0)
            i, f, g_, o = a[0](Z[:, :H]), a[1](Z[:, H:2 * H]), a[2](Z[:, 2 * H:3 * H]), a[3](Z[:, 3 * H:])
            cn = f * cp + i * g_
            hn = o * a[4](cn)
            cp = torch.where(m, cn, cp)
        else:
            hn = a[0](xw + hp @ Ut + (bht if net.v2 else 0))
        hp = torch.where(m, hn, hp)
        outs.append(torch.where(m, hn, torch.zeros_like(hn)))
    hh = torch.stack(outs, 1)
    if net.seq:
        loss = (hh * torch.tensor(np.where(msk.numpy()[:, :, None], dout, 0.0)).double()).sum()
    else:
        loss = (hp * torch.tensor(dout).double()).sum()
    if dhT is not None:
        loss = loss + (hp * torch.tensor(dhT).double()).sum()
    if dcT is not None and kind == "lstm":
        loss = loss + (cp * torch.tensor(dcT).double()).sum()
    loss = loss + 0.0 * (h0t.sum() + c0t.sum() + bht.sum())            # every leaf gets a gradient
    loss.backward()
    dbh = bht.grad.numpy() if (kind == "gru" or net.v2) else bit.grad.numpy()      # without v2 the reference still reports d_b_h = d_gates
    grads = [Wt.grad.numpy(), Ut.grad.numpy(), bit.grad.numpy(), dbh, xt.grad.numpy(), h0t.grad.numpy(), c0t.grad.numpy() if kind == "lstm" else None]
    out = hh.detach().numpy() if net.seq else hp.detach().numpy()
    return (out, hp.detach().numpy(), cp.detach().numpy() if kind == "lstm" else None), grads


PARTS = ("dW", "dU", "dbi", "dbh", "dX", "dh0", "dc0")


def check_grads(tag, got, ref, tol):
    for part, a, b_ in zip(PARTS, got, ref):
        if a is None or b_ is None:
            continue
        sc = max(1.0, float(np.abs(b_).max()))
        err = float(np.abs(a - b_).max())
        print("%s %s: %.2e (scale %.1f, bound %.2e)" % (tag, part, err, sc, tol * sc))
        assert np.isfinite(a).all() and err <= tol * sc, (tag, part, err, tol * sc)


# kind, B, T, in, H, return_sequences, v2, non-default activations, train_bptt.  Routes: mini-batch < 32 and >= 32 (not multiples of 16),
# default activations (persistent BPTT), a non-default gate activation, train_bptt = 0, H not a multiple of 16 (per-step BPTT), in > 128
SHAPES = [
    ("gru", 20, 9, 16, 64, True, True, None, "auto"),
    ("gru", 37, 12, 40, 64, False, True, None, "auto"),
    ("gru", 5, 7, 6, 12, True, True, None, "auto"),
    ("gru", 18, 8, 10, 32, True, True, ("sigmoid", "tanh", "tanh"), "auto"),
    ("gru", 33, 6, 200, 32, True, True, None, "auto"),
    ("gru", 21, 10, 16, 32, True, True, None, 0),
    ("lstm", 20, 9, 16, 64, True, True, None, "auto"),
    ("lstm", 37, 12, 40, 64, False, False, None, "auto"),
    ("lstm", 5, 7, 6, 12, True, True, None, "auto"),
    ("lstm", 18, 8, 10, 32, False, True, ("sigmoid", "sigmoid", "tanh", "sigmoid", "sigmoid"), "auto"),
    ("lstm", 33, 6, 200, 32, True, True, None, "auto"),
    ("lstm", 21, 10, 16, 32, True, False, None, 0),
    ("rnn", 20, 9, 16, 64, True, True, None, "auto"),
    ("rnn", 37, 12, 40, 24, False, False, ("sigmoid",), "auto"),
    ("rnn", 5, 7, 6, 12, True, True, None, "auto"),
    ("rnn", 33, 6, 200, 32, True, True, None, "auto"),
]
IDS = ["%s-B%d-T%d-in%d-H%d-%s%s%s%s" % (k, B, T, i, H, "seq" if s else "last", "" if v else "-v1", "-acts" if a else "", "-perstep" if o == 0 else "")
       for k, B, T, i, H, s, v, a, o in SHAPES]


@pytest.fixture
def bptt_option():
    yield lambda v: capi.set_option("train_bptt", v)
    capi.set_option("train_bptt", "auto")


def _data(net, seed, states=True):
    r = np.random.default_rng(seed)
    x, dout = u(r, net.B, net.T, net.n_in), u(r, *net.out_shape)
    st = [u(r, net.B, net.H, sc=0.5) for _ in range(4)]
    if not states:
        st = [None] * 4
    h0, c0, dhT, dcT = st
    if net.kind != "lstm":
        c0 = dcT = None
    return x, dout, h0, c0, dhT, dcT


@pytest.mark.parametrize("kind,B,T,n_in,H,seq,v2,acts,bptt", SHAPES, ids=IDS)
def test_unused_varlen_arguments_change_no_bit(gpu, bptt_option, kind, B, T, n_in, H, seq, v2, acts, bptt):
    """lengths = NULL and no states: output, d_X and the accumulated gradient block equal the existing device calls on a twin handle bit
    for bit; the host forms equal the device forms."""
    import torch
    bptt_option(bptt)
    L = capi.load()
    a, b = Net(kind, B, T, n_in, H, seq, 3, acts, v2), Net(kind, B, T, n_in, H, seq, 3, acts, v2)
    x, dout, *_ = _data(a, 11, states=False)
    dp = lambda t: C.c_void_p(t.data_ptr())
    xd, dd = torch.from_numpy(x).cuda(), torch.from_numpy(dout).cuda()
    res = []
    for net, new in ((a, False), (b, True)):
        yd, gx = torch.full(net.out_shape, 7.0, device="cuda"), torch.full((B, T, n_in), 7.0, device="cuda")
        gd = torch.full((net.nblk,), 0.25, device="cuda")                # ADDED to: start from a non-zero block
        if not new:
            assert net.f("ApplyTrainingBatchDevice")(net.h, dp(xd), dp(yd)) == 0, capi.last_error()
            assert net.f("CalculateGradientDevice")(net.h, dp(gd), dp(gx), dp(dd)) == 0, capi.last_error()
        elif kind == "lstm":
            assert L.LSTMApplyTrainingBatchDeviceVarLen(net.h, dp(xd), dp(yd), None, None, None, None, None) == 0, capi.last_error()
            assert L.LSTMCalculateGradientDeviceVarLen(net.h, dp(gd), dp(gx), dp(dd), None, None, None, None) == 0, capi.last_error()
        else:
            assert net.f("ApplyTrainingBatchDeviceVarLen")(net.h, dp(xd), dp(yd), None, None, None) == 0, capi.last_error()
            assert net.f("CalculateGradientDeviceVarLen")(net.h, dp(gd), dp(gx), dp(dd), None, None) == 0, capi.last_error()
        assert L.nntk_hip_synchronize() == 0
        res.append([t.cpu().numpy() for t in (yd, gx, gd)])
    for nm, p_, q_ in zip(("out", "dX", "grad block"), *res):
        assert np.isfinite(p_).all()
        np.testing.assert_array_equal(p_, q_, err_msg=nm)
    # host forms: the same bits (their block starts from zeros: a device block that does so too)
    gd, gx = torch.zeros(b.nblk, device="cuda"), torch.empty(B, T, n_in, device="cuda")
    if kind == "lstm":
        assert L.LSTMCalculateGradientDeviceVarLen(b.h, dp(gd), dp(gx), dp(dd), None, None, None, None) == 0, capi.last_error()
    else:
        assert b.f("CalculateGradientDeviceVarLen")(b.h, dp(gd), dp(gx), dp(dd), None, None) == 0, capi.last_error()
    assert L.nntk_hip_synchronize() == 0
    y, _, _ = b.forward(x)
    got = b.backward(dout)
    np.testing.assert_array_equal(y, res[1][0])
    np.testing.assert_array_equal(got[4], res[1][1])
    np.testing.assert_array_equal(np.concatenate([g.ravel() for g in got[:4]]), gd.cpu().numpy())
    if kind == "rnn":                                                    # the RNN's plain device forms are new as well: against its host forms
        yh = np.empty(a.out_shape, np.float32)
        assert L.RNNApplyTrainingBatch(a.h, P(x), P(yh)) == 0
        g = L.RNNGradientCreate(a.cfg, a.tc)
        L.RNNCalculateGradient(a.h, g, P(dout))
        assert capi.last_error() == ""
        np.testing.assert_array_equal(yh, res[0][0])
        np.testing.assert_array_equal(np.ctypeslib.as_array(g.contents.d_X, shape=x.shape), res[0][1])
        np.testing.assert_array_equal(np.ctypeslib.as_array(g.contents.d_W, shape=(a.W.size,)), got[0].ravel())
        L.RecurrentGradientDestroy(g)
    a.close(); b.close()


@pytest.mark.parametrize("kind,B,T,n_in,H,seq,v2,acts,bptt", SHAPES, ids=IDS)
def test_padding_cannot_leak(gpu, bptt_option, kind, B, T, n_in, H, seq, v2, acts, bptt):
    """x[b][t >= L] and d_dout[b][t >= L] zero against NaN: every output is equal bit for bit and finite; out and d_X past a row's length
    are exact zeros."""
    bptt_option(bptt)
    net = Net(kind, B, T, n_in, H, seq, 5, acts, v2)
    x, dout, h0, c0, dhT, dcT = _data(net, 21)
    ln = lengths_for(B, T, 7)
    pad = np.arange(T)[None, :] >= ln[:, None]
    runs = []
    for fill in (0.0, np.nan):
        xf, df = x.copy(), dout.copy()
        xf[pad] = fill
        if seq:
            df[pad] = fill
        y, hT, cT = net.forward(xf, ln, h0, c0)
        runs.append([y, hT, cT] + net.backward(df, dhT, dcT))
    for nm, p_, q_ in zip(("out", "hT", "cT") + PARTS, *runs):
        if p_ is None:
            continue
        assert np.isfinite(q_).all(), nm
        np.testing.assert_array_equal(p_, q_, err_msg=nm)
    if seq:
        assert not runs[1][0][pad].any()
    assert not runs[1][7][pad].any()
    net.close()


@pytest.mark.parametrize("kind,B,T,n_in,H,seq,v2,acts,bptt", SHAPES, ids=IDS)
def test_rows_match_the_oracle(gpu, bptt_option, kind, B, T, n_in, H, seq, v2, acts, bptt):
    """zero state: every row equals the oracle's training pass on x[b, :L] with d_dout[b, :L]; weight gradients summed over rows in float64"""
    bptt_option(bptt)
    net = Net(kind, B, T, n_in, H, seq, 6, acts, v2)
    x, dout, *_ = _data(net, 31, states=False)
    ln = lengths_for(B, T, 8)
    y, hT, cT = net.forward(x, ln)
    got = net.backward(dout)
    kinds = tuple(KIND[a] for a in net.acts)
    ref_y, ref_hT = np.zeros_like(y), np.zeros_like(hT)
    ref = [np.zeros(s, np.float64) for s in (net.W.shape, net.U.shape, net.bi.shape, net.bh.shape, x.shape)]
    for b in range(B):
        n = int(ln[b])
        if n == 0:
            continue
        d = dout[b:b + 1, :n] if seq else dout[b:b + 1]
        if kind == "gru":
            o_h, g = O.gru_training(x[b:b + 1, :n], net.W, net.U, net.bi, net.bh, d, return_sequences=seq, acts=kinds)
        elif kind == "lstm":
            o_h, g = O.lstm_training(x[b:b + 1, :n], net.W, net.U, net.bi, net.bh, d, return_sequences=seq, v2=v2, acts=kinds)
        else:
            o_h, g = O.rnn_training(x[b:b + 1, :n], net.W, net.U, net.bi, net.bh, d, return_sequences=seq, v2=v2, act=kinds[0])
        if seq:
            ref_y[b, :n] = o_h[0]
        else:
            ref_y[b] = o_h[0, -1]
        ref_hT[b] = o_h[0, -1]
        for acc, part in zip(ref[:4], g[:4]):
            acc += part
        ref[4][b, :n] = g[4][0]
    np.testing.assert_allclose(y, ref_y, rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(hT, ref_hT, rtol=2e-5, atol=2e-6)
    check_grads("%s vs oracle rows" % kind, got[:5], ref, 2e-7 * np.sqrt(B * T))
    net.close()


@pytest.mark.parametrize("kind,B,T,n_in,H,seq,v2,acts,bptt", SHAPES, ids=IDS)
def test_everything_on_matches_float64_autograd(gpu, bptt_option, kind, B, T, n_in, H, seq, v2, acts, bptt):
    """ragged rows, random h0 / c0, random d_hT / d_cT: all of d_W, d_U, d_b_i, d_b_h, d_X, d_h0, d_c0 against torch float64 autograd
    within the project's gradient tolerance (d_h0 / d_c0 included: their achieved error is printed next to the bound; measured on
    MI355X: d_h0 <= 1.9e-7, d_c0 <= 9.5e-8 at scales 1.0-1.5 against bounds of 1.2e-6 and up -- the existing bound holds unchanged)"""
    bptt_option(bptt)
    net = Net(kind, B, T, n_in, H, seq, 9, acts, v2)
    x, dout, h0, c0, dhT, dcT = _data(net, 41)
    ln = lengths_for(B, T, 9)
    y, hT, cT = net.forward(x, ln, h0, c0)
    got = net.backward(dout, dhT, dcT)
    (r_y, r_hT, r_cT), ref = ref64(net, x, ln, h0, c0, dout, dhT, dcT)
    np.testing.assert_allclose(y, r_y, rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(hT, r_hT, rtol=2e-5, atol=2e-6)
    if kind == "lstm":
        np.testing.assert_allclose(cT, r_cT, rtol=2e-5, atol=2e-6)
    check_grads("%s vs torch float64" % kind, got, ref, 2e-7 * np.sqrt(B * T))
    # the states alone, lengths NULL
    y, hT, cT = net.forward(x, None, h0, c0)
    got = net.backward(dout, dhT, dcT)
    (r_y, r_hT, r_cT), ref = ref64(net, x, None, h0, c0, dout, dhT, dcT)
    np.testing.assert_allclose(y, r_y, rtol=2e-5, atol=2e-6)
    check_grads("%s vs torch float64, full rows" % kind, got, ref, 2e-7 * np.sqrt(B * T))
    net.close()


@pytest.mark.parametrize("kind,B,Tc,k,n_in,H,v2", [("gru", 20, 6, 3, 16, 64, True), ("lstm", 37, 5, 4, 24, 32, True), ("lstm", 20, 6, 3, 16, 64, False),
                                                 ("rnn", 18, 7, 3, 12, 24, True), ("gru", 40, 8, 3, 40, 128, True)])
def test_truncated_bptt_closes(gpu, kind, B, Tc, k, n_in, H, v2):
    """k chunks on a timesteps = Tc handle -- state carried forward, d_h0 -> d_hT (d_c0 -> d_cT) carried backward, the weight gradients
    accumulated in one block -- against the EXISTING one-shot training calls on a timesteps = k Tc handle; then ragged rows (a row ends
    inside some chunk, later chunks see length 0 for it) against the float64 loop."""
    T = k * Tc
    L = capi.load()
    full, chunk = Net(kind, B, T, n_in, H, True, 12, None, v2), Net(kind, B, Tc, n_in, H, True, 12, None, v2)
    x, dout, *_ = _data(full, 51, states=False)
    tol = 2e-7 * np.sqrt(B * T)

    def run_chunks(ln):
        h, c, ys, h0s = None, None, [], []
        lens = [None if ln is None else np.clip(ln - j * Tc, 0, Tc).astype(np.int32) for j in range(k)]
        # the backward pass needs each chunk's forward caches, which a handle keeps for ONE mini-batch: forward again, chunk by chunk
        for j in range(k):
            h0s.append((h, c))
            y, h, c = chunk.forward(np.ascontiguousarray(x[:, j * Tc:(j + 1) * Tc]), lens[j], h, c)
            ys.append(y)
        blk = chunk.f("GradientCreate")(chunk.cfg, chunk.tc)
        dh, dc, dX = None, None, np.empty_like(x)
        for j in reversed(range(k)):
            chunk.forward(np.ascontiguousarray(x[:, j * Tc:(j + 1) * Tc]), lens[j], *h0s[j])
            got = chunk.backward(np.ascontiguousarray(dout[:, j * Tc:(j + 1) * Tc]), dh, dc, block=blk)
            dX[:, j * Tc:(j + 1) * Tc], dh, dc = got[4], got[5], got[6]
        L.RecurrentGradientDestroy(blk)
        return np.concatenate(ys, 1), got[:4] + [dX, dh, dc]

    y1 = np.empty(full.out_shape, np.float32)
    assert full.f("ApplyTrainingBatch")(full.h, P(x), P(y1)) == 0, capi.last_error()
    g = full.f("GradientCreate")(full.cfg, full.tc)
    full.f("CalculateGradient")(full.h, g, P(dout))
    assert capi.last_error() == ""
    gc = g.contents
    one = [np.ctypeslib.as_array(p_, shape=s).copy() for p_, s in ((gc.d_W, full.W.shape), (gc.d_U, full.U.shape), (gc.d_b_i, full.bi.shape),
                                                                   (gc.d_b_h, full.bh.shape), (gc.d_X, x.shape))]
    L.RecurrentGradientDestroy(g)
    yk, gk = run_chunks(None)
    np.testing.assert_allclose(yk, y1, rtol=2e-5, atol=2e-6)
    check_grads("%s chunks vs one shot" % kind, gk[:5], one, tol)
    ln = lengths_for(B, T, 13)
    yk, gk = run_chunks(ln)
    (r_y, _, _), ref = ref64(full, x, ln, None, None, dout, None, None)
    np.testing.assert_allclose(yk, r_y, rtol=2e-5, atol=2e-6)
    check_grads("%s ragged chunks vs torch float64" % kind, gk, ref, tol)
    full.close(); chunk.close()


@pytest.mark.parametrize("kind,B,T,n_in,H,seq", [("lstm", 64, 40, 128, 512, True), ("lstm", 37, 12, 40, 64, False), ("gru", 64, 40, 128, 256, True),
                                                 ("gru", 20, 9, 16, 64, False), ("gru", 33, 2, 24, 64, True)])
def test_persistent_bptt_equals_the_per_step_loop_on_ragged_batches(gpu, bptt_option, kind, B, T, n_in, H, seq):
    """the criterion of test_persistent_bptt_equals_the_per_step_loop (<= 2e-5 max(1, |ref|max) per gradient part) for the new calls: ragged
    batch, states in and gradients of the states out"""
    res = []
    for opt in ("auto", 0):
        bptt_option(opt)
        net = Net(kind, B, T, n_in, H, seq, 14)
        x, dout, h0, c0, dhT, dcT = _data(net, 61)
        ln = lengths_for(B, T, 15)
        net.forward(x, ln, h0, c0)
        res.append(net.backward(dout, dhT, dcT))
        # the two runs really are the two routes (the persistent kernel steps aside silently when it is not co-resident or after a fault)
        assert net.last_kernel() == ("bptt_persistent_kernel<%s>" % kind.upper() if opt == "auto" else "%s_train_bwd_step_kernel" % kind)
        net.close()
    for nm, p_, q_ in zip(PARTS, *res):
        if p_ is None:
            continue
        sc = max(1.0, float(np.abs(q_).max()))
        err = float(np.abs(p_ - q_).max())
        print("persistent vs per-step BPTT, ragged, %s %s: %.2e (scale %.1f)" % (kind, nm, err, sc))
        assert err <= 2e-5 * sc, (nm, err)


@pytest.mark.parametrize("seq", [True, False], ids=["seq", "last"])
@pytest.mark.parametrize("kind,B,T,n_in,H", [("gru", 17, 4, 8, 64), ("lstm", 17, 4, 8, 16)])
def test_a_rows_last_step_has_the_same_bits_on_both_bptt_routes(gpu, bptt_option, kind, B, T, n_in, H, seq):
    """The persistent kernel and the per-step loop run ONE backward cell (gru_cell_bwd / lstm_cell_bwd, train.hip) and differ only in
    the product that carries d_h back.  At a row's own last step nothing has been carried yet -- d_h is d_hT plus the output gradient --
    so the gate gradients there are the cell alone and the two routes agree bit for bit: d_h0 / d_c0 of the rows of length 1 (their
    last step is step 0), and d_X at every non-empty row's last step (d_xW W^T and d_hU U^T are per-row products at these sizes)."""
    ln = lengths_for(B, T, 19)
    assert {0, 1, T} <= set(ln.tolist())
    res = []
    for opt in ("auto", 0):
        bptt_option(opt)
        net = Net(kind, B, T, n_in, H, seq, 22)
        x, dout, h0, c0, dhT, dcT = _data(net, 91)
        net.forward(x, ln, h0, c0)
        res.append(net.backward(dout, dhT, dcT))
        # (the persistent kernel steps aside silently when it cannot run: the comparison must not be of the loop with itself)
        assert net.last_kernel() == ("bptt_persistent_kernel<%s>" % kind.upper() if opt == "auto" else "%s_train_bwd_step_kernel" % kind)
        net.close()
    one, rows = ln == 1, np.nonzero(ln > 0)[0]
    for nm in ("dh0", "dc0"):
        p_, q_ = (r[PARTS.index(nm)] for r in res)
        if p_ is not None:
            assert np.isfinite(p_).all()
            np.testing.assert_array_equal(p_[one], q_[one], err_msg=nm)
    np.testing.assert_array_equal(res[0][4][rows, ln[rows] - 1], res[1][4][rows, ln[rows] - 1], err_msg="dX at the last step")


@pytest.mark.parametrize("kind,B,T,n_in,H,seq,v2", [("gru", 37, 12, 104, 64, True, True), ("gru", 33, 6, 200, 64, False, True), ("gru", 64, 40, 128, 256, True, True),
                                                    ("gru", 130, 9, 72, 128, True, True), ("lstm", 37, 12, 40, 64, True, False),
                                                    ("lstm", 33, 6, 200, 64, False, True), ("lstm", 64, 40, 128, 512, True, True),
                                                    ("lstm", 130, 9, 64, 128, True, True), ("lstm", 20, 9, 16, 320, True, True)])
def test_ragged_calls_take_the_register_resident_forward_and_the_persistent_bptt(gpu, kind, B, T, n_in, H, seq, v2):
    """default activations at shapes the fixed-length call runs on gru_rr_kernel / lstm_rr_kernel<.., TRAIN> (every KH / KX instantiation: H up
    to 256 / above, in up to 64 / 128 / 256; more than one 64-row batch tile): the ragged, carried-state call runs the same kernel family
    (its TRAIN + VL instantiation) and the persistent BPTT kernel, and everything matches float64 autograd; padding as NaN.  (The one
    shape class without such an instantiation -- GRU, H <= 256, in <= 64: it would spill -- runs the per-timestep forward and is in SHAPES.)"""
    net = Net(kind, B, T, n_in, H, seq, 17, None, v2)
    x, dout, h0, c0, dhT, dcT = _data(net, 81)
    ln = lengths_for(B, T, 18)
    if B > 64:
        ln[64:128] = np.minimum(ln[64:128], T // 2)                      # a whole 64-row tile that stops early
    pad = np.arange(T)[None, :] >= ln[:, None]
    xf, df = x.copy(), dout.copy()
    xf[pad] = np.nan
    if seq:
        df[pad] = np.nan
    plain = np.empty(net.out_shape, np.float32)
    assert net.f("ApplyTrainingBatch")(net.h, P(x), P(plain)) == 0, capi.last_error()
    family = net.last_kernel().split("<")[0]
    assert family == kind + "_rr_kernel"                                 # what the fixed-length call runs here
    y, hT, cT = net.forward(xf, ln, h0, c0)
    assert net.last_kernel().split("<")[0] == family
    got = net.backward(df, dhT, dcT)
    assert net.last_kernel() == "bptt_persistent_kernel<%s>" % kind.upper()
    (r_y, r_hT, r_cT), ref = ref64(net, x, ln, h0, c0, dout, dhT, dcT)
    if seq:
        assert not y[pad].any()
    assert not got[4][pad].any()
    np.testing.assert_allclose(y, r_y, rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(hT, r_hT, rtol=2e-5, atol=2e-6)
    if kind == "lstm":
        np.testing.assert_allclose(cT, r_cT, rtol=2e-5, atol=2e-6)
    check_grads("%s rr forward + persistent bptt vs torch float64" % kind, got, ref, 2e-7 * np.sqrt(B * T))
    # a carried-in state alone (lengths NULL) stays on the family too
    y, hT, cT = net.forward(x, None, h0, c0)
    assert net.last_kernel().split("<")[0] == family
    got = net.backward(dout, dhT, dcT)
    (r_y, r_hT, r_cT), ref = ref64(net, x, None, h0, c0, dout, dhT, dcT)
    np.testing.assert_allclose(y, r_y, rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(hT, r_hT, rtol=2e-5, atol=2e-6)
    check_grads("%s rr forward, full rows, vs torch float64" % kind, got, ref, 2e-7 * np.sqrt(B * T))
    net.close()


@pytest.mark.parametrize("kind", ["gru", "lstm", "rnn"])
def test_argument_errors_write_nothing(gpu, kind):
    import torch
    L = capi.load()
    B, T, n_in, H = 6, 5, 4, 16
    net = Net(kind, B, T, n_in, H, True, 16)
    x, dout, *_ = _data(net, 71, states=False)
    dp = lambda t: C.c_void_p(t.data_ptr())
    xd, dd = torch.from_numpy(x).cuda(), torch.from_numpy(dout).cuda()
    yd, hT = torch.full((B, T, H), 7.0, device="cuda"), torch.full((B, H), 7.0, device="cuda")
    gd, gx, dh0 = torch.full((net.nblk,), 7.0, device="cuda"), torch.full((B, T, n_in), 7.0, device="cuda"), torch.full((B, H), 7.0, device="cuda")
    lstm = kind == "lstm"
    fwd = lambda h, ln: (net.f("ApplyTrainingBatchDeviceVarLen")(h, dp(xd), dp(yd), IP(ln), None, None, dp(hT), None) if lstm else
                         net.f("ApplyTrainingBatchDeviceVarLen")(h, dp(xd), dp(yd), IP(ln), None, dp(hT)))
    bwd = lambda h: (net.f("CalculateGradientDeviceVarLen")(h, dp(gd), dp(gx), dp(dd), None, None, dp(dh0), None) if lstm else
                     net.f("CalculateGradientDeviceVarLen")(h, dp(gd), dp(gx), dp(dd), None, dp(dh0)))
    untouched = lambda: L.nntk_hip_synchronize() == 0 and all(bool((t == 7.0).all()) for t in (yd, hT, gd, gx, dh0))
    assert bwd(net.h) == -1 and "first" in capi.last_error() and untouched()          # gradient before any forward
    for bad in (-1, T + 1):
        ln = np.full(B, T, np.int32); ln[2] = bad
        assert fwd(net.h, ln) == -1 and "lengths[2]" in capi.last_error() and untouched()
        yh = np.full((B, T, H), 7.0, np.float32)
        args = (net.h, P(x), P(yh), IP(ln), None, None, None, None) if lstm else (net.h, P(x), P(yh), IP(ln), None, None)
        assert net.f("ApplyTrainingBatchVarLen")(*args) == -1 and "lengths[2]" in capi.last_error() and (yh == 7.0).all()
    assert bwd(net.h) == -1 and untouched()                                            # still no forward
    hi = net.f("CreateForInference")(net.cfg)
    assert fwd(hi, None) == -1 and "inference" in capi.last_error() and untouched()
    assert bwd(hi) == -1 and untouched()
    net.f("Destroy")(hi)
    assert fwd(net.h, np.full(B, T, np.int32)) == 0 and bwd(net.h) == 0 and L.nntk_hip_synchronize() == 0
    assert all(bool(torch.isfinite(t).all()) for t in (yd, hT, gd, gx, dh0)) and not bool((yd == 7.0).any())
    net.close()
