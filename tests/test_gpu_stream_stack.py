"""StreamingStack on the cfg-5 stack shape (Spectrogram 512/400/240 -> Conv1d 257->128 k5 + BN + ReLU -> LSTM 128->512 -> TDD 512->1000),
B = 64 streams with random per-row chunk schedules of up to 160 ms: every valid row equals, bit for bit, the one-shot per-layer chain
(SpectrogramApplyDevice per stream -> conv at batch B -> LSTMApplyDeviceVarLen with the final counts -> TimeDistributedDense).  Rows 0
and B-1 are also within the stack tolerance of the CPU oracle.  A GRU stack (two GRU-256 layers) and one RNN layer likewise."""
import numpy as np
import pytest

import oracle as O
from nntoolkitcore_amd import layers as NL
from nntoolkitcore_amd.streaming import StreamingStack

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NFFT, WIN, NOV, CAP = 512, 400, 240, 2560           # 160 ms of 16 kHz audio per row per push at most


def _u(rng, *s, sc=1.0):
    return rng.uniform(-sc, sc, s).astype(np.float32)


def _front(rng, T):
    spec = NL.Spectrogram(NFFT, WIN, NOV, CAP)
    _, mf = spec.stream_sizes()
    conv = NL.Conv1d(257, 128, 5, 1, mf)
    W, b = _u(rng, 128, 257, 5, sc=(257 * 5) ** -0.5), _u(rng, 128, sc=0.1)
    conv.set_weights(W, b)
    bn = NL.BatchNorm(128, 1e-3, 1)
    bnw = (1 + _u(rng, 128, sc=0.5), _u(rng, 128, sc=0.5), _u(rng, 128, sc=0.1), 1 + np.abs(_u(rng, 128, sc=0.5)))
    bn.set_weights(*bnw)
    relu = NL.Activation("relu", 1, 1.0)
    return spec, conv, (W, b), bn, bnw, relu, conv.stream_sizes()[1]


def _schedules(rng, totals):
    out = []
    for t in totals:
        s, left = [], int(t)
        hop = int(rng.choice([160, 640, 2560]))              # 10 / 40 / 160 ms chunks, with ragged and empty ones mixed in
        while left > 0:
            c = int(min(left, rng.choice([hop, hop, 0, int(rng.integers(1, CAP + 1))])))
            s.append(c)
            left -= c
        out.append(s)
    return out


def _run_stream(stack, streams, scheds):
    B = len(streams)
    got = [[] for _ in range(B)]
    pos = [0] * B
    for i in range(max(len(s) for s in scheds)):
        x = np.zeros((B, CAP), np.float32)
        n_new, final = np.zeros(B, np.int32), np.zeros(B, np.int32)
        for b in range(B):
            if i < len(scheds[b]):
                n = scheds[b][i]
                x[b, :n] = streams[b][pos[b]:pos[b] + n]
                pos[b] += n
                n_new[b], final[b] = n, int(i == len(scheds[b]) - 1)
        out, cnt = stack.push(torch.from_numpy(x).cuda(), n_new, final)
        o = out.cpu().numpy()
        for b in range(B):
            got[b].append(o[b, :cnt[b]])
            assert not o[b, cnt[b]:].any()
    return [np.concatenate(g) for g in got]


def _one_shot_front(streams, conv_w, bn, relu):
    """spectrogram per stream, then the conv at batch B on the padded frames; returns conv output and the per-row valid lengths"""
    B = len(streams)
    specs = []
    for s in streams:
        sp = NL.Spectrogram(NFFT, WIN, NOV, len(s))
        specs.append(sp.apply_device(torch.from_numpy(s[None]).cuda())[0])
        sp.destroy()
    Fm = max(t.shape[0] for t in specs)
    xp = torch.zeros((B, Fm, 257), device="cuda")
    for b, t in enumerate(specs):
        xp[b, :t.shape[0]] = t
    conv = NL.Conv1d(257, 128, 5, 1, Fm)
    conv.set_weights(*conv_w)
    c = conv.apply_device(xp, bn=bn, act=relu)
    conv.destroy()
    lens = np.array([max(0, t.shape[0] - 4) for t in specs], np.int32)
    return c, lens


def _oracle_front(s, conv_w, bnw):
    rs = O.spectrogram(s, O.window("hann", WIN), NFFT, NOV)
    return O.activation(O.ACT_RELU, O.batch_norm(O.conv1d(rs, conv_w[0], conv_w[1], 1), *bnw, 1e-3))


@pytest.mark.parametrize("seed", [0, 1])
def test_lstm_stack_stream_equals_one_shot_chain(seed):
    rng = np.random.default_rng(seed)
    B = 64
    totals = [int(rng.integers(WIN, 16000)) for _ in range(B)]
    streams = [(0.1 * rng.standard_normal(t)).astype(np.float32) for t in totals]
    spec, conv, conv_w, bn, bnw, relu, T = _front(rng, None)
    H, V = 512, 1000
    lw = (_u(rng, 128, 4 * H, sc=128 ** -0.5), _u(rng, H, 4 * H, sc=H ** -0.5), _u(rng, 4 * H, sc=0.1), _u(rng, 4 * H, sc=0.1))
    dw = (_u(rng, H, V, sc=H ** -0.5), _u(rng, V, sc=0.1))
    lstm = NL.LSTM(128, H, True, T, v2=True)
    lstm.set_weights(*lw)
    tdd = NL.TimeDistributedDense(T, H, V)
    tdd.set_weights(*dw)
    stack = StreamingStack(spec, [(conv, bn, relu)], [lstm], head=tdd, batch=B)
    got = _run_stream(stack, streams, _schedules(rng, totals))

    c, lens = _one_shot_front(streams, conv_w, bn, relu)
    Tm = c.shape[1]
    l1 = NL.LSTM(128, H, True, Tm, v2=True)
    l1.set_weights(*lw)
    d1 = NL.TimeDistributedDense(Tm, H, V)
    d1.set_weights(*dw)
    ref = d1.apply_device(l1.apply_device_varlen(c, lens)).cpu().numpy()
    for b in range(B):
        assert got[b].shape[0] == lens[b]
        assert np.array_equal(got[b], ref[b, :lens[b]]), "row %d differs from the one-shot chain" % b
    for b in (0, B - 1):
        r = O.time_distributed_dense(O.lstm(_oracle_front(streams[b], conv_w, bnw)[None], *lw, v2=True), *dw)[0]
        assert np.abs(got[b] - r).max() < 1e-4
    # the slots start new streams after final: state is empty again
    assert not stack.front_state[1].any() and not stack.conv_states[0][1].any() and not stack.h[0][0].any() and not stack.c[0][0].any()
    for o in (spec, conv, bn, relu, lstm, tdd, l1, d1):
        o.destroy()


@pytest.mark.parametrize("kind", ["gru2", "rnn"])
def test_gru_and_rnn_stacks_stream_equal_one_shot_chain(kind):
    rng = np.random.default_rng(7 if kind == "gru2" else 8)
    B = 16
    totals = [int(rng.integers(WIN, 12000)) for _ in range(B)]
    streams = [(0.1 * rng.standard_normal(t)).astype(np.float32) for t in totals]
    spec, conv, conv_w, bn, bnw, relu, T = _front(rng, None)
    if kind == "gru2":
        dims = [(128, 256), (256, 256)]
        ws = [(_u(rng, i, 3 * h, sc=i ** -0.5), _u(rng, h, 3 * h, sc=h ** -0.5), _u(rng, 3 * h, sc=0.1), _u(rng, 3 * h, sc=0.1)) for i, h in dims]
        mk = lambda i, h, t: NL.GRU(i, h, True, t)
    else:
        dims = [(128, 192)]
        ws = [(_u(rng, 128, 192, sc=128 ** -0.5), _u(rng, 192, 192, sc=192 ** -0.5), _u(rng, 192, sc=0.1), _u(rng, 192, sc=0.1))]
        mk = lambda i, h, t: NL.RNN(i, h, True, t, v2=True)
    rec = [mk(i, h, T) for i, h in dims]
    for r, w in zip(rec, ws):
        r.set_weights(*w)
    stack = StreamingStack(spec, [(conv, bn, relu)], rec, batch=B)
    got = _run_stream(stack, streams, _schedules(rng, totals))
    c, lens = _one_shot_front(streams, conv_w, bn, relu)
    y = c
    one = [mk(i, h, c.shape[1]) for i, h in dims]
    for r, w in zip(one, ws):
        r.set_weights(*w)
        y = r.apply_device_varlen(y, lens)
    ref = y.cpu().numpy()
    for b in range(B):
        assert np.array_equal(got[b], ref[b, :lens[b]]), "row %d differs from the one-shot chain" % b
    for o in [spec, conv, bn, relu] + rec + one:
        o.destroy()


def test_stack_checks_shapes_and_resets_rows():
    rng = np.random.default_rng(2)
    spec, conv, conv_w, bn, bnw, relu, T = _front(rng, None)
    bad = NL.LSTM(128, 64, True, T + 1)
    with pytest.raises(ValueError):
        StreamingStack(spec, [(conv, bn, relu)], [bad], batch=2)
    noseq = NL.GRU(128, 64, False, T)
    with pytest.raises(ValueError):
        StreamingStack(spec, [(conv, bn, relu)], [noseq], batch=2)
    g = NL.GRU(128, 64, True, T)
    g.set_weights(_u(rng, 128, 192, sc=.1), _u(rng, 64, 192, sc=.1), _u(rng, 192, sc=.1), _u(rng, 192, sc=.1))
    st = StreamingStack(spec, [(conv, bn, relu)], [g], batch=2)
    x = torch.from_numpy((0.1 * rng.standard_normal((2, CAP))).astype(np.float32)).cuda()
    st.push(x, [CAP, CAP - 300])
    assert st.front_state[1].all() and st.h[0][0].abs().sum() > 0
    st.reset([0])
    assert st.front_state[1][0] == 0 and st.conv_states[0][1][0] == 0 and not st.h[0][0][0].any()
    assert st.front_state[1][1] > 0 and st.h[0][0][1].abs().sum() > 0
    for o in (spec, conv, bn, relu, bad, noseq, g):
        o.destroy()
