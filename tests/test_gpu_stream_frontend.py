"""Streaming front end (SpectrogramApplyDeviceStream, LogMelSpectrogramApplyDeviceStream, Conv1dBatchNormActivationApplyDeviceStream,
TimeDistributedDenseApplyDeviceVarLen): B ragged streams with random per-row chunk schedules; the concatenated stream output equals the
one-shot call on each stream's whole input BIT FOR BIT, padding rows are zeros, state is updated in place, and every refused call
leaves the output, the state and the host counts untouched."""
import numpy as np
import pytest

from nntoolkitcore_amd import capi
from nntoolkitcore_amd import layers as NL

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _schedules(rng, totals, cap):
    """per row: chunk sizes in [0, cap], zero-length and sub-hop chunks included, summing to the row's total"""
    out = []
    for t in totals:
        s, left = [], int(t)
        while left > 0:
            c = int(min(left, rng.choice([0, 1, 7, cap, int(rng.integers(0, cap + 1)), int(rng.integers(0, cap + 1))])))
            s.append(c)
            left -= c
        out.append(s)
    return out


def _stream(stage, streams, scheds, cap, state, feat_shape, extra=None):
    """push every row's chunks; a row's last chunk carries final.  Returns per-row concatenated outputs (numpy)."""
    B = len(streams)
    n_calls = max(len(s) for s in scheds)
    got = [[] for _ in range(B)]
    pos = [0] * B
    for i in range(n_calls):
        x = np.zeros((B, cap) + feat_shape, np.float32)
        n_new = np.zeros(B, np.int32)
        final = np.zeros(B, np.int32)
        for b in range(B):
            if i < len(scheds[b]):
                n = scheds[b][i]
                x[b, :n] = streams[b][pos[b]:pos[b] + n]
                pos[b] += n
                n_new[b] = n
                final[b] = int(i == len(scheds[b]) - 1)
        out, cnt = stage(torch.from_numpy(x).cuda(), n_new, state, final)
        o = out.cpu().numpy()
        for b in range(B):
            got[b].append(o[b, :cnt[b]])
            assert not o[b, cnt[b]:].any(), "padding rows must be zeros"
    return [np.concatenate(g) for g in got]


SPEC_CASES = [
    # nfft, win, nov, mode, window, fft_norm          route
    (512, 400, 240, "magnitude", "hann_window", 1.0),      # pair kernel, NZ7
    (512, 320, 160, "psd", "hamming_window", 0.5),         # pair kernel, all rows masked, NORM
    (1024, 800, 480, "magnitude", "blackman_window", 1.0),  # mixed radix
    (98, 80, 40, "psd", "ones", 1.0),                       # direct DFT (7 * 7 * 2)
]


@pytest.mark.parametrize("case", SPEC_CASES, ids=lambda c: "nfft%d_w%d_%s" % (c[0], c[1], c[3]))
def test_spectrogram_stream_equals_one_shot(case):
    nfft, win, nov, mode, wname, norm = case
    rng = np.random.default_rng(nfft + win)
    step = win - nov
    B, cap = 7, 3 * step + 11
    totals = [int(rng.integers(win, 14 * step)) for _ in range(B)] + [win - 1, win + step]   # also: no frame at all, exactly two frames
    B = len(totals)
    streams = [rng.standard_normal(t).astype(np.float32) for t in totals]
    spec = NL.Spectrogram(nfft, win, nov, cap, mode=mode, fft_norm=norm, window_name=wname)
    state = spec.new_stream_state(B)
    tail_ptr = state[0].data_ptr()
    got = _stream(lambda x, n, st, f: spec.apply_device_stream(x, n, st, final=f), streams, _schedules(rng, totals, cap), cap, state, ())
    assert state[0].data_ptr() == tail_ptr and not state[1].any()
    parity = set()
    for b in range(B):
        one = NL.Spectrogram(nfft, win, nov, totals[b], mode=mode, fft_norm=norm, window_name=wname)
        ref = one.apply_device(torch.from_numpy(streams[b][None]).cuda()).cpu().numpy()[0] if one.cfg.ntime_series > 0 else \
            np.zeros((0, spec.cfg.nfreq), np.float32)
        assert got[b].shape == ref.shape, (b, got[b].shape, ref.shape)
        assert np.array_equal(got[b], ref), "row %d differs from the one-shot call" % b
        parity.add(ref.shape[0] % 2)
        one.destroy()
    assert parity == {0, 1}
    spec.destroy()


def _logmel_stream_equals_one_shot(nfft, win, nov, fused, **spec_kw):
    rng = np.random.default_rng(5 + nfft + fused)
    step = win - nov
    B, cap = 6, 2 * step + 5
    totals = [int(rng.integers(win, 12 * step)) for _ in range(B)]
    streams = [rng.standard_normal(t).astype(np.float32) for t in totals]
    if not fused:
        capi.set_option("spec_variant", 1)
    try:
        spec = NL.Spectrogram(nfft, win, nov, cap, **spec_kw)
        lm = NL.LogMelSpectrogram(spec, 40)
        state = lm.new_stream_state(B)
        got = _stream(lambda x, n, st, f: lm.apply_device_stream(x, n, st, final=f), streams, _schedules(rng, totals, cap), cap, state, ())
        for b in range(B):
            s1 = NL.Spectrogram(nfft, win, nov, totals[b], **spec_kw)
            l1 = NL.LogMelSpectrogram(s1, 40)
            ref = l1.apply_device(torch.from_numpy(streams[b][None]).cuda()).cpu().numpy()[0]
            assert got[b].shape == ref.shape, (b, got[b].shape, ref.shape)
            assert np.array_equal(got[b], ref), "row %d differs from the one-shot call" % b
            l1.destroy(); s1.destroy()
        lm.destroy(); spec.destroy()
    finally:
        capi.set_option("spec_variant", "auto")


@pytest.mark.parametrize("nfft,win,nov,fused", [(512, 400, 240, True), (512, 400, 240, False), (1024, 800, 480, False)])
def test_logmel_stream_equals_one_shot(nfft, win, nov, fused):
    _logmel_stream_equals_one_shot(nfft, win, nov, fused)


@pytest.mark.parametrize("nfft,win,nov", [(512, 512, 128), (512, 320, 160)])
def test_fused_logmel_stream_equals_one_shot_psd_norm_unmasked_rows(nfft, win, nov):
    """the fused stream form beyond window 400: all eight register rows masked, four loads per lane (512, 128) and three (320, 160),
    fft_norm 0.5, PSD"""
    _logmel_stream_equals_one_shot(nfft, win, nov, True, mode="psd", fs=16000, fft_norm=0.5)


CONV_CASES = [(257, 128, 5, 1), (40, 128, 5, 1), (64, 64, 5, 2)]   # cfg-5 shape, flat-K shape, stride 2


def _conv_layers(rng, cin, cout, k, s, T):
    conv = NL.Conv1d(cin, cout, k, s, T)
    conv.set_weights(rng.uniform(-1, 1, (cout, cin, k)).astype(np.float32) * (cin * k) ** -0.5, rng.uniform(-.1, .1, cout).astype(np.float32))
    return conv


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "%d_%d_k%d_s%d" % c)
def test_conv_stream_equals_one_shot(case):
    cin, cout, k, s = case
    rng = np.random.default_rng(cin + s)
    B, cap = 9, 13
    totals = [int(rng.integers(k, 90)) for _ in range(B)] + [k - 1]
    B = len(totals)
    streams = [rng.standard_normal((t, cin)).astype(np.float32) for t in totals]
    W, bias = rng.uniform(-1, 1, (cout, cin, k)).astype(np.float32) * (cin * k) ** -0.5, rng.uniform(-.1, .1, cout).astype(np.float32)
    bn = NL.BatchNorm(cout, 1e-3, 1)
    bn.set_weights(1 + rng.uniform(-.5, .5, cout), rng.uniform(-.5, .5, cout), rng.uniform(-.1, .1, cout), 1 + rng.uniform(0, .5, cout))
    relu = NL.Activation("relu", 1, 1.0)
    conv = NL.Conv1d(cin, cout, k, s, cap)
    conv.set_weights(W, bias)
    state = conv.new_stream_state(B)
    got = _stream(lambda x, n, st, f: conv.apply_device_stream(x, n, st, bn=bn, act=relu, final=f), streams,
                  _schedules(rng, totals, cap), cap, state, (cin,))
    Tm = max(totals)
    one = NL.Conv1d(cin, cout, k, s, Tm)
    one.set_weights(W, bias)
    xp = np.zeros((B, Tm, cin), np.float32)
    for b in range(B):
        xp[b, :totals[b]] = streams[b]
    ref = one.apply_device(torch.from_numpy(xp).cuda(), bn=bn, act=relu).cpu().numpy()
    for b in range(B):
        n = max(0, (totals[b] - k) // s + 1) if totals[b] >= k else 0
        assert got[b].shape[0] == n
        assert np.array_equal(got[b], ref[b, :n]), "row %d differs from the one-shot call" % b
    for o in (conv, one, bn, relu):
        o.destroy()


def test_spectrogram_state_in_place_and_slot_reuse():
    """the tail holds the row's unconsumed samples, in the caller's buffer; a final row followed by a new stream in the same slot
    equals a one-shot of the new stream"""
    nfft, win, nov = 512, 400, 240
    step = win - nov
    rng = np.random.default_rng(11)
    cap = 1000
    spec = NL.Spectrogram(nfft, win, nov, cap)
    tail, tl = state = spec.new_stream_state(2)
    a = rng.standard_normal(1700).astype(np.float32)
    x = np.zeros((2, cap), np.float32)
    x[0, :cap] = a[:cap]
    out, fr = spec.apply_device_stream(torch.from_numpy(x).cuda(), [cap, 0], state)
    F = (cap - nov) // step
    assert fr[0] == F - F % 2 and fr[1] == 0
    assert tl[0] == cap - fr[0] * step and tl[1] == 0
    assert np.array_equal(tail[0, :tl[0]].cpu().numpy(), a[fr[0] * step:cap])
    x[0, :700] = a[cap:]
    spec.apply_device_stream(torch.from_numpy(x).cuda(), [700, 0], state, final=[1, 0])
    assert tl[0] == 0
    bnew = rng.standard_normal(900).astype(np.float32)
    x[0, :900] = bnew
    out, fr = spec.apply_device_stream(torch.from_numpy(x).cuda(), [900, 0], state, final=[1, 0])
    one = NL.Spectrogram(nfft, win, nov, 900)
    ref = one.apply_device(torch.from_numpy(bnew[None]).cuda()).cpu().numpy()[0]
    assert np.array_equal(out[0, :fr[0]].cpu().numpy(), ref)
    one.destroy(); spec.destroy()


def _untouched(call, outs, states, hosts):
    before = [t.clone() for t in outs + states] + [h.copy() for h in hosts]
    with pytest.raises(capi.NNTKError):
        call()
    torch.cuda.synchronize()
    after = [t for t in outs + states] + list(hosts)
    for x, y in zip(before, after):
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, y)
        else:
            assert torch.equal(x, y)


def test_stream_validation_leaves_everything_untouched():
    nfft, win, nov, cap = 512, 400, 240, 320
    spec = NL.Spectrogram(nfft, win, nov, cap)
    B = 3
    tail, tl = state = spec.new_stream_state(B)
    tail.fill_(0.25)
    tl[:] = [5, 0, 100]
    x = torch.randn(B, cap, device="cuda")
    tf, mf = spec.stream_sizes()
    out = torch.full((B, mf, spec.cfg.nfreq), 7.0, device="cuda")
    fr = np.full(B, -3, np.int32)
    L = capi.load()

    def sp(n_new, tl_=None, o=out, xx=x, batch=B):
        t = tl if tl_ is None else tl_
        rc = L.SpectrogramApplyDeviceStream(spec.h, NL._dp(xx), np.asarray(n_new, np.int32).ctypes.data_as(capi.ip), None, NL._dp(tail),
                                            t.ctypes.data_as(capi.ip), NL._dp(o), fr.ctypes.data_as(capi.ip), batch)
        capi.check(rc, "SpectrogramApplyDeviceStream")

    _untouched(lambda: sp([1, cap + 1, 0]), [out], [tail], [tl, fr])          # n_new above input_size
    _untouched(lambda: sp([1, -1, 0]), [out], [tail], [tl, fr])               # negative n_new
    bad = tl.copy(); bad[2] = tf + 1
    _untouched(lambda: sp([1, 1, 1], bad), [out], [tail], [tl, fr, bad])      # tail_len above tail_floats
    _untouched(lambda: sp([1, 1, 1], batch=-1), [out], [tail], [tl, fr])      # batch < 0
    big = torch.zeros(B * cap + B * mf * spec.cfg.nfreq, device="cuda")
    _untouched(lambda: sp([1, 1, 1], o=big[B * cap - 8:], xx=big), [big], [tail], [tl, fr])    # output overlaps the input
    _untouched(lambda: capi.check(L.SpectrogramApplyDeviceStream(spec.h, NL._dp(x), None, None, NL._dp(tail), tl.ctypes.data_as(capi.ip),
                                                                 NL._dp(out), fr.ctypes.data_as(capi.ip), B), "x"), [out], [tail], [tl, fr])

    # conv: stride > kernel_size, BN channels, activation, overlap, hist_len
    conv = NL.Conv1d(16, 32, 3, 1, 8)
    conv.set_weights(np.ones((32, 16, 3), np.float32), np.zeros(32, np.float32))
    hist, hl = cst = conv.new_stream_state(B)
    hist.fill_(0.5)
    hl[:] = [2, 1, 0]
    cx = torch.randn(B, 8, 16, device="cuda")
    cout = torch.full((B, 8, 32), 3.0, device="cuda")
    nco = np.full(B, -5, np.int32)
    bn_bad = NL.BatchNorm(16, 1e-3, 1)
    soft = NL.Activation("softmax", 32, vector_size=32)
    for kw in (dict(bn=bn_bad), dict(act=soft)):
        _untouched(lambda: conv.apply_device_stream(cx, [1, 1, 1], cst, out=cout, **kw), [cout], [hist], [hl])
    _untouched(lambda: conv.apply_device_stream(cx, [9, 1, 1], cst, out=cout), [cout], [hist], [hl])
    bad = hl.copy(); bad[0] = 3
    _untouched(lambda: conv.apply_device_stream(cx, [1, 1, 1], (hist, bad), out=cout), [cout], [hist], [hl, bad])
    big = torch.zeros(B * 8 * 16 + B * 8 * 32, device="cuda")
    xv, ov = big[:B * 8 * 16].view(B, 8, 16), big[B * 8 * 16 - 16:B * 8 * 16 - 16 + B * 8 * 32].view(B, 8, 32)
    _untouched(lambda: conv.apply_device_stream(xv, [1, 1, 1], cst, out=ov), [big], [hist], [hl])      # output overlaps the input
    # the Python wrappers refuse tensors whose shape is not the handle's before the C call reads them
    with pytest.raises(ValueError):
        conv.apply_device_stream(cx[:, :4].contiguous(), [1, 1, 1], cst)
    with pytest.raises(ValueError):
        spec.apply_device_stream(x[:, :cap // 2].contiguous(), [1, 1, 1], state)
    wide = NL.Conv1d(16, 32, 3, 4, 8)
    wide.set_weights(np.ones((32, 16, 3), np.float32), np.zeros(32, np.float32))
    _untouched(lambda: wide.apply_device_stream(cx, [1, 1, 1], cst, out=cout), [cout], [hist], [hl])
    for o in (spec, conv, wide, bn_bad, soft):
        o.destroy()


@pytest.mark.parametrize("nfft,force_unfused", [(1024, False), (512, True)])
def test_logmel_stream_validation_on_the_two_kernel_form(nfft, force_unfused):
    """the two-kernel log-mel form (spectrogram into handle scratch, then the mel GEMM into the caller's output) refuses a NULL output
    and an output that overlaps the tail before anything is enqueued: tail, counts and output untouched"""
    win, nov, cap, B, n_mels = (800, 480, 640, 3, 40) if nfft == 1024 else (400, 240, 320, 3, 40)
    if force_unfused:
        capi.set_option("spec_variant", 1)
    try:
        spec = NL.Spectrogram(nfft, win, nov, cap)
        lm = NL.LogMelSpectrogram(spec, n_mels)
        tf, mf = lm.stream_sizes()
        L = capi.load()
        n_tail, n_out = B * tf, B * mf * n_mels
        big = torch.full((n_tail + n_out,), 0.5, device="cuda")
        tail = big[:n_tail]
        tl = np.array([3, 0, tf], np.int32)
        fr = np.full(B, -3, np.int32)
        x = torch.randn(B, cap, device="cuda")
        nn = np.array([cap, 5, 0], np.int32)
        out = torch.full((n_out,), 7.0, device="cuda")

        def call(o):
            capi.check(L.LogMelSpectrogramApplyDeviceStream(lm.h, NL._dp(x), nn.ctypes.data_as(capi.ip), None, NL._dp(tail),
                                                            tl.ctypes.data_as(capi.ip), o, fr.ctypes.data_as(capi.ip), B),
                       "LogMelSpectrogramApplyDeviceStream")

        _untouched(lambda: call(None), [out], [big], [tl, fr, nn])                                   # NULL output
        _untouched(lambda: call(NL._dp(big[n_tail - 16:n_tail - 16 + n_out])), [out], [big], [tl, fr, nn])   # output overlaps the tail
        # ... and the same arguments with a proper output go through
        call(NL._dp(out))
        torch.cuda.synchronize()
        assert (fr >= 0).all() and not (out == 7.0).any()      # every output row is a frame or a zero row
        lm.destroy(); spec.destroy()
    finally:
        capi.set_option("spec_variant", "auto")


def test_tdd_varlen_zeros_past_lengths_and_keeps_bits():
    rng = np.random.default_rng(3)
    B, T, I, V = 5, 11, 64, 96
    tdd = NL.TimeDistributedDense(T, I, V)
    tdd.set_weights(rng.uniform(-.2, .2, (I, V)).astype(np.float32), rng.uniform(-.1, .1, V).astype(np.float32))
    x = torch.randn(B, T, I, device="cuda")
    ref = tdd.apply_device(x)
    lens = np.array([0, 3, 11, 7, 1], np.int32)
    got = tdd.apply_device_varlen(x, lens)
    for b in range(B):
        assert torch.equal(got[b, :lens[b]], ref[b, :lens[b]])
        assert not got[b, lens[b]:].any()
    assert torch.equal(tdd.apply_device_varlen(x), ref)
    out = torch.full_like(ref, 2.0)
    with pytest.raises(capi.NNTKError):
        tdd.apply_device_varlen(x, [0, 3, 12, 7, 1], out=out)
    assert (out == 2.0).all()
    tdd.destroy()
