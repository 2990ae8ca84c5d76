"""Count arithmetic of the streaming calls (nntk_spectrogram_stream_plan / _sizes, nntk_conv1d_stream_plan / _sizes): pure host
functions, checked against brute-force enumeration of frame and window start positions.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from nntoolkitcore_amd import capi


def _L():
    return capi.load()


def _spec_cfg(nfft, win, nov, n):
    return _L().SpectrogramConfigCreate(nfft, win, nov, n, C.c_float(1.0))


def _sizes(fn, cfg):
    a, b = C.c_int(-7), C.c_int(-7)
    rc = fn(cfg, C.byref(a), C.byref(b))
    return rc, a.value, b.value


def _plan(fn, cfg, state, n_new, final):
    a, b = C.c_int(-7), C.c_int(-7)
    rc = fn(cfg, state, n_new, int(final), C.byref(a), C.byref(b))
    return rc, a.value, b.value


def _schedule(rng, total, cap):
    """random chunk sizes in [0, cap] (zero-length chunks and chunks shorter than a hop included) that sum to total"""
    out, left = [], total
    while left > 0:
        c = int(min(left, rng.choice([0, 1, rng.integers(0, cap + 1), cap, rng.integers(0, max(1, cap // 8) + 1)])))
        out.append(c)
        left -= c
    out += [0] * int(rng.integers(0, 3))
    return out


def _run_spec(cfg, sched, final_at, tf):
    """stream a schedule; final after chunk final_at (then a fresh stream of the rest).  Returns per-stream emitted totals and
    checks every plan against enumeration of frame start positions."""
    L = _L()
    win, step = cfg.window_size, cfg.step
    g = tail = recv = 0
    totals, lens = [], []
    for i, n in enumerate(sched):
        fin = i == final_at or i == len(sched) - 1
        rc, E, nt = _plan(L.nntk_spectrogram_stream_plan, cfg, tail, n, fin)
        assert rc == 0
        recv += n
        # brute force: frames j >= g that are complete within the samples received so far
        F = sum(1 for j in range(g, recv + 1) if j * step + win <= recv)
        assert E == (F if fin else F - (F % 2))
        assert tail + n == recv - g * step                    # the tail holds samples g*step .. recv-1
        g += E
        assert nt == (0 if fin else recv - g * step)
        assert 0 <= nt <= tf
        tail = nt
        if fin:
            totals.append(g)
            lens.append(recv)
            g = tail = recv = 0
    return totals, lens


@pytest.mark.parametrize("seed", range(6))
def test_spectrogram_plan_matches_enumeration(seed):
    rng = np.random.default_rng(seed)
    L = _L()
    for _ in range(25):
        nfft = int(rng.choice([64, 256, 512, 1024]))
        win = int(rng.integers(2, nfft + 1))
        nov = int(rng.integers(0, win))
        cap = int(rng.integers(1, 3 * win))
        cfg = _spec_cfg(nfft, win, nov, cap)
        rc, tf, mf = _sizes(L.nntk_spectrogram_stream_sizes, cfg)
        assert rc == 0 and tf == win + cfg.step - 1 and mf == -(-cap // cfg.step) + 1
        sched = _schedule(rng, int(rng.integers(0, 8 * win)), cap)
        final_at = int(rng.integers(-1, len(sched)))
        totals, lens = _run_spec(cfg, sched, final_at, tf)
        for got, n in zip(totals, lens):
            ts = int((n - nov) / cfg.step) if n >= nov else -1     # C truncation of the one-shot ntime_series
            assert got == max(0, ts)
        # every chunk's frame count fits the output row stride
        for n in range(0, cap + 1, max(1, cap // 7)):
            for t in (0, tf // 2, tf):
                for fin in (0, 1):
                    rc, E, _ = _plan(L.nntk_spectrogram_stream_plan, cfg, t, n, fin)
                    assert rc == 0 and 0 <= E <= mf


def test_spectrogram_plan_refuses_bad_counts():
    L = _L()
    cfg = _spec_cfg(512, 400, 240, 160)
    tf = 400 + 160 - 1
    for t, n in ((-1, 0), (tf + 1, 0), (0, -1), (0, 161)):
        rc, E, nt = _plan(L.nntk_spectrogram_stream_plan, cfg, t, n, 0)
        assert rc == -1 and (E, nt) == (-7, -7) and capi.last_error()
    assert _plan(L.nntk_spectrogram_stream_plan, cfg, tf, 160, 0)[0] == 0


def _run_conv(cfg, sched, final_at, hr):
    L = _L()
    k, s = cfg.kernel_size, cfg.stride
    g = hist = recv = 0
    totals, lens = [], []
    for i, n in enumerate(sched):
        fin = i == final_at or i == len(sched) - 1
        rc, O, nh = _plan(L.nntk_conv1d_stream_plan, cfg, hist, n, fin)
        assert rc == 0
        recv += n
        assert hist + n == recv - g * s                       # the history holds rows g*s .. recv-1
        O_bf = sum(1 for o in range(g, recv + 1) if o * s + k <= recv)
        assert O == O_bf
        g += O
        assert nh == (0 if fin else recv - g * s) and 0 <= nh <= hr
        hist = nh
        if fin:
            totals.append(g)
            lens.append(recv)
            g = hist = recv = 0
    return totals, lens


@pytest.mark.parametrize("seed", range(6))
def test_conv1d_plan_matches_enumeration(seed):
    rng = np.random.default_rng(100 + seed)
    L = _L()
    for _ in range(30):
        k = int(rng.integers(1, 10))
        s = min(k, int(rng.choice([1, 2, k, int(rng.integers(1, k + 1))])))
        cap = int(rng.integers(1, 40))
        cfg = L.Conv1dConfigCreate(8, 16, k, s, cap)
        rc, hr, mo = _sizes(L.nntk_conv1d_stream_sizes, cfg)
        assert rc == 0 and hr == k - 1 and mo == -(-cap // s)
        sched = _schedule(rng, int(rng.integers(0, 200)), cap)
        final_at = int(rng.integers(-1, len(sched)))
        totals, lens = _run_conv(cfg, sched, final_at, hr)
        for got, n in zip(totals, lens):
            if n >= k - s:
                assert got == L.Conv1dConfigCreate(8, 16, k, s, n).output_size
            else:
                assert got == 0
        for n in range(0, cap + 1):
            for h in range(0, hr + 1):
                rc, O, _ = _plan(L.nntk_conv1d_stream_plan, cfg, h, n, 0)
                assert rc == 0 and 0 <= O <= mo


def test_conv1d_stride_above_kernel_is_refused():
    L = _L()
    cfg = L.Conv1dConfigCreate(8, 16, 3, 4, 20)
    assert _sizes(L.nntk_conv1d_stream_sizes, cfg)[0] == -1
    rc, O, nh = _plan(L.nntk_conv1d_stream_plan, cfg, 0, 10, 0)
    assert rc == -1 and (O, nh) == (-7, -7) and "stride" in capi.last_error()
    cfg = L.Conv1dConfigCreate(8, 16, 5, 1, 20)
    for h, n in ((-1, 0), (5, 0), (0, 21), (0, -1)):
        assert _plan(L.nntk_conv1d_stream_plan, cfg, h, n, 0)[0] == -1
