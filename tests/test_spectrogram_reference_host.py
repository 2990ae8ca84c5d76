"""CPU-only premises of tests/test_gpu_spectrogram_matrix.py: for every case of that file the float64 reference
(spectrogram_reference.py) agrees with the float32 oracle within a bound worked out from float32 arithmetic alone, the oracle's
error is recorded (the GPU test's yardstick e32), the case takes the kernel form its name claims, and the 64 forms of
spectrogram512_kernel<MODE, NORM, NZ7, NLD, MEL, DMA = false, ST> are all reached.

Bounds on the float32 evaluations, as multiples of U = 2^-24, relative to max |ref|:
  * the scale factor is a left-to-right float32 sum of `window` non-negative terms: relative error <= (window - 1) U;
  * a float32 FFT of nfft points loses c log2(nfft) U of the spectrum's root mean square per element (<= max |X|); c = 32 covers
    kissfft's radix-2/3/4/5 butterflies and its generic prime-radix one with room to spare;
  * the PSD squares the spectrum (twice the relative error).
  So e32 <= (1 or 2) * (window + 32 log2 nfft) U.  The direct float32 DFT has the textbook bound of a recursive sum instead:
  |error of bin k| <= gamma * sum_n |frame[n]| with gamma = (window + 2) U / (1 - (window + 2) U), evaluated on the case's own frames.
  * log-mel: a mel value is a sum of non-negative terms, so |d mel_m| <= sum_k W[k, m] * max |d spec| + (run + 1) U mel_m, and
    |d log| <= -log(1 - d mel_m / (mel_m + eps)) + 2 U |log|.
"""
import numpy as np
import pytest

import oracle as O
import spectrogram_reference as SR

U = SR.U


def _spec_rel_bound(case):
    return (2 if case.mode == "psd" else 1) * (case.win + 32 * np.log2(case.nfft)) * U


@pytest.mark.parametrize("case", SR.ALL_CASES, ids=lambda c: c.name)
def test_reference_agrees_with_the_float32_oracle(case):
    res = SR.evaluate(case)
    w = O.window("hann", case.win)
    nts = (case.N - case.nov) // (case.win - case.nov)
    assert res.spec.shape == ((case.B if case.rows is None else len(case.rows)), nts, case.nfft // 2 + 1)
    assert res.spec.dtype == np.float64 and np.isfinite(res.spec).all() and res.spec.max() > 0
    top = float(np.abs(res.spec).max())
    rel = _spec_rel_bound(case)
    if res.kernel == "direct":
        # the FFT oracle checks the float64 reference at this size; the yardstick of the direct kernel is the direct float32 sum
        fft32 = O.spectrogram(res.x, w, case.nfft, case.nov, mode=case.mode, fs=SR.FS, fft_norm=case.fft_norm)
        e_fft = float(np.abs(fft32 - res.spec).max() / top)
        print("%s: kissfft oracle error %.3e (bound %.3e)" % (case.name, e_fft, rel))
        assert e_fft <= rel
        g = (case.win + 2) * U
        g = g / (1 - g)
        fr = np.abs(res.x[:, SR._frames(res.x, case.win, case.nov)].astype(np.float64) * w).sum(-1).max()     # max_frame sum_n |frame[n]|
        X = g * fr * float(np.float32(case.fft_norm))
        # |d |X|| <= |dX| (magnitude); |d |X|^2| <= 2 |X| |dX| + |dX|^2 (PSD, interior bins doubled), both over the float64 scale
        ws = w.astype(np.float64)
        if case.mode == "magnitude":
            lim = X / ws.sum() / top + rel
        else:
            xmax = np.sqrt(top * SR.FS * (ws * ws).sum())       # >= |X| of every bin (edge bins are not doubled)
            lim = 2 * (2 * xmax * X + X * X) / (SR.FS * (ws * ws).sum()) / top + rel
        print("%s: direct float32 DFT error e32 %.3e (worst-case bound %.3e)" % (case.name, res.e32_spec, lim))
        assert res.e32_spec <= lim
    else:
        print("%s: oracle error e32 %.3e (bound %.3e)" % (case.name, res.e32_spec, rel))
        assert res.e32_spec <= rel
    assert res.e32_spec > 0                      # a yardstick of exactly zero would mean the two evaluations are the same code
    if not case.n_mels:
        assert res.logmel is None
        return
    W = O.mel_filterbank_weights(case.n_mels, case.nfft, SR.FS, case.lo_hz, case.hi_hz).astype(np.float64)
    assert res.logmel.shape == (case.B, nts, case.n_mels) and np.isfinite(res.logmel).all()
    if case.rows is None:
        mel = res.spec @ W
        run = (W != 0).sum(0)
        dmel = W.sum(0) * (rel * top) + (run + 1) * U * mel
        r = dmel / (mel + SR.LOG_EPS)
        assert r.max() < 0.5, "a mel value this close to zero has no usable log bound: choose another input"
        lim = -np.log1p(-r) + 2 * U * np.abs(res.logmel)
        err = np.abs(res.o32_logmel - res.logmel)
        print("%s: oracle log-mel error e32 %.3e (largest error / bound %.3f)" % (case.name, res.e32_logmel, (err / lim).max()))
        assert (err <= lim).all()
        assert res.e32_logmel == err.max()
    else:
        print("%s: oracle log-mel error e32 %.3e" % (case.name, res.e32_logmel))
    assert res.e32_logmel > 0


@pytest.mark.parametrize("case", SR.FORM_CASES, ids=lambda c: c.name)
def test_form_cases_take_the_route_their_name_claims(case):
    mode, norm, nz7, nld = SR.FORM_EXPECT[case.name]
    step = case.win - case.nov
    nts = (case.N - case.nov) // step
    assert case.B == 3 and case.N % 2 == 1 and nts % 2 == 1 and 5 <= nts <= 9
    assert case.name == SR.form_name(case.mode, case.fft_norm, case.win, case.nov)
    for mel in (False, True):
        for st in (False, True):
            r = SR.route(case.nfft, case.win, case.nov, case.mode, case.fft_norm, mel, st, B=case.B, nts=nts, n_mels=case.n_mels)
            assert r.kernel == "512" and r.fused == mel
            assert r.form == (mode, norm, nz7, nld, mel, st), (case.name, mel, st, r.form)
            assert r.gy == case.B and r.gx == 1


def test_the_form_cases_reach_all_64_forms():
    seen = set()
    for case in SR.FORM_CASES:
        nts = (case.N - case.nov) // (case.win - case.nov)
        for mel in (False, True):
            for st in (False, True):
                seen.add(SR.route(case.nfft, case.win, case.nov, case.mode, case.fft_norm, mel, st, B=case.B, nts=nts,
                                  n_mels=case.n_mels).form)
    assert len(SR.ALL_FORMS) == 64
    assert seen == SR.ALL_FORMS, sorted(SR.ALL_FORMS - seen)


def test_pairs_per_wave_cases_walk_the_prefetch_loop_as_claimed():
    """spec_ppw in {1, 2, 3, 16} at 45 frames: waves with 1, 2, 5 and 6 pairs and one idle wave -- prologue only, even tail, odd tail,
    and several turns of the unrolled-by-two loop; the short inputs give every wave 0 or 1 pairs."""
    counts = set()
    idle = False
    for ppw in SR.PPW_VALUES:
        r = SR.route(512, 400, 240, "magnitude", 1.0, False, False, B=2, nts=45, ppw=ppw)
        assert r.gy == 2 and r.form == (0, False, True, 3, False, False)
        per = SR.pairs_per_wave(45, r.gx)
        assert sum(per) == 23
        counts |= set(per)
        idle |= 0 in per
    assert {1, 2, 5, 6} <= counts and idle, counts
    assert SR.route(512, 400, 240, "magnitude", 1.0, False, False, B=2, nts=45).gx == 2          # the automatic ppw = 4
    for nts in (1, 2, 3):
        for ppw in SR.PPW_VALUES + (0,):
            per = SR.pairs_per_wave(nts, SR.route(512, 400, 240, "magnitude", 1.0, False, False, B=2, nts=nts, ppw=ppw).gx)
            assert set(per) <= {0, 1} and sum(per) == (nts + 1) // 2
    for nts, case in SR.PPW_CASES.items():
        assert (case.N - case.nov) // (case.win - case.nov) == nts and case.N % 2 == 1 and case.B == 2


def test_row_stride_case_strides_over_rows():
    c = SR.STRIDE_CASE
    nts = (c.N - c.nov) // (c.win - c.nov)
    assert nts == 66 and c.N % 2 == 1
    for mel in (False, True):
        r = SR.route(c.nfft, c.win, c.nov, c.mode, c.fft_norm, mel, False, B=c.B, nts=nts, ppw=1, n_mels=c.n_mels)
        assert r.kernel == "512" and r.fused == mel and (r.gx, r.gy) == (9, 1024) and r.gy < c.B
    # without the option no shape below 65536 rows makes a block take a second row: a large B drives ppw to 16
    assert SR.route(c.nfft, c.win, c.nov, c.mode, c.fft_norm, False, False, B=c.B, nts=nts).gy == c.B
    assert {0, 1, c.B // 2 - 1, c.B // 2, c.B - 1} == set(c.rows)      # first and last row of both turns of the loop


def test_mel_limit_and_direct_cases_take_their_routes():
    for c in SR.MEL_LIMIT_CASES:
        r = SR.route(c.nfft, c.win, c.nov, c.mode, c.fft_norm, True, False, B=c.B, nts=7, n_mels=c.n_mels)
        assert r.fused == (c.n_mels <= 257) and r.form[4] == r.fused and r.form[:4] == (0, False, True, 3)
    assert sorted(c.n_mels for c in SR.MEL_LIMIT_CASES) == [128, 200, 256, 257, 258]
    for c in SR.DIRECT_CASES:
        assert c.nfft > 4096 and SR.route(c.nfft, c.win, c.nov, c.mode, c.fft_norm, False, False).kernel == "direct"
    R = SR.REFUSED
    assert R["win"] > 16384 and SR.route(R["nfft"], R["win"], R["nov"], "magnitude", 1.0, False, False).kernel == "refused"
    # the routes of the cases the older tests run, as a check of route() itself
    assert SR.route(1024, 800, 480, "magnitude", 1.0, False, False).kernel == "mixed"
    assert SR.route(480, 400, 240, "magnitude", 1.0, True, False).fused is False
    for nfft in (77, 98, 1022, 4099, 8192):
        assert SR.route(nfft, min(nfft, 600), 0, "psd", 1.0, False, False).kernel == "direct"


@pytest.mark.parametrize("case,ahead", SR.POISON_CASES, ids=lambda v: getattr(v, "name", str(v)))
def test_poison_cases_put_the_sample_where_only_the_mask_stops_it(case, ahead):
    step = case.win - case.nov
    x, spec, logmel, bad, pair_bad = SR.evaluate_poisoned(case, ahead)
    nts = spec.shape[1]
    assert nts % 2 == 1 and not bad[0].any()
    reach = 4 * ((step + case.win + 3) // 4) - step     # samples of frame B that the pair's 16-byte loads bring in
    assert case.win < reach
    for (b, q, v), pair in zip(SR.poison_positions(case, ahead), (0, 1)):
        assert not np.isfinite(x[b, q]) and np.isfinite(np.delete(x[b], q)).all()
        start = 2 * pair * step
        assert start + step + case.win <= q < start + step + reach           # loaded with pair `pair`, past frame B's window
        assert not pair_bad[b, 2 * pair] and not pair_bad[b, 2 * pair + 1]   # ... so that pair stays finite
        assert bad[b].any() and bad[b, :2 * pair + 2].sum() == 0
        assert not np.isfinite(logmel[b][bad[b]]).all(-1).any() and np.isfinite(logmel[b][~bad[b]]).all()
    form = SR.route(case.nfft, case.win, case.nov, case.mode, case.fft_norm, False, False, B=case.B, nts=nts).form
    assert form[2] == (case.win == 401)


def test_reference_matches_a_literal_dft_on_a_tiny_frame():
    """the reference against the definition written out: one frame, nfft 16, window 12"""
    rng = np.random.default_rng(1)
    x = rng.standard_normal(12).astype(np.float32)
    w = O.window("hann", 12)
    n, k = np.arange(16)[None, :], np.arange(9)[:, None]
    f = np.zeros(16)
    f[:12] = x.astype(np.float64) * w
    X = (f[None, :] * np.exp(-2j * np.pi * k * n / 16)).sum(1) * 0.5
    mag = SR.spectrogram64(x[None], w, 16, 4, fft_norm=0.5)[0, 0]
    np.testing.assert_allclose(mag, np.abs(X) / w.astype(np.float64).sum(), rtol=1e-12, atol=1e-15)
    psd = SR.spectrogram64(x[None], w, 16, 4, mode="psd", fs=8000, fft_norm=0.5)[0, 0]
    want = np.abs(X) ** 2 * np.r_[1.0, np.full(7, 2.0), 1.0] / (8000 * (w.astype(np.float64) ** 2).sum())
    np.testing.assert_allclose(psd, want, rtol=1e-12, atol=1e-18)
    d32 = SR.direct_dft32(x[None], w, 16, 4, mode="psd", fs=8000, fft_norm=0.5)[0, 0]
    np.testing.assert_allclose(d32, want, rtol=64 * U, atol=64 * U * want.max())
