"""Every form of the 512-point spectrogram kernel, and the routes around it, against a float64 reference.

spectrogram512_kernel<MODE, NORM, NZ7, NLD, MEL, DMA = false, ST> exists in 64 forms; the cases below run each of them one-shot
(compared with tests/spectrogram_reference.py, a float64 numpy restatement of the operation) and streamed (bit for bit equal to the
one-shot call).  Further: the pairs a wavefront walks through its two-deep prefetch loop (option spec_ppw), the loop in which one
workgroup takes several rows, the fused mel tables at their limits (257 filters, one- and two-bin runs, empty runs) and the fall-back
beyond them, the direct DFT above nfft 4096 and its refusal of a window that does not fit into LDS.
tests/test_spectrogram_reference_host.py checks on the CPU that every case takes the route claimed here.

Tolerance.  |device - ref| <= max(FACTOR * e32, FLOOR) * max |ref| on a spectrogram; on a log-mel output the same on the absolute
error of the logarithm, the floor times max(1, max |ref|).  e32 is the error of a float32 CPU evaluation of the same case against the
float64 reference -- the oracle (kissfft) for the 512-point kernel, a left-to-right float32 sum of the same terms for the direct DFT,
whose error grows with the window as kissfft's does not -- and never a device figure.  FACTOR = 4, FLOOR = 16 * 2^-24: another
summation order may cost a few roundings, not an order of magnitude.  Every test prints its ratio error / bound.

Also here, beyond the forms: a non-finite sample that a pair's loads bring in but that lies in neither frame's window.  At window 400,
hop 160 no such sample exists (step + window is a multiple of four, and the lanes past it read zeros), so nothing there can tell the
kernel's AND masks from a product with the zero tap; windows 401 / hop 161 and 300 / hop 263 can.

Measured (device errors on an MI355X; e32 on the CPU), worst case per route, spectrogram figures relative to max |ref|:
  512-point kernel, spectrogram (24 runs):  e32 4.7e-07, device error 5.4e-07, bound 9.5e-07 .. 1.9e-06, worst error / bound 0.35
  512-point kernel, fused log-mel (24 runs): e32 6.8e-06, device error 3.9e-06, bound 5.8e-06 .. 2.8e-05, worst error / bound 0.47
  two-kernel log-mel at 258 filters:         e32 1.7e-06, device error 2.4e-06, bound 2.8e-05 (the floor times |log eps| = 29.5)
  direct DFT (nfft 8192 and 4099):           e32 3.8e-06, device error 3.9e-06, bound 1.2e-05 .. 1.5e-05, worst error / bound 0.26
"""
import numpy as np
import pytest

import spectrogram_reference as SR
from nntoolkitcore_amd import capi
from nntoolkitcore_amd import layers as NL

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _check_spec(tag, got, ref, e32):
    assert got.shape == ref.shape and np.isfinite(got).all(), tag
    err, bound = float(np.abs(got.astype(np.float64) - ref).max()), SR.bound_spec(e32, ref)
    top = float(np.abs(ref).max())
    print("%s: spectrogram error %.3e of max, e32 %.3e, bound %.3e, ratio %.3f" % (tag, err / top, e32, bound / top, err / bound))
    assert err <= bound, (tag, err, bound)


def _check_logmel(tag, got, ref, e32):
    assert got.shape == ref.shape and np.isfinite(got).all(), tag
    err, bound = float(np.abs(got.astype(np.float64) - ref).max()), SR.bound_logmel(e32, ref)
    print("%s: log-mel error %.3e, e32 %.3e, bound %.3e, ratio %.3f" % (tag, err, e32, bound, err / bound))
    assert err <= bound, (tag, err, bound)


class _FrontEnd:
    """the case's Spectrogram handle (hann window) and, with mel, the LogMelSpectrogram over it"""

    def __init__(self, case, mel, input_size=None):
        self.sp = NL.Spectrogram(case.nfft, case.win, case.nov, case.N if input_size is None else input_size, mode=case.mode, fs=SR.FS,
                                 fft_norm=case.fft_norm, window_name="hann_window")
        self.lm = NL.LogMelSpectrogram(self.sp, case.n_mels, SR.FS, case.lo_hz, case.hi_hz) if mel else None
        self.top = self.lm or self.sp

    def one_shot(self, x):
        """the output buffer starts as NaN: an element the kernel does not store fails the comparison"""
        out = torch.full((x.shape[0],) + self.top.out_shape, float("nan"), device="cuda")
        self.top.apply_device(x, out=out)
        return out

    def destroy(self):
        if self.lm:
            self.lm.destroy()
        self.sp.destroy()


def _one_shot(case, mel):
    fe = _FrontEnd(case, mel)
    out = fe.one_shot(torch.tensor(SR.evaluate(case).x).cuda())
    fe.destroy()
    return out


# ------------------------------------------------------------------------------------------------- a. the 64 forms ---

def _pushes(case):
    """two or three ragged pushes per row, every row's pushes adding up to the case's input_size"""
    N, step = case.N, case.win - case.nov
    return [[N // 2, N - N // 2],                                   # (no frame boundary is a multiple of these)
            [case.win - 1, 2 * step + 1, N - case.win - 2 * step],   # no frame yet; then an odd frame held back
            [step + 3, N - step - 3]]


def _streamed(case, mel):
    x = SR.evaluate(case).x
    sched = _pushes(case)
    assert len(sched) == case.B and all(sum(s) == case.N and min(s) > 0 for s in sched)
    cap = max(max(s) for s in sched)
    fe = _FrontEnd(case, mel, input_size=cap)
    state = fe.top.new_stream_state(case.B)
    got, pos = [[] for _ in sched], [0] * case.B
    for i in range(max(len(s) for s in sched)):
        chunk = np.zeros((case.B, cap), np.float32)
        n_new, final = np.zeros(case.B, np.int32), np.zeros(case.B, np.int32)
        for b, s in enumerate(sched):
            if i < len(s):
                chunk[b, :s[i]] = x[b, pos[b]:pos[b] + s[i]]
                pos[b] += s[i]
                n_new[b], final[b] = s[i], int(i == len(s) - 1)
        out, cnt = fe.top.apply_device_stream(torch.from_numpy(chunk).cuda(), n_new, state, final=final)
        out = out.cpu().numpy()
        for b in range(case.B):
            got[b].append(out[b, :cnt[b]])
            assert not out[b, cnt[b]:].any(), "padding rows must be zeros"
    assert not state[1].any()
    fe.destroy()
    return [np.concatenate(g) for g in got]


@pytest.mark.parametrize("mel", [False, True], ids=["plain", "mel40"])
@pytest.mark.parametrize("case", SR.FORM_CASES, ids=lambda c: c.name)
def test_one_shot_form_matches_the_float64_reference(gpu, case, mel):
    res = SR.evaluate(case)
    got = _one_shot(case, mel).cpu().numpy()
    if mel:
        _check_logmel(case.name + "/mel", got, res.logmel, res.e32_logmel)
    else:
        _check_spec(case.name, got, res.spec, res.e32_spec)


@pytest.mark.parametrize("mel", [False, True], ids=["plain", "mel40"])
@pytest.mark.parametrize("case", SR.FORM_CASES, ids=lambda c: c.name)
def test_streamed_form_equals_its_one_shot_form_bit_for_bit(gpu, case, mel):
    one = _one_shot(case, mel).cpu().numpy()
    got = _streamed(case, mel)
    for b in range(case.B):
        assert got[b].shape == one[b].shape, (b, got[b].shape, one[b].shape)
        assert np.array_equal(got[b], one[b]), "row %d differs from the one-shot call" % b


@pytest.mark.parametrize("mel", [False, True], ids=["plain", "mel40"])
@pytest.mark.parametrize("case,ahead", SR.POISON_CASES, ids=lambda v: getattr(v, "name", str(v)))
def test_a_non_finite_sample_past_the_window_stays_out_of_the_pair(gpu, case, ahead, mel):
    """an inf / NaN sample that a pair's loads bring in but that belongs to neither of its frames: the pair stays finite and right (the
    kernel clears such samples with an AND; a product with the zero tap would be NaN).  Frames that hold the sample are non-finite, and
    take their pair partner with them -- nothing else."""
    x, spec, logmel, bad, pair_bad = SR.evaluate_poisoned(case, ahead)
    res = SR.evaluate(case)
    fe = _FrontEnd(case, mel)
    got = fe.one_shot(torch.tensor(x).cuda()).cpu().numpy()
    fe.destroy()
    got_bad = ~np.isfinite(got).all(-1)
    assert not (got_bad & ~pair_bad).any(), "a frame outside the poisoned pairs is not finite"
    assert (got_bad | ~bad).all(), "a frame whose window holds the sample is finite"
    if mel:
        _check_logmel(case.name + "/mel", got[~pair_bad], logmel[~pair_bad], res.e32_logmel)
    else:
        _check_spec(case.name, got[~pair_bad], spec[~pair_bad], res.e32_spec)


# --------------------------------------------------------------------------------------------- b. pairs per wave ---

@pytest.mark.parametrize("nts", SR.PPW_NTS)
def test_pairs_per_wave_only_move_pairs_between_waves(gpu, nts):
    case = SR.PPW_CASES[nts]
    res = SR.evaluate(case)
    x = torch.tensor(res.x).cuda()
    for mel in ([False, True] if case.n_mels else [False]):
        fe = _FrontEnd(case, mel)
        base = fe.one_shot(x)
        assert base.shape[1] == nts
        if mel:
            _check_logmel("%s/mel ppw auto" % case.name, base.cpu().numpy(), res.logmel, res.e32_logmel)
        else:
            _check_spec("%s ppw auto" % case.name, base.cpu().numpy(), res.spec, res.e32_spec)
        for ppw in SR.PPW_VALUES:
            capi.set_option("spec_ppw", ppw)
            out = fe.one_shot(x)
            capi.set_option("spec_ppw", "auto")
            assert torch.equal(out, base), "spec_ppw = %d changes the output (mel %s)" % (ppw, mel)
        fe.destroy()


# --------------------------------------------------------------------------------------------- c. row stride loop ---

def test_a_workgroup_that_takes_several_rows(gpu):
    """spec_ppw = 1 and 2048 rows of 33 pairs: a 9 x 1024 grid, every workgroup takes rows b and b + 1024"""
    case = SR.STRIDE_CASE
    res = SR.evaluate(case)
    nts = res.spec.shape[1]
    assert SR.route(case.nfft, case.win, case.nov, case.mode, case.fft_norm, True, False, B=case.B, nts=nts, ppw=1, n_mels=case.n_mels).gy < case.B
    x = torch.tensor(res.x).cuda()
    capi.set_option("spec_ppw", 1)
    fe = _FrontEnd(case, True)
    mel = fe.one_shot(x).cpu().numpy()
    plain = torch.full((case.B,) + fe.sp.out_shape, float("nan"), device="cuda")
    fe.sp.apply_device(x, out=plain)
    rows = plain[list(case.rows)].cpu().numpy()
    assert not bool(torch.isnan(plain).any())
    del plain
    capi.set_option("spec_ppw", "auto")
    fe.destroy()
    _check_spec(case.name, rows, res.spec, res.e32_spec)
    _check_logmel(case.name + "/mel", mel, res.logmel, res.e32_logmel)


# ---------------------------------------------------------------------------------------- d. fused-mel table limits ---

@pytest.mark.parametrize("case", SR.MEL_LIMIT_CASES, ids=lambda c: c.name)
def test_fused_mel_at_the_limits_of_its_tables(gpu, case):
    res = SR.evaluate(case)
    nts = res.spec.shape[1]
    fused = SR.route(case.nfft, case.win, case.nov, case.mode, case.fft_norm, True, False, B=case.B, nts=nts, n_mels=case.n_mels).fused
    assert fused == (case.n_mels <= 257)
    got = _one_shot(case, True).cpu().numpy()
    _check_logmel(case.name, got, res.logmel, res.e32_logmel)
    if fused:
        capi.set_option("spec_variant", 1)
        two = _one_shot(case, True).cpu().numpy()
        capi.set_option("spec_variant", "auto")
        print("%s: fused vs two-kernel form, max abs diff %.3e; two-kernel form vs reference %.3e" %
              (case.name, np.abs(two - got).max(), np.abs(two - res.logmel).max()))
        # (the tolerance of test_mel_filterbank_and_log_mel_spectrogram's fused-vs-two-kernel comparison)
        np.testing.assert_allclose(got, two, atol=2e-5, rtol=1e-5)


# ---------------------------------------------------------------------- e. the direct DFT above 4096, and its refusal ---

@pytest.mark.parametrize("case", SR.DIRECT_CASES, ids=lambda c: c.name)
def test_direct_dft_above_4096(gpu, case):
    res = SR.evaluate(case)
    assert res.kernel == "direct"
    _check_spec(case.name, _one_shot(case, False).cpu().numpy(), res.spec, res.e32_spec)


def test_direct_dft_refuses_a_window_that_does_not_fit(gpu):
    """a host-side check that returns before any launch: error code, message, output untouched"""
    R = SR.REFUSED
    assert SR.route(R["nfft"], R["win"], R["nov"], "magnitude", 1.0, False, False).kernel == "refused"
    sp = NL.Spectrogram(R["nfft"], R["win"], R["nov"], R["N"])
    assert sp.out_shape == (1, R["nfft"] // 2 + 1)
    x = torch.randn(1, R["N"], device="cuda")
    out = torch.full((1,) + sp.out_shape, 7.0, device="cuda")
    with pytest.raises(capi.NNTKError):
        sp.apply_device(x, out=out)
    torch.cuda.synchronize()
    assert "window too large" in capi.last_error()
    assert bool((out == 7.0).all())
    sp.destroy()
