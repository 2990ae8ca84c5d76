"""Float64 restatement of the spectrogram / log-mel front end, the launch decision of spectrogram_launch, and the cases of
tests/test_gpu_spectrogram_matrix.py with their CPU yardsticks.  No GPU, no product library: numpy and the float32 oracle only.

The operation (signal/spectrogram.c:113-135, signal/log_mel_spectrogram.c:31-36): frame the signal with hop window - noverlap,
multiply by the window, zero-pad to nfft, DFT, multiply by fft_norm, then |X| / sum(w) (magnitude) or |X|^2 / (fs * sum(w^2)) with
the interior bins doubled and the two edge bins not (PSD); optionally spec @ W and log(x + eps).  The window taps and the mel weights
are the oracle's float32 values, so this reference differs from the device in arithmetic only.

evaluate(case) is cached: the host test and the GPU test of one process share one reference per case and never modify it.
"""
import collections
import functools
import zlib

import numpy as np

import oracle as O

FS = 16000
LOG_EPS = float(np.float32(1.5849e-13))       # log_mel_spectrogram.c:31-36, the constant as the float the reference holds
FACTOR = 4.0
FLOOR = 16 * 2.0 ** -24
U = 2.0 ** -24                                 # unit roundoff of float32


# ------------------------------------------------------------------------------------------------ float64 reference ---

def _frames(x, win, nov):
    step = win - nov
    nts = (x.shape[1] - nov) // step
    return np.arange(nts)[:, None] * step + np.arange(win)[None, :]


def spectrogram64(x, w, nfft, nov, mode="magnitude", fs=FS, fft_norm=1.0):
    """x [B, N], w [win] (float32 taps) -> float64 [B, nts, nfft // 2 + 1]"""
    x = np.atleast_2d(np.asarray(x, np.float64))
    w = np.asarray(w, np.float64)
    X = np.fft.rfft(x[:, _frames(x, w.size, nov)] * w, n=nfft, axis=-1) * float(np.float32(fft_norm))
    p = X.real ** 2 + X.imag ** 2
    if mode == "magnitude":
        return np.sqrt(p) / w.sum()
    p[..., 1:-1] *= 2.0
    return p / (fs * (w * w).sum())


def log_mel64(spec, W):
    W = np.asarray(W, np.float64)
    return np.log((spec.reshape(-1, W.shape[0]) @ W).reshape(spec.shape[:-1] + (W.shape[1],)) + LOG_EPS)


def direct_dft32(x, w, nfft, nov, mode="magnitude", fs=FS, fft_norm=1.0):
    """The direct DFT in float32, every sum left to right over the window's samples: re += frame[n] * cos, im += frame[n] * -sin with
    the float32 table exp(-2 pi i m / nfft) evaluated in double and rounded (the table a float32 implementation holds), then the
    reference's float32 finish.  Its error against spectrogram64 grows with the window length as any such sum's does."""
    x = np.atleast_2d(np.asarray(x, np.float32))
    w = np.asarray(w, np.float32)
    ph = -2.0 * np.pi * np.arange(nfft) / nfft
    tc, ts = np.cos(ph).astype(np.float32), np.sin(ph).astype(np.float32)
    fr = x[:, _frames(x, w.size, nov)] * w                        # float32 product
    nfreq = nfft // 2 + 1
    k = np.arange(nfreq)
    m = np.zeros(nfreq, np.int64)
    re = np.zeros(fr.shape[:2] + (nfreq,), np.float32)
    im = np.zeros_like(re)
    for n in range(w.size):
        f = fr[:, :, n, None]
        re += f * tc[m]
        im += f * ts[m]
        m = (m + k) % nfft
    nrm = np.float32(fft_norm)
    if nrm != 1:
        re, im = re * nrm, im * nrm
    p = re * re + im * im
    scale = np.float32(O.spectrogram_scale(w, mode, fs))
    if mode == "magnitude":
        return np.sqrt(p) / scale
    p[..., 1:-1] *= np.float32(2.0) / scale
    p[..., 0] /= scale
    p[..., -1] /= scale
    return p


# ------------------------------------------------------------------------------------- the launch decision, mirrored ---

Route = collections.namedtuple("Route", "kernel form fused gx gy")

# nntoolkitcore_amd/csrc/hip/spectrogram.hip, spectrogram_launch -- the constants below restate these lines:
MEL_MAX_FILTERS = 257        # "if (mel && n_mels > 257) return 1;"                       (the LDS tables of spectrogram512_kernel)
PPW_DIV, PPW_MIN, PPW_MAX = 4096, 4, 16      # "long ppw_l = (long)B * ppu / 4096; ... ppw_l < 4 ? 4 : ppw_l > 16 ? 16"
WAVES = 4                    # "unsigned gx = (ppu + 4 * ppw - 1) / (4 * ppw)": four wavefronts per workgroup
GY_MAX = 65535               # "unsigned gy = B < 65535 ? B : 65535"
GRID_MAX = 256 * 8 * 8       # "while ((long)gx * gy > 256L * 8 * 8 && gy > 1) gy = (gy + 1) / 2"
NZ7_LO, NZ7_HI = 384, 448    # "nz7 = window_size > 384 && window_size <= 448"
LD3_BYTES = 3072             # "ld3 = (step + window_size) * 4 <= 3072"
MIXED_MAX = 4096             # "nfft <= 4096 && mixed_plan(nfft, &plan)": radices 4, 2, 3, 5 only
DFT_LDS_BYTES = 64 * 1024    # "if (lds > 64 * 1024) return nntk_fail_msg(... window too large ...)", lds = window_size * 4


def _smooth235(n):
    if n < 2:
        return False
    for r in (2, 3, 5):
        while n % r == 0:
            n //= r
    return n == 1


def route(nfft, win, nov, mode, fft_norm, mel, stream, B=1, nts=1, ppw=0, n_mels=40):
    """Which kernel spectrogram_launch starts for this call.  kernel: "512" / "mixed" / "direct" / "refused"; form (512 only):
    (MODE, NORM, NZ7, NLD, MEL, ST); fused: the mel projection runs inside the kernel (otherwise the caller runs the two-kernel form
    and this is the route of its plain spectrogram launch); gx, gy: the grid of the 512 kernel (nts = the output's row stride, i.e.
    max_frames for a streaming call; ppw = the spec_ppw option, 0 = automatic)."""
    step = win - nov
    fused = bool(mel) and nfft == 512 and n_mels <= MEL_MAX_FILTERS
    if nfft == 512:
        ppu = (nts + 1) // 2
        auto = B * ppu // PPW_DIV
        p = ppw if ppw > 0 else min(max(auto, PPW_MIN), PPW_MAX)
        gx = (ppu + WAVES * p - 1) // (WAVES * p)
        gy = min(B, GY_MAX)
        while gx * gy > GRID_MAX and gy > 1:
            gy = (gy + 1) // 2
        form = (1 if mode == "psd" else 0, bool(np.float32(fft_norm) != np.float32(1.0)), NZ7_LO < win <= NZ7_HI,
                3 if (step + win) * 4 <= LD3_BYTES else 4, fused, bool(stream))
        return Route("512", form, fused, gx, gy)
    if nfft <= MIXED_MAX and _smooth235(nfft):
        return Route("mixed", None, False, None, None)
    if win * 4 > DFT_LDS_BYTES:
        return Route("refused", None, False, None, None)
    return Route("direct", None, False, None, None)


def pairs_per_wave(nts, gx):
    """frame pairs each of the 4 * gx wavefronts of one row walks: wave i takes pairs i, i + 4 gx, ... (pr = blockIdx.x * 4 + wave;
    pr += gridDim.x * 4)"""
    ppu = (nts + 1) // 2
    return [len(range(i, ppu, WAVES * gx)) for i in range(WAVES * gx)]


ALL_FORMS = frozenset((m, n, z, l, e, s) for m in (0, 1) for n in (False, True) for z in (False, True) for l in (3, 4)
                      for e in (False, True) for s in (False, True))


# -------------------------------------------------------------------------------------------------------- the cases ---

# name: what the GPU test calls it; rows: the rows whose plain spectrogram is compared (None = all); n_mels = 0: no log-mel form
Case = collections.namedtuple("Case", "name nfft win nov N B mode fft_norm n_mels lo_hz hi_hz rows")


def _case(name, nfft, win, nov, N, B, mode="magnitude", fft_norm=1.0, n_mels=0, lo_hz=0.0, hi_hz=8000.0, rows=None):
    return Case(name, nfft, win, nov, N, B, mode, float(fft_norm), n_mels, float(lo_hz), float(hi_hz), rows)


# a. the 64 forms.  window, noverlap, input_size (odd, odd frame count 5..9), and the (NZ7, NLD) the geometry stands for
GEOMETRIES = [(400, 240, 1437, True, 3), (448, 0, 2371, True, 4), (320, 160, 1651, False, 3), (512, 128, 2349, False, 4)]
FORM_MELS = 40


def form_name(mode, norm, win, nov):
    return "%s_norm%g_w%d_o%d" % (mode, norm, win, nov)


FORM_CASES = [_case(form_name(mode, norm, win, nov), 512, win, nov, N, 3, mode, norm, FORM_MELS)
              for mode in ("magnitude", "psd") for norm in (1.0, 0.5) for (win, nov, N, _, _) in GEOMETRIES]
FORM_EXPECT = {form_name(mode, norm, win, nov): (1 if mode == "psd" else 0, norm != 1.0, nz7, nld)
               for mode in ("magnitude", "psd") for norm in (1.0, 0.5) for (win, nov, _, nz7, nld) in GEOMETRIES}

# b. pairs per wave
PPW_NTS = (1, 2, 3, 45, 98)
PPW_VALUES = (1, 2, 3, 16)
PPW_CASES = {nts: _case("ppw_nts%d" % nts, 512, 400, 240, 240 + 160 * nts + 3, 2, n_mels=40 if nts == 45 else 0) for nts in PPW_NTS}

# c. the row stride loop
STRIDE_ROWS = (0, 1, 1023, 1024, 2047)
STRIDE_CASE = _case("row_stride", 512, 64, 48, 48 + 16 * 66 + 5, 2048, n_mels=13, rows=STRIDE_ROWS)

# d. the fused mel tables at their limits
MEL_LIMIT_CASES = [_case("mels%d" % n, 512, 400, 240, 240 + 160 * 7 + 77, 2, n_mels=n) for n in (200, 256, 257, 258)] + \
                  [_case("mels128_narrow", 512, 400, 240, 240 + 160 * 7 + 77, 2, n_mels=128, lo_hz=300.0, hi_hz=3400.0)]

# e. the direct DFT above 4096
DIRECT_CASES = [_case("direct8192", 8192, 6000, 0, 16384, 1, "magnitude", 0.5),
                _case("direct4099", 4099, 4099, 2000, 9000, 2, "psd", 1.0)]
REFUSED = dict(nfft=16400, win=16390, nov=0, N=16390 + 20)      # 16390 * 4 bytes > 64 KiB; 16400 > 4096 takes the direct route

# f. a non-finite sample that a pair loads but that lies outside both of its frames' windows (spectrogram.hip: "out-of-window samples
# are ANDed away, not multiplied by 0").  A pair's 16-byte loads cover samples [0, step + window) of the pair, rounded up to four; frame
# B's window ends at step + window, so the sample at pair start + step + window reaches the kernel's registers only when step + window
# is no multiple of four (everything further on is never loaded: those lanes read zeros; and frame A's samples past its window lie
# inside frame B's).  At window 400, hop 160 no sample can tell an AND from a product with the zero tap; these two geometries can:
#   NZ7 (window 401, hop 161): the loads bring samples 562 and 563, register row 6 holds them (lanes 17, 18);
#   all rows masked (window 300, hop 263): the loads bring sample 563, register row 4 holds it.
POISON_CASES = [(_case("poison_w401_o240", 512, 401, 240, 240 + 161 * 7 + 50, 3, "magnitude", 1.0, 40), 0),
                (_case("poison_w300_o37", 512, 300, 37, 37 + 263 * 5 + 45, 3, "psd", 0.5, 40), 0)]

ALL_CASES = FORM_CASES + list(PPW_CASES.values()) + [STRIDE_CASE] + MEL_LIMIT_CASES + DIRECT_CASES + [c for c, _ in POISON_CASES]


def poison_positions(case, ahead):
    """(row, sample, value): row 1 gets +inf just past frame 1 (pair 0), row 2 a NaN just past frame 3 (pair 1); row 0 stays clean"""
    step = case.win - case.nov
    return [(1, step + case.win + ahead, np.inf), (2, 2 * step + step + case.win + ahead, np.nan)]


@functools.lru_cache(maxsize=None)
def evaluate_poisoned(case, ahead):
    """(x, spec, logmel, bad, pair_bad): the case's input with the samples of poison_positions, its float64 reference, the frames whose
    window holds such a sample (bad, [B, nts]) and those that share a frame pair (2p, 2p + 1) with one (pair_bad)"""
    x = evaluate(case).x.copy()
    for b, q, v in poison_positions(case, ahead):
        x[b, q] = v
    with np.errstate(all="ignore"):
        spec = spectrogram64(x, O.window("hann", case.win), case.nfft, case.nov, mode=case.mode, fs=FS, fft_norm=case.fft_norm)
        logmel = log_mel64(spec, O.mel_filterbank_weights(case.n_mels, case.nfft, FS, case.lo_hz, case.hi_hz))
    bad = ~np.isfinite(spec).all(-1)
    pair_bad = bad.copy()
    nts = bad.shape[1]
    for t in range(nts):
        mate = t ^ 1
        if mate < nts:
            pair_bad[:, t] |= bad[:, mate]
    for a in (x, spec, logmel, bad, pair_bad):
        a.setflags(write=False)
    return x, spec, logmel, bad, pair_bad


Result = collections.namedtuple("Result", "x spec e32_spec logmel e32_logmel kernel o32_spec o32_logmel yard_rows")


def bound_spec(e32, ref):
    """largest allowed |device - ref| on a spectrogram"""
    return max(FACTOR * e32, FLOOR) * float(np.abs(ref).max())


def bound_logmel(e32, ref):
    """largest allowed |device - ref| on a log-mel output"""
    return max(FACTOR * e32, FLOOR * max(1.0, float(np.abs(ref).max())))


@functools.lru_cache(maxsize=None)
def evaluate(case):
    """The case's input (float32 [B, N]), its float64 reference and the float32 CPU yardstick.
    spec [len(rows) or B, nts, nfreq] and logmel [B, nts, n_mels] (None without a mel form) are the float64 reference.
    The float32 CPU evaluation is the oracle (kissfft) on the 512 and mixed-radix routes and direct_dft32 on the direct route; it runs
    on yard_rows -- every row, or, where the case names the rows it compares, those rows and every eighth row (the oracle is the slow
    part of a 2048-row case): o32_spec [like spec], o32_logmel [len(yard_rows), nts, n_mels],
    e32_spec = max |o32_spec - spec| / max |spec|, e32_logmel = max |o32_logmel - logmel[yard_rows]|."""
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    x = (0.1 * rng.standard_normal((case.B, case.N))).astype(np.float32)
    w = O.window("hann", case.win)
    kernel = route(case.nfft, case.win, case.nov, case.mode, case.fft_norm, False, False).kernel
    W = O.mel_filterbank_weights(case.n_mels, case.nfft, FS, case.lo_hz, case.hi_hz) if case.n_mels else None
    rows = list(range(case.B)) if case.rows is None else sorted(case.rows)
    yard = rows if W is None else sorted(set(rows) | set(range(0, case.B, 8)))
    kw = dict(mode=case.mode, fs=FS, fft_norm=case.fft_norm)
    f32 = direct_dft32 if kernel == "direct" else O.spectrogram
    spec, lm = [], []
    for r0 in range(0, case.B, 128):                     # the float64 spectrogram of 2048 rows is not held at once
        sel = [r for r in range(r0, min(r0 + 128, case.B)) if W is not None or r in rows]
        if not sel:
            continue
        s64 = spectrogram64(x[sel], w, case.nfft, case.nov, **kw)
        if W is not None:
            lm.append(log_mel64(s64, W))
        spec.append(s64[[i for i, r in enumerate(sel) if r in rows]])
    spec = np.concatenate(spec)
    s32 = f32(x[yard], w, case.nfft, case.nov, **kw)
    o32 = s32[[i for i, r in enumerate(yard) if r in rows]]
    e32 = float(np.abs(o32 - spec).max() / np.abs(spec).max())
    if W is None:
        res = Result(x, spec, e32, None, None, kernel, o32, None, yard)
    else:
        lm = np.concatenate(lm)
        lm32 = np.stack([O.log_mel(s, W) for s in s32])
        res = Result(x, spec, e32, lm, float(np.abs(lm32 - lm[yard]).max()), kernel, o32, lm32, yard)
    for a in res:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)      # shared between tests
    return res
