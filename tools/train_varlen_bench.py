#!/usr/bin/env python3
"""Wall time of the ragged / carried-state training calls against the fixed-length ones (device-pointer forms, one forward + one
gradient call, each synchronised and timed on its own, with the kernels they ran): GRU(128->256) and LSTM(128->512), B = 64, T = 200 -- the shapes of tools/train_bench.py.
  (a) the VarLen calls with lengths = NULL and no states against the existing calls (same kernels: the difference must stay inside the
      baseline's own spread);
  (b) a ragged batch, rows sorted by length (16-row tiles homogeneous), lengths uniform in [T/4, T], with h0 / c0 in and d_h0 / d_c0
      out, against the full-length call.
The variants are alternated in one process; best of --reps (>= 5) after a warm-up.  usage: python tools/train_varlen_bench.py [--reps N]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from nntoolkitcore_amd import capi
    L = capi.load()
    torch.cuda.set_device(0)
    reps = max(5, int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 7)
    r = np.random.default_rng(0)
    u = lambda *s, sc=1.0: r.uniform(-sc, sc, s).astype(np.float32)
    dp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    sync = L.nntk_hip_synchronize
    B, T, n_in = 64, 200, 128
    for name, G, H in (("GRU(128->256)", 3, 256), ("LSTM(128->512)", 4, 512)):
        lstm = G == 4
        if lstm:
            cfg = L.LSTMConfigCreate(n_in, H, True, T, True, L.LSTMActivationsCreateDefault(H))
            h = L.LSTMCreateForTraining(cfg, capi.ConvTrainingConfig(B)); w = L.LSTMGetWeights(h).contents
            fwd0, bwd0, fwd1, bwd1, destroy = (L.LSTMApplyTrainingBatchDevice, L.LSTMCalculateGradientDevice,
                                               L.LSTMApplyTrainingBatchDeviceVarLen, L.LSTMCalculateGradientDeviceVarLen, L.LSTMDestroy)
        else:
            cfg = L.GRUConfigCreate(n_in, H, True, T, L.GRUActivationsCreateDefault(H))
            h = L.GRUCreateForTraining(cfg, capi.ConvTrainingConfig(B)); w = L.GRUGetWeights(h).contents
            fwd0, bwd0, fwd1, bwd1, destroy = (L.GRUApplyTrainingBatchDevice, L.GRUCalculateGradientDevice,
                                               L.GRUApplyTrainingBatchDeviceVarLen, L.GRUCalculateGradientDeviceVarLen, L.GRUDestroy)
        W = u(n_in * G * H + H * G * H + 2 * G * H, sc=0.05); C.memmove(w.W, W.ctypes.data, W.nbytes)
        xd, dd, yd = torch.from_numpy(u(B, T, n_in)).cuda(), torch.from_numpy(u(B, T, H)).cuda(), torch.empty(B, T, H, device="cuda")
        gd, gx = torch.zeros(W.size, device="cuda"), torch.empty(B, T, n_in, device="cuda")
        st = [torch.from_numpy(u(B, H, sc=0.5)).cuda() for _ in range(4)] + [torch.empty(B, H, device="cuda") for _ in range(4)]
        h0, c0, dhT, dcT, hT, cT, dh0, dc0 = st
        ln = np.sort(r.integers(T // 4, T + 1, B)).astype(np.int32)[::-1].copy()
        lp = ln.ctypes.data_as(capi.ip)

        def old():
            return (lambda: fwd0(h, dp(xd), dp(yd))), (lambda: bwd0(h, dp(gd), dp(gx), dp(dd)))

        def new(lengths, states):
            s = (h0, c0, hT, cT, dhT, dcT, dh0, dc0) if states else (None,) * 8
            if lstm:
                return ((lambda: fwd1(h, dp(xd), dp(yd), lengths, dp(s[0]), dp(s[1]), dp(s[2]), dp(s[3]))),
                        (lambda: bwd1(h, dp(gd), dp(gx), dp(dd), dp(s[4]), dp(s[5]), dp(s[6]), dp(s[7]))))
            return (lambda: fwd1(h, dp(xd), dp(yd), lengths, dp(s[0]), dp(s[2]))), (lambda: bwd1(h, dp(gd), dp(gx), dp(dd), dp(s[4]), dp(s[6])))

        full = np.full(B, T, np.int32)
        variants = (("existing calls", old()), ("VarLen, lengths NULL, no states", new(None, False)),
                    ("VarLen, all rows T, states", new(full.ctypes.data_as(capi.ip), True)),
                    ("VarLen, ragged sorted [T/4, T], states", new(lp, True)))
        times = {n: [] for n, _ in variants}                             # (forward, gradient, both) per repeat, each synchronised
        kern = {}
        for n, (f, g) in variants:                                       # warm-up
            assert f() == 0, capi.last_error()
            kf = L.nntk_hip_last_recurrent_kernel().decode()
            assert g() == 0, capi.last_error()
            kern[n] = kf + " / " + L.nntk_hip_last_recurrent_kernel().decode()
            assert sync() == 0
        for _ in range(reps):                                            # alternated
            for n, (f, g) in variants:
                t0 = time.perf_counter()
                rf = f(); sync()
                t1 = time.perf_counter()
                rg = g(); sync()
                t2 = time.perf_counter()
                times[n].append((t1 - t0, t2 - t1, t2 - t0))
                assert (rf, rg) == (0, 0), capi.last_error()
        base = np.array(times["existing calls"])[:, 2]
        print("%s B=%d T=%d, best of %d (mean length of the ragged batch %.0f)" % (name, B, T, reps, ln.mean()))
        for n, _ in variants:
            t = np.array(times[n]) * 1e3
            print("  %-40s forward %7.3f ms  gradient %7.3f ms  both: best %7.3f median %7.3f worst %7.3f  ratio to existing %.3f   [%s]" %
                  (n, t[:, 0].min(), t[:, 1].min(), t[:, 2].min(), np.median(t[:, 2]), t[:, 2].max(), t[:, 2].min() / (base.min() * 1e3), kern[n]))
        print("  baseline repeat-to-repeat spread: %.1f %%" % (100.0 * (base.max() - base.min()) / base.min()), flush=True)
        destroy(h)


if __name__ == "__main__":
    main()
