#!/usr/bin/env python3
"""Times the *ApplyDeviceVarLen calls against *ApplyDevice on the GPU (device pointers, torch events, warm-up first; the variants
alternate inside every round so that clock and power drift spread over all of them):
  (a) *ApplyDevice   (b) VarLen, every length T   (c) lengths uniform in [T/2, T], sorted descending   (d) the same lengths unsorted
usage: python tools/varlen_time.py [--rounds N] cell:in:H:B:T ...   default: gru:128:256:1024:1000 gru:256:256:1024:1000 lstm:128:512:512:996"""
import sys
import numpy as np
import torch
from timing import open_device, timed
from nntoolkitcore_amd import layers as NL


def main():
    L = open_device()
    rounds = 7
    args = sys.argv[1:]
    if args and args[0] == "--rounds":
        rounds = int(args[1]); args = args[2:]
    r = np.random.default_rng(5)
    u = lambda *sh, sc=1.0: r.uniform(-sc, sc, sh).astype(np.float32)
    for spec in args or ["gru:128:256:1024:1000", "gru:256:256:1024:1000", "lstm:128:512:512:996"]:
        f = spec.split(":")
        kind, I, H, B, T = f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4])
        G = 4 if kind == "lstm" else 3
        lay = NL.LSTM(I, H, True, T, v2=True) if kind == "lstm" else NL.GRU(I, H, True, T)
        lay.set_weights(u(I, G * H, sc=I ** -0.5), u(H, G * H, sc=H ** -0.5), u(G * H, sc=0.1), u(G * H, sc=0.1))
        x = torch.randn(B, T, I, device="cuda"); h = torch.empty(B, T, H, device="cuda")
        ragged = r.integers(T // 2, T + 1, B).astype(np.int32)
        variants = {
            "a ApplyDevice": lambda: lay.apply_device(x, out=h),
            "b VarLen all T": lambda: lay.apply_device_varlen(x, lengths=np.full(B, T, np.int32), out=h),
            "c VarLen sorted": lambda: lay.apply_device_varlen(x, lengths=np.sort(ragged)[::-1], out=h),
            "d VarLen unsorted": lambda: lay.apply_device_varlen(x, lengths=ragged, out=h),
        }
        kernels = {}
        for name, fn in variants.items():          # warm-up: every variant twice
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            kernels[name] = L.nntk_hip_last_recurrent_kernel().decode()
        ts = {name: [] for name in variants}
        for _ in range(rounds):
            for name, fn in variants.items():
                ts[name].append(timed(fn, 1, warmup=0).median)
        a = np.median(ts["a ApplyDevice"])
        print("%s  mean length of (c)/(d): %.3f T" % (spec, ragged.mean() / T))
        for name in variants:
            v = np.array(ts[name])
            print("  %-18s %-26s med %8.3f ms  min %8.3f  max %8.3f  = %.3f x (a)" % (name, kernels[name], np.median(v), v.min(), v.max(),
                                                                                   np.median(v) / a), flush=True)
        lay.destroy()


if __name__ == "__main__":
    main()
