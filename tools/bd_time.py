#!/usr/bin/env python3
"""Times the one-call bidirectional layer (*BidirectionalApplyDevice) against the composed recipe it replaces on the GPU (device
pointers, torch events, warm-up first; the two variants alternate inside every round so that clock and power drift spread over both), and
checks in the same run that both give identical outputs:
  (a) composed: bd_reverse_*_device, *ApplyDevice[VarLen] twice, bd_reverse of the backward output, bd_merge_concat_device -- five calls
  (b) fused:    *BidirectionalApplyDevice -- one pack pass, one launch of both directions
Each shape runs with every length T and with ragged lengths (uniform in [T/2, T]).
usage: python tools/bd_time.py [--rounds N] [--batches 64,256,...] cell:in:H:T ...
default: gru:128:256:1000 gru:256:256:1000 lstm:128:512:996 at B = 64, 256, 512, 1024"""
import sys
import numpy as np
import torch
from timing import open_device, timed
from nntoolkitcore_amd import capi, layers as NL


def main():
    L = open_device()
    rounds, batches = 7, [64, 256, 512, 1024]
    args = sys.argv[1:]
    while args and args[0].startswith("--"):
        if args[0] == "--rounds":
            rounds = int(args[1])
        elif args[0] == "--batches":
            batches = [int(b) for b in args[1].split(",")]
        args = args[2:]
    r = np.random.default_rng(5)
    u = lambda *sh, sc=1.0: r.uniform(-sc, sc, sh).astype(np.float32)
    ok = True
    for spec in args or ["gru:128:256:1000", "gru:256:256:1000", "lstm:128:512:996"]:
        f = spec.split(":")
        kind, I, H, T = f[0], int(f[1]), int(f[2]), int(f[3])
        G = 4 if kind == "lstm" else 3
        mk = (lambda: NL.LSTM(I, H, True, T, v2=True)) if kind == "lstm" else (lambda: NL.GRU(I, H, True, T))
        fwd, bwd = mk(), mk()
        for lay in (fwd, bwd):
            lay.set_weights(u(I, G * H, sc=I ** -0.5), u(H, G * H, sc=H ** -0.5), u(G * H, sc=0.1), u(G * H, sc=0.1))
        for B in batches:
            x = torch.randn(B, T, I, device="cuda")
            of, obr, ob = (torch.empty(B, T, H, device="cuda") for _ in range(3))
            xr = torch.empty_like(x)
            out_a, out_b = (torch.empty(B, T, 2 * H, device="cuda") for _ in range(2))
            cfg_in, cfg_out = capi.RecurrentConfig(I, I, True, T), capi.RecurrentConfig(H, H, True, T)
            for lens in (None, r.integers(T // 2, T + 1, B).astype(np.int32)):
                lp = None if lens is None else lens.ctypes.data_as(capi.ip)

                def composed():
                    if lens is None:
                        L.bd_reverse_input_batch_device(NL._dp(x), NL._dp(xr), cfg_in, B)
                        fwd.apply_device(x, out=of); bwd.apply_device(xr, out=obr)
                        L.bd_reverse_backward_batch_device(NL._dp(obr), NL._dp(ob), cfg_out, B)
                    else:
                        L.bd_reverse_input_batch_varlen_device(NL._dp(x), NL._dp(xr), cfg_in, B, lp)
                        fwd.apply_device_varlen(x, lengths=lens, out=of); bwd.apply_device_varlen(xr, lengths=lens, out=obr)
                        L.bd_reverse_backward_batch_varlen_device(NL._dp(obr), NL._dp(ob), cfg_out, B, lp)
                    L.bd_merge_concat_device(NL._dp(of), NL._dp(ob), NL._dp(out_a), cfg_out, B)

                variants = {"a composed": composed,
                            "b fused": lambda: NL.bidirectional_apply_device(fwd, bwd, x, lengths=lens, out=out_b)}
                kernels = {}
                for name, fn in variants.items():          # warm-up: every variant twice
                    for _ in range(2):
                        fn()
                    torch.cuda.synchronize()
                    kernels[name] = L.nntk_hip_last_recurrent_kernel().decode()
                same = torch.equal(out_a, out_b)
                ok &= same
                ts = {name: [] for name in variants}
                for _ in range(rounds):
                    for name, fn in variants.items():
                        ts[name].append(timed(fn, 1, warmup=0).median)
                a = np.median(ts["a composed"])
                print("%s B=%d %s  identical outputs: %s" % (spec, B, "all T" if lens is None else "ragged (mean %.3f T)" % (lens.mean() / T),
                                                            same))
                for name in variants:
                    v = np.array(ts[name])
                    print("  %-11s %-28s med %8.3f ms  min %8.3f  max %8.3f  = %.3f x (a)" % (name, kernels[name], np.median(v), v.min(),
                                                                                       v.max(), np.median(v) / a), flush=True)
            del x, of, obr, ob, xr, out_a, out_b
            torch.cuda.empty_cache()
        fwd.destroy(); bwd.destroy()
    print("all outputs identical" if ok else "OUTPUTS DIFFER")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
