#!/usr/bin/env python3
"""Times the bidirectional training pair (*BidirectionalApplyTrainingBatchDevice + *BidirectionalCalculateGradientDevice) against the same
recipe composed from the public device calls: bd_reverse_input_batch_device, *ApplyTrainingBatchDeviceVarLen twice,
bd_reverse_backward_batch_device, bd_merge_concat_device | bd_merge_gradient_varlen_device, *CalculateGradientDeviceVarLen twice,
bd_accumulate_d_x_varlen_device -- on twin handles with the same weights.  Device pointers, torch events around a whole forward + gradient
pair, warm-up first, the two variants alternating inside every round; the outputs, d_X and the gradient blocks of both are compared in the
same run.  Then the share of the pair's time spent in the three new kernels: the tool first (before it opens the GPU itself) starts one child process of itself
(`--pair-only N`) under `rocprofv3 --kernel-trace --stats`, reads the kernel statistics it leaves and divides the per-pair device time of bd_merge_kernel +
bd_scatter_kernel + bd_accumulate_kernel by the per-pair device time of all kernels (and by the event-timed median above).  `--no-share`
skips that step.
usage: python tools/bd_train_time.py [--rounds N] [--pair-only N] [--no-share] [cell:in:H:T:B]     default lstm:128:512:200:64, lengths all T"""
import csv
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch
from timing import open_device, timed
from nntoolkitcore_amd import capi, layers as NL


NEW_KERNELS = ("bd_merge_kernel", "bd_scatter_kernel", "bd_accumulate_kernel")


def kernel_trace(spec, pairs):
    """one traced child run of `pairs` pairs, started before this process opens the GPU: (per-kernel lines, device time of the new kernels
    per pair, device time of all kernels per pair) in ms, or None when the trace failed"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--pair-only", str(pairs), spec]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if res.returncode != 0 or not files:
            print("kernel trace failed (exit %d): the share is NOT measured\n%s" % (res.returncode, res.stdout[-2000:]))
            return None
        rows = list(csv.DictReader(open(files[0])))
    name_key = next(k for k in rows[0] if k.lower() == "name")
    total_key = next(k for k in rows[0] if k.lower().startswith("totalduration"))
    calls_key = next(k for k in rows[0] if k.lower() == "calls")
    lines, new_ns = [], 0.0
    for r_ in rows:
        if any(k in r_[name_key] for k in NEW_KERNELS):
            new_ns += float(r_[total_key])
            lines.append("  %-60s %4d calls  %9.1f us per pair" % (r_[name_key][:60], int(r_[calls_key]), float(r_[total_key]) / pairs / 1e3))
    return lines, new_ns / pairs / 1e6, sum(float(r_[total_key]) for r_ in rows) / pairs / 1e6


def main():
    rounds, pair_only, share, spec = 15, 0, True, "lstm:128:512:200:64"
    args = sys.argv[1:]
    while args:
        if args[0] == "--rounds":
            rounds, args = int(args[1]), args[2:]
        elif args[0] == "--pair-only":
            pair_only, args = int(args[1]), args[2:]
        elif args[0] == "--no-share":
            share, args = False, args[1:]
        else:
            spec, args = args[0], args[1:]
    trace = kernel_trace(spec, 10) if share and not pair_only else None
    L = open_device()
    f = spec.split(":")
    kind, I, H, T, B = f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4])
    G = {"lstm": 4, "gru": 3, "rnn": 1}[kind]
    cls = {"lstm": NL.LSTM, "gru": NL.GRU, "rnn": NL.RNN}[kind]
    pre = kind.upper()
    r = np.random.default_rng(5)
    u = lambda *sh, sc=1.0: r.uniform(-sc, sc, sh).astype(np.float32)
    weights = [(u(I, G * H, sc=I ** -0.5), u(H, G * H, sc=H ** -0.5), u(G * H, sc=0.1), u(G * H, sc=0.1)) for _ in range(2)]
    pair = [cls(I, H, True, T, mini_batch=B) for _ in range(2)]
    twin = [cls(I, H, True, T, mini_batch=B) for _ in range(2)]
    for lay, w in zip(pair + twin, weights + weights):
        lay.set_weights(*w)
    nblk = I * G * H + H * G * H + 2 * G * H
    dp = NL._dp
    nul = (None,) * (4 if kind == "lstm" else 2)
    x, dout = torch.randn(B, T, I, device="cuda"), torch.randn(B, T, 2 * H, device="cuda")
    cfg = capi.RecurrentConfig(I, H, True, T)
    fwd_vl, grad_vl = getattr(L, pre + "ApplyTrainingBatchDeviceVarLen"), getattr(L, pre + "CalculateGradientDeviceVarLen")
    ok = lambda rc: capi.check(rc, "bd_train_time")

    class Bufs:
        def __init__(self):
            self.out, self.dX = torch.empty(B, T, 2 * H, device="cuda"), torch.empty(B, T, I, device="cuda")
            self.gf, self.gb = torch.zeros(nblk, device="cuda"), torch.zeros(nblk, device="cuda")

    a, b = Bufs(), Bufs()
    xr, dxf, dxb = (torch.empty(B, T, I, device="cuda") for _ in range(3))
    of, obr, ob, dof, dob = (torch.empty(B, T, H, device="cuda") for _ in range(5))

    def composed():
        a.gf.zero_(); a.gb.zero_()
        ok(L.bd_reverse_input_batch_device(dp(x), dp(xr), cfg, B))
        ok(fwd_vl(twin[0].h, dp(x), dp(of), None, *nul)); ok(fwd_vl(twin[1].h, dp(xr), dp(obr), None, *nul))
        ok(L.bd_reverse_backward_batch_device(dp(obr), dp(ob), cfg, B))
        ok(L.bd_merge_concat_device(dp(of), dp(ob), dp(a.out), cfg, B))
        ok(L.bd_merge_gradient_varlen_device(dp(dout), dp(dof), dp(dob), cfg, B, None, 0))
        ok(grad_vl(twin[0].h, dp(a.gf), dp(dxf), dp(dof), *nul)); ok(grad_vl(twin[1].h, dp(a.gb), dp(dxb), dp(dob), *nul))
        ok(L.bd_accumulate_d_x_varlen_device(dp(dxf), dp(dxb), dp(a.dX), cfg, B, None))

    def one_call():
        b.gf.zero_(); b.gb.zero_()
        NL.bidirectional_train_forward_device(pair[0], pair[1], x, out=b.out)
        NL.bidirectional_train_backward_device(pair[0], pair[1], dout, b.gf, b.gb, dX=b.dX)

    if pair_only:
        for _ in range(pair_only):
            one_call()
        torch.cuda.synchronize()
        print("ran the pair %d times" % pair_only)
        return 0

    variants = {"a composed": composed, "b one call per pass": one_call}
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    same = all(torch.equal(p, q) for p, q in ((a.out, b.out), (a.dX, b.dX), (a.gf, b.gf), (a.gb, b.gb)))
    ts = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            ts[name].append(timed(fn, 1, warmup=0).median)
    print("%s B=%d, lengths all T, forward + gradient; identical output / d_X / gradient blocks: %s" % (spec, B, same))
    base = np.median(ts["a composed"])
    for name in variants:
        v = np.array(ts[name])
        print("  %-20s med %8.3f ms  min %8.3f  max %8.3f  = %.3f x (a)" % (name, np.median(v), v.min(), v.max(), np.median(v) / base), flush=True)
    for lay in pair + twin:
        lay.destroy()
    if not share:
        return 0 if same else 1
    if trace is None:
        return 1
    lines, new_ms, all_ms = trace
    pair_ms = float(np.median(ts["b one call per pass"]))
    print("\n".join(lines))
    print("  new kernels: %.1f us per pair = %.4f of the device time of all kernels of a pair (%.3f ms, traced run) = %.4f of the pair's "
          "event-timed median (%.3f ms)" % (1e3 * new_ms, new_ms / all_ms, all_ms, new_ms / pair_ms, pair_ms))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
