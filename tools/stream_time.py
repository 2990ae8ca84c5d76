#!/usr/bin/env python3
"""Time the streaming stack (nntoolkitcore_amd.streaming.StreamingStack) on the cfg-5 shape: Spectrogram 512/400/240 -> Conv1d
257->128 k5 + BN + ReLU -> LSTM 128->512 -> TimeDistributedDense 512->1000.

  python tools/stream_time.py                 per-push time for B in {64, 512} x chunks of 10 / 40 / 160 ms (16 kHz), and 10 s of audio
                                              streamed in 160 ms chunks against the one-shot per-layer chain on the same audio
  python tools/stream_time.py --profile       only a few 160 ms pushes at B = 512 (run under rocprofv3 --kernel-trace --stats)
  python tools/stream_time.py --stats FILE    share of the stream-only passes (gather, zero padding, count upload) in a
                                              rocprofv3 kernel_stats.csv
"""
import argparse
import csv

import numpy as np
import torch

from timing import open_device, timed
from nntoolkitcore_amd import layers as NL

STREAM_ONLY = ("stream_gather_kernel", "varlen_zero_pad_kernel", "upload_ints_kernel")


def build(B, chunk, rng, T_one=None):
    from nntoolkitcore_amd.streaming import StreamingStack
    u = lambda *s, sc=1.0: rng.uniform(-sc, sc, s).astype(np.float32)
    spec = NL.Spectrogram(512, 400, 240, chunk)
    T = spec.stream_sizes()[1]
    conv = NL.Conv1d(257, 128, 5, 1, T)
    conv.set_weights(u(128, 257, 5, sc=(257 * 5) ** -0.5), u(128, sc=0.1))
    bn = NL.BatchNorm(128, 1e-3, 1)
    bn.set_weights(1 + u(128, sc=.5), u(128, sc=.5), u(128, sc=.1), 1 + np.abs(u(128, sc=.5)))
    relu = NL.Activation("relu", 1, 1.0)
    T = conv.stream_sizes()[1]
    w = (u(128, 2048, sc=128 ** -0.5), u(512, 2048, sc=512 ** -0.5), u(2048, sc=.1), u(2048, sc=.1))
    lstm = NL.LSTM(128, 512, True, T, v2=True)
    lstm.set_weights(*w)
    dw = (u(512, 1000, sc=512 ** -0.5), u(1000, sc=.1))
    tdd = NL.TimeDistributedDense(T, 512, 1000)
    tdd.set_weights(*dw)
    return StreamingStack(spec, [(conv, bn, relu)], [lstm], head=tdd, batch=B), (conv, bn, relu, w, dw)


def time_ms(fn, n, warm=3):
    return timed(fn, 1, warmup=warm, inner=n).median


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--stats")
    a = ap.parse_args()
    if a.stats:
        rows = list(csv.DictReader(open(a.stats)))
        tot = sum(float(r["TotalDurationNs"]) for r in rows)
        so = sum(float(r["TotalDurationNs"]) for r in rows if any(k in r["Name"] for k in STREAM_ONLY))
        for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
            print("%-70s %8s calls %10.3f ms %5.1f %%" % (r["Name"][:70], r["Calls"], float(r["TotalDurationNs"]) / 1e6,
                                                        100 * float(r["TotalDurationNs"]) / tot))
        print("stream-only passes (%s): %.2f %% of the GPU time" % (", ".join(STREAM_ONLY), 100 * so / tot))
        return
    open_device()
    rng = np.random.default_rng(0)
    if a.profile:
        B, chunk = 512, 2560
        st, _ = build(B, chunk, rng)
        x = torch.from_numpy((0.1 * rng.standard_normal((B, chunk))).astype(np.float32)).cuda()
        n = np.full(B, chunk, np.int32)
        for _ in range(12):
            st.push(x, n)
        torch.cuda.synchronize()
        print("profiled 12 pushes of 160 ms at B = 512")
        return
    for B in (64, 512):
        for chunk in (160, 640, 2560):
            st, _ = build(B, chunk, rng)
            x = torch.from_numpy((0.1 * rng.standard_normal((B, chunk))).astype(np.float32)).cuda()
            n = np.full(B, chunk, np.int32)
            ms = time_ms(lambda: st.push(x, n), 20)
            print("B %4d  chunk %4d samples (%3d ms): %.3f ms per push, %.1f x real time" % (B, chunk, chunk // 16, ms, chunk / 16 / ms))
    # 10 s of audio: streamed in 160 ms chunks vs the one-shot per-layer chain
    N = 160000
    for B in (64, 512):
        audio = torch.from_numpy((0.1 * rng.standard_normal((B, N))).astype(np.float32)).cuda()
        st, (conv_s, bn, relu, w, dw) = build(B, 2560, rng)
        # 160 ms chunks: the stack's input rows are always 2560 samples wide; the last chunk brings the remaining 1280
        nch = -(-N // 2560)
        padded = torch.zeros((B, nch * 2560), device="cuda")
        padded[:, :N] = audio
        chunks = [(padded[:, i * 2560:(i + 1) * 2560].contiguous(), np.full(B, min(2560, N - i * 2560), np.int32)) for i in range(nch)]

        def stream():
            st.reset(np.arange(B))
            for i, (c, n) in enumerate(chunks):
                st.push(c, n, final=np.ones(B, np.int32) if i == nch - 1 else None)
        spec = NL.Spectrogram(512, 400, 240, N)
        F = spec.out_shape[0]
        conv = NL.Conv1d(257, 128, 5, 1, F)
        conv.set_weights(rng.uniform(-.03, .03, (128, 257, 5)).astype(np.float32), np.zeros(128, np.float32))     # (timing only)
        lstm = NL.LSTM(128, 512, True, F - 4, v2=True)
        lstm.set_weights(*w)
        tdd = NL.TimeDistributedDense(F - 4, 512, 1000)
        tdd.set_weights(*dw)

        def one_shot():
            tdd.apply_device(lstm.apply_device(conv.apply_device(spec.apply_device(audio), bn=bn, act=relu)))
        ts, to = time_ms(stream, 2, warm=1), time_ms(one_shot, 2, warm=1)
        print("B %4d  10 s of audio: streamed in 160 ms chunks %.1f ms, one-shot chain %.1f ms (%.2f x)" % (B, ts, to, ts / to))


if __name__ == "__main__":
    main()
