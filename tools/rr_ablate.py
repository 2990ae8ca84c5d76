#!/usr/bin/env python3
"""Diagnostics build only (tools/build_variant.sh <lib> -DNNTK_RR_DBG; NNTK_LIB=<lib>, one library per compile-time mask: tools/rr_ablate.sh): time lstm_rr_kernel at the stack's
LSTM shape with parts of the half-step removed (WRONG results, timing only).  usage: rr_ablate.py [B] [T]"""
import sys
import torch
from timing import open_device, timed
import bench
from nntoolkitcore_amd import layers as NL


def main():
    open_device()
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    B, T = 512, 996
    w = bench.make_weights("stack", 3)
    lstm = NL.LSTM(128, 512, True, T, v2=True)
    lstm.set_weights(w["lstm_W"], w["lstm_U"], w["lstm_bi"], w["lstm_bh"])
    x = torch.randn(B, T, 128, device="cuda"); h = torch.empty(B, T, 512, device="cuda")
    names = {1: "no operand loads", 2: "no finish", 4: "no arrive/poll", 8: "no x", 16: "no MFMA", 32: "no partial writes"}
    ms = timed(lambda: lstm.apply_device(x, out=h), 1, warmup=3, inner=5).median
    print("dbg %3d: %.3f ms = %.2f us/step   [%s]" % (m, ms, ms * 1e3 / T, ", ".join(v for k, v in names.items() if m & k) or "everything"), flush=True)
    lstm.destroy()


if __name__ == "__main__":
    main()
