#!/usr/bin/env python
"""Time one nntk_optimizer_step_device against (a) one nntk_sgd_optimize_device plus one memset per block -- the way a step was taken
before the optimizer existed -- and (b) torch.optim.Adam(fused=True) + clip_grad_norm_ on the same GPU.

Two block sets: the bench's config-5 parameters (conv 257->128 k 5 | BN 128 | LSTM 128->512 | TDD 512->1000, W and b as the gradient
blocks hand them out) and the edge set of tests/test_gpu_optimizer.py.  Per measurement: WARMUP calls, then REPEATS timings of INNER
back-to-back steps between two events (tools/timing.py); the median per step, the spread (min .. max) and bytes moved / time as a
fraction of 8 TB/s.
Writes profiles/opt_time.json (--out)."""
import argparse
import ctypes as C
import json
import os

import torch

import timing
from nntoolkitcore_amd import capi, layers as NL

WARMUP, REPEATS, INNER = 20, 15, 50
SETS = {
    "config5": [257 * 128 * 5, 128, 128, 128, 128 * 2048, 512 * 2048, 2048, 2048, 512 * 1000, 1000],
    "edges": [1, 0, 3, 4, 5, 255, 256, 257, 4099, 65537, 2 ** 20 + 3],
}


def step_us(fn):
    return {k + "_us": 1e3 * ms for k, ms in timing.timed(fn, REPEATS, WARMUP, INNER).dict.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "opt_time.json"))
    args = ap.parse_args()
    L = timing.open_device()
    res = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "repeats": REPEATS, "inner": INNER, "sets": {}}
    for name, sizes in SETS.items():
        n = sum(sizes)
        ws = [torch.randn(s, device="cuda") for s in sizes]
        gs = [torch.randn(s, device="cuda") * 1e-3 for s in sizes]
        blocks = list(zip(ws, gs))
        r = {"floats": n, "blocks": len(sizes)}
        for tag, kind, cfg, bytes_per in (
                ("adam_clip_zero", "adam", dict(learning_rate=1e-3, clip_norm=1.0, zero_gradients=1), 4 * (1 + 4 + 4)),   # pass 1 reads g; pass 2 reads g w m v, writes w m v g
                ("sgd_zero", "sgd", dict(learning_rate=1e-3, zero_gradients=1), 4 * (1 + 2 + 2))):
            opt = NL.Optimizer(kind, blocks, **cfg)
            t = step_us(opt.step)
            t["bytes"] = bytes_per * n
            t["fraction_of_8TBs"] = t["bytes"] / (t["median_us"] * 1e-6) / 8e12
            r["optimizer_" + tag] = t
            opt.destroy()

        def parent():
            for w, g in blocks:
                if w.numel():
                    L.nntk_sgd_optimize_device(capi.SGD(1e-3), C.c_void_p(g.data_ptr()), C.c_void_p(w.data_ptr()), w.numel())
                    g.zero_()
        t = step_us(parent)
        t["bytes"] = 4 * (2 + 1 + 1) * n
        t["fraction_of_8TBs"] = t["bytes"] / (t["median_us"] * 1e-6) / 8e12
        r["per_block_sgd_plus_memset"] = t
        params = [torch.nn.Parameter(w.clone()) for w in ws if w.numel()]
        for p, g in zip(params, [g for g in gs if g.numel()]):
            p.grad = g.clone()
        topt = torch.optim.Adam(params, lr=1e-3, fused=True)

        def torch_step():
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            topt.step()
        t = step_us(torch_step)
        t["bytes"] = 4 * (1 + 2 + 4 + 3) * n
        t["fraction_of_8TBs"] = t["bytes"] / (t["median_us"] * 1e-6) / 8e12
        r["torch_adam_fused_plus_clip"] = t
        res["sets"][name] = r
        for k, v in r.items():
            if isinstance(v, dict):
                print("%-8s %-28s %8.1f us (%.1f .. %.1f)  %.3f of 8 TB/s" % (name, k, v["median_us"], v["min_us"], v["max_us"], v["fraction_of_8TBs"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
