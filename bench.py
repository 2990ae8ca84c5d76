#!/usr/bin/env python3
"""bench.py -- audio frames/sec of the NNToolkitCore time-series inference hot path on MI355X.

A "step" is one pass of the hot path over one batch of synthetic 16 kHz audio, through
the C boundary (libnntoolkitcore_hip.so, device-pointer entry points).  Default workload
= BASELINE.json configs[4] ("stack"):
    Spectrogram(win 400, hop 160, nfft 512) -> Conv1d(257->128,k=5)+BatchNorm+ReLU
      -> LSTM(512, v2) -> TimeDistributedDense(1000)
with 512 utterances x 1000 frames PER GPU (weak scaling: 8 GPUs = the named batch 4096).
Other BASELINE configs are selectable with --workload {spectrogram,conv,gru} for the
per-kernel roofline lines in BASELINE.md / DESIGN.md (with --full).

Contract: W untimed warm-up steps, then exactly K timed steps bracketed by barrier +
torch.cuda.synchronize() on both sides, MAX over ranks, rank 0 prints ONE JSON line.
Inputs are resident in HBM before the timed region.  `value` = whole-job frames/s.
A plain run prints only what the timed steps measured.  With --full the line also holds
`roofline`, the dominant kernel from HIP-event timings taken inside this run, and
`cpu_baseline`, which times the CPU oracle (oracle/, a restatement of the reference's
single-threaded scalar path) on a bounded sample of the same workload, rank 0, N=1 only.
--dump-outputs DIR writes what the last timed step computed (rank 0's output tensor, or a
fixed seeded sample of its frames when it is larger than 32 MiB) as DIR/<workload>_out.npy;
inputs and weights are seeded, so the same arguments give the same inputs on every run.

Multi-GPU: one process per GPU.  Under a launcher (torch.distributed.run sets RANK / LOCAL_RANK /
WORLD_SIZE / MASTER_*) this file is a rank.  Run bare as `python bench.py --gpus N` with N > 1 it
is its own launcher: the parent -- before importing torch or touching the GPU in any way --
starts N fresh rank processes of this same file, waits for them, and exits non-zero if any of them
failed; rank 0's JSON line is the output.  No data-path collective: utterances are sharded, the only
RCCL traffic is one weight broadcast, an all_gather of the rank ids (`config.ranks_seen`) and the
barrier / MAX-reduce of the timing contract.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

F32_MFMA_PEAK_TFLOPS = 157.3     # MI355X_MICROARCH.md: exact-f32 MFMA = f32 vector peak
BF16_MFMA_PEAK_TFLOPS = 2500.0   # MI355X_MICROARCH.md: dense bf16 MFMA
SPLIT_PRODUCTS = 6               # bf16 MFMA products per f32 product in the split-bf16x3 contraction (conv1d.hip)
HBM_PEAK_GBS = 8000.0            # HBM3E spec (6290 GB/s measured copy)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="stack", choices=["stack", "spectrogram", "conv", "gru"])
    ap.add_argument("--batch-per-gpu", type=int, default=0, help="utterances per GPU (0 = the BASELINE shape)")
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--conv-stride", type=int, default=1, help="stride of the conv workload's Conv1d (2 = the sub-sampling front end; not a BASELINE config)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out the CPU oracle timing")
    ap.add_argument("--full", action="store_true", help="also the roofline line and the CPU oracle baseline (off by default)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's output (float32; a fixed seeded sample of frames above 32 MiB) as DIR/<workload>_out.npy")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher rehearsal on the CPU (gloo): rendezvous + all_gather of the rank ids, no GPU work, "
                         "prints {\"dry_run\": true, ...} and NO metric")
    return ap.parse_args()


def self_launch(a):
    """`python bench.py --gpus N` (N > 1) with no launcher around it: become the launcher.  Runs before torch is
    imported and before anything touches the GPU; children are fresh processes (never os.exec*), one per GPU."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(a.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(a.gpus), LOCAL_WORLD_SIZE=str(a.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # only rank 0 prints the JSON line; the other ranks' stdout goes to our stderr
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr, text=True))

    def relay(stream):                   # rank 0: JSON lines to stdout, any library chatter to stderr
        for line in stream:
            (sys.stdout if line.lstrip().startswith("{") else sys.stderr).write(line)
            sys.stdout.flush()

    import threading
    pump = threading.Thread(target=relay, args=(procs[0].stdout,), daemon=True)
    pump.start()
    deadline = time.time() + float(os.environ.get("NNTK_BENCH_LAUNCH_TIMEOUT", "1500"))
    rc = 0
    live = set(range(a.gpus))
    while live and rc == 0:
        for r in sorted(live):
            code = procs[r].poll()
            if code is not None:
                live.discard(r)
                if code != 0:
                    sys.stderr.write("bench.py: rank %d exited with code %d\n" % (r, code))
                    rc = code if code > 0 else 1
        if time.time() > deadline:
            sys.stderr.write("bench.py: ranks still running at the launch timeout\n")
            rc = 124
        if live and rc == 0:
            time.sleep(0.05)
    for r in live:                       # a rank failed or timed out: stop exactly the processes started here
        procs[r].terminate()
    for r in live:
        try:
            procs[r].wait(timeout=20)
        except subprocess.TimeoutExpired:
            procs[r].kill()
    pump.join(timeout=10)
    return rc


# ------------------------------------------------------------------ weights ---

def make_weights(workload, seed):
    """Synthetic random-init weights, U(-1/sqrt(fan_in), 1/sqrt(fan_in)), as one
    flat fp32 vector so that rank 0 can broadcast it over RCCL in a single collective."""
    r = np.random.default_rng(seed)
    u = lambda shape, fan: r.uniform(-fan ** -0.5, fan ** -0.5, shape).astype(np.float32)
    parts = {}
    if workload in ("stack", "conv"):
        cin = 257 if workload == "stack" else 40
        parts["conv_W"], parts["conv_b"] = u((128, cin, 5), cin * 5), u((128,), cin * 5)
        parts["bn_gamma"] = r.uniform(0.5, 1.5, 128).astype(np.float32)
        parts["bn_beta"] = r.uniform(-0.5, 0.5, 128).astype(np.float32)
        parts["bn_mean"] = (0.1 * r.standard_normal(128)).astype(np.float32)
        parts["bn_var"] = r.uniform(0.5, 1.5, 128).astype(np.float32)
    if workload == "stack":
        parts["lstm_W"], parts["lstm_U"] = u((128, 2048), 128), u((512, 2048), 512)
        parts["lstm_bi"], parts["lstm_bh"] = u((2048,), 512), u((2048,), 512)
        parts["tdd_W"], parts["tdd_b"] = u((512, 1000), 512), u((1000,), 512)
    if workload == "gru":
        parts["g1_W"], parts["g1_U"], parts["g1_bi"], parts["g1_bh"] = u((128, 768), 128), u((256, 768), 256), u((768,), 256), u((768,), 256)
        parts["g2_W"], parts["g2_U"], parts["g2_bi"], parts["g2_bh"] = u((256, 768), 256), u((256, 768), 256), u((768,), 256), u((768,), 256)
    return parts


def pack(parts):
    return np.concatenate([v.ravel() for v in parts.values()]) if parts else np.zeros(1, np.float32)


def unpack(flat, parts):
    out, o = {}, 0
    for k, v in parts.items():
        out[k] = flat[o:o + v.size].reshape(v.shape)
        o += v.size
    return out


# ---------------------------------------------------------------- workloads ---

def capi_lib():
    from nntoolkitcore_amd import capi
    return capi.load()


class Workload:
    """Builds the layer handles through the reference-shaped C API and runs one step."""

    def __init__(self, name, B, frames, weights, torch, NL):
        self.name, self.B, self.frames, self.torch, self.NL = name, B, frames, torch, NL
        self.layers = []
        w = weights
        dev = "cuda"
        g = torch.Generator(device=dev)
        g.manual_seed(1234 + int(os.environ.get("RANK", "0")))
        if name in ("stack", "spectrogram"):
            N = 16000 if name == "spectrogram" else 240 + 160 * frames
            self.spec = NL.Spectrogram(512, 400, 240, N)
            self.layers.append(self.spec)
            self.x = (0.1 * torch.randn(B, N, device=dev, generator=g)).clamp_(-1, 1)
            self.frames_per_utt = self.spec.out_shape[0]
            self.spec_out = torch.empty((B,) + self.spec.out_shape, device=dev)
        if name in ("stack", "conv"):
            cin = 257 if name == "stack" else 40
            T = self.spec.out_shape[0] if name == "stack" else frames
            self.conv = NL.Conv1d(cin, 128, 5, int(os.environ.get("NNTK_BENCH_CONV_STRIDE", "1")) if name == "conv" else 1, T)
            Tc = self.conv.out_shape[0]
            self.bn = NL.BatchNorm(128, 1e-3, Tc)
            self.relu = NL.Activation("relu", Tc * 128, 1.0)
            self.conv.set_weights(w["conv_W"], w["conv_b"])
            self.bn.set_weights(w["bn_gamma"], w["bn_beta"], w["bn_mean"], w["bn_var"])
            self.layers += [self.conv, self.bn, self.relu]
            self.conv_out = torch.empty((B, Tc, 128), device=dev)
            if name == "conv":
                self.x = torch.randn(B, T, cin, device=dev, generator=g)
                self.frames_per_utt = T
        if name == "stack":
            Tc = self.conv.out_shape[0]
            self.lstm = NL.LSTM(128, 512, True, Tc, v2=True)
            self.lstm.set_weights(w["lstm_W"], w["lstm_U"], w["lstm_bi"], w["lstm_bh"])
            self.tdd = NL.TimeDistributedDense(Tc, 512, 1000)
            self.tdd.set_weights(w["tdd_W"], w["tdd_b"])
            self.layers += [self.lstm, self.tdd]
            self.tdd_out = torch.empty((B, Tc, 1000), device=dev)
            # default: the LSTM hands its output to the dense layer in frag3 form (already split for the split-bf16 contraction, MFMA
            # fragment order -- the LSTM kernel's own hand-off buffer); NNTK_BENCH_STACK_F32=1: through an f32 tensor, as round 3 did
            self.f32_route = bool(int(os.environ.get("NNTK_BENCH_STACK_F32", "0")))
            if self.f32_route:
                self.lstm_out = torch.empty((B, Tc, 512), device=dev)
            else:
                self.lstm_f3 = torch.empty(capi_lib().nntk_frag3_floats(B, Tc, 512), device=dev)
            # ... by default in FRAG2H form (two f16 images of h * 2^15 written by the LSTM kernel's output wave; the dense GEMM sums three
            # products per k step instead of six -- what LSTMTimeDistributedDenseApplyDevice does); NNTK_DENSE_F16X2=0: the frag3 route
            from nntoolkitcore_amd import capi as _capi
            self.h2_route = not self.f32_route and _capi.get_option("dense_f16x2") != 0
            if self.h2_route:
                self.lstm_h2 = torch.empty(capi_lib().nntk_frag2h_floats(B, Tc, 512), device=dev)
            # ... and the conv layer hands ITS output to the LSTM in frag3 form too, written by the conv kernel's epilogue
            # (Conv1dBatchNormActivationApplyDeviceFrag3); NNTK_BENCH_CONV_F32=1: f32 tensor + the LSTM call's pack pass, as round 4 did
            self.conv_f3_route = not self.f32_route and not bool(int(os.environ.get("NNTK_BENCH_CONV_F32", "0")))
            if self.conv_f3_route:
                self.conv_f3 = torch.empty(capi_lib().nntk_frag3_floats(B, Tc, 128), device=dev)
        if name == "gru":
            self.g1 = NL.GRU(128, 256, True, frames)
            self.g2 = NL.GRU(256, 256, True, frames)
            self.g1.set_weights(w["g1_W"], w["g1_U"], w["g1_bi"], w["g1_bh"])
            self.g2.set_weights(w["g2_W"], w["g2_U"], w["g2_bi"], w["g2_bh"])
            self.layers += [self.g1, self.g2]
            self.x = torch.randn(B, frames, 128, device=dev, generator=g)
            self.h1 = torch.empty((B, frames, 256), device=dev)
            self.h2 = torch.empty((B, frames, 256), device=dev)
            self.frames_per_utt = frames
        self.phase_ms = {}

    def step(self, timed=False):
        t = self.torch
        ev = []

        def mark(name):
            if timed:
                e = t.cuda.Event(enable_timing=True)
                e.record()
                ev.append((name, e))

        mark("start")
        if self.name in ("stack", "spectrogram"):
            self.spec.apply_device(self.x, out=self.spec_out)
            mark("spectrogram")
        if self.name == "stack":
            if self.conv_f3_route:
                self.conv.apply_device_frag3(self.spec_out, out_f3=self.conv_f3, bn=self.bn, act=self.relu)
            else:
                self.conv.apply_device(self.spec_out, out=self.conv_out, bn=self.bn, act=self.relu)
            mark("conv_bn_relu")
            if self.f32_route:
                self.lstm.apply_device(self.conv_out, out=self.lstm_out)
                mark("lstm")
                self.tdd.apply_device(self.lstm_out, out=self.tdd_out)
            elif self.h2_route:       # = LSTMTimeDistributedDenseApplyDevice, as its two halves so that each gets its own HIP-event phase
                if self.conv_f3_route:
                    self.NL.lstm_apply_device_frag2h(self.lstm, x_f3=self.conv_f3, batch=self.B, out_h2=self.lstm_h2)
                else:
                    self.NL.lstm_apply_device_frag2h(self.lstm, x=self.conv_out, out_h2=self.lstm_h2)
                mark("lstm")
                self.NL.tdd_apply_device_frag2h(self.tdd, self.lstm_h2, self.B, out=self.tdd_out)
            else:       # ... on the frag3 form (option dense_f16x2 = 0)
                if self.conv_f3_route:
                    self.NL.recurrent_apply_device_frag3(self.lstm, x_f3=self.conv_f3, batch=self.B, want_f32=False, out_f3=self.lstm_f3)
                else:
                    self.NL.recurrent_apply_device_frag3(self.lstm, x=self.conv_out, want_f32=False, out_f3=self.lstm_f3)
                mark("lstm")
                self.NL.tdd_apply_device_frag3(self.tdd, self.lstm_f3, self.B, out=self.tdd_out)
            mark("tdd")
        if self.name == "conv":
            self.conv.apply_device(self.x, out=self.conv_out, bn=self.bn, act=self.relu)
            mark("conv_bn_relu")
        if self.name == "gru":
            if os.environ.get("NNTK_BENCH_GRU_UNFUSED"):          # A/B: the two layers as two calls
                self.g1.apply_device(self.x, out=self.h1)
                mark("gru1")
                self.g2.apply_device(self.h1, out=self.h2)
                mark("gru2")
            else:                                                  # one call: both layers in one persistent launch
                self.NL.gru_stack2_apply_device(self.g1, self.g2, self.x, out=self.h2)
                mark("gru_stack2")
        return ev

    def output(self):
        """The tensor a caller of the timed path receives (every step overwrites it)."""
        return getattr(self, {"stack": "tdd_out", "spectrogram": "spec_out", "conv": "conv_out", "gru": "h2"}[self.name])

    def destroy(self):
        for l in self.layers:
            l.destroy()


DUMP_BYTES = 32 << 20


def dump_outputs(wl, path, seed):
    """Writes wl's output as float32 DIR/<workload>_out.npy: whole when it fits in DUMP_BYTES, otherwise as many of its
    rows (one row = one frame's channels) as fit, drawn with `seed` and kept in ascending order, shape [rows, channels]."""
    y = wl.output()
    if y.numel() * 4 > DUMP_BYTES:
        y = y.reshape(-1, y.shape[-1])
        rows = np.sort(np.random.default_rng(seed).choice(y.shape[0], DUMP_BYTES // (4 * y.shape[1]), replace=False))
        y = y.index_select(0, wl.torch.from_numpy(rows).to(y.device))
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, wl.name + "_out.npy"), y.float().cpu().numpy())


def pmc_traffic(kernel_prefix, B):
    """HBM bytes per launch of the dominant kernel from a committed rocprofv3 PMC summary (profiles/*_pmc_traffic.json:
    FETCH_SIZE / WRITE_SIZE collected in separate --pmc runs of this same command and corrected as
    MI355X_MICROARCH.md prescribes).  PMC counters cannot be read from inside a timed run, so this is a profiled
    value -- returned ONLY when the profile is stamped with the hash of the sources this library was built from
    and the same utterances per GPU; otherwise (None, why)."""
    import glob
    from nntoolkitcore_amd import capi
    # the hash the LOADED library carries (embedded at build time), not the source tree's: a stale .so must not borrow a
    # newer profile's counters
    want = (capi.load().nntk_build_source_hash() or b"").decode()
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic*.json")), reverse=True):
        try:
            d = json.load(open(path))
        except (OSError, ValueError):
            continue
        if d.get("source_hash") != want or d.get("utterances_per_gpu") != B:
            continue
        hits = [v.get("hbm_bytes_per_launch") for name, v in d.get("kernels", {}).items() if name.startswith(kernel_prefix)]   # (str or tuple of str)
        hits = [h for h in hits if h is not None]
        if hits:      # several instantiations of one kernel in a step (the two GRU layers): their average, like ms_per_launch
            return sum(hits) / len(hits), "%s (source_hash %s)" % (os.path.relpath(path, ROOT), want)
    return None, "no profiles/*_pmc_traffic.json stamped with this library's source_hash %s at %d utterances/GPU" % (want, B)


def gemm_mode():
    """Which contraction the conv / dense / TDD kernels run (library option gemm_split_bf16; auto = split)."""
    from nntoolkitcore_amd import capi
    return "exact-f32" if capi.get_option("gemm_split_bf16") == 0 else "split-bf16x3 (f32 operands as 3 bf16 terms, f32 accumulate)"


def roofline_for(wl, phase_ms, prof):
    """Dominant-kernel roofline from live HIP-event timings (ms per launch)."""
    B = wl.B
    if wl.name == "spectrogram":
        nts, nfreq = wl.spec.out_shape
        bytes_ = B * (wl.x.shape[1] * 4 + nts * nfreq * 4)
        ms = phase_ms["spectrogram"]
        ach = bytes_ / (ms * 1e-3) / 1e9
        traffic, traffic_source = pmc_traffic("spectrogram512_kernel", B)
        return {"kernel": "spectrogram512_kernel", "bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": ach / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source, "ms_per_launch": ms,
                "algorithmic_bytes": bytes_}
    if wl.name == "conv":
        Tc = wl.conv.out_shape[0]
        cin = wl.conv.cfg.input_feature_channels
        flops = 2.0 * cin * 5 * 128 * Tc * B
        bytes_ = B * (wl.conv.cfg.input_size * cin + Tc * 128) * 4
        ms = phase_ms["conv_bn_relu"]
        ach = flops / (ms * 1e-3) / 1e12
        hbm_frac = bytes_ / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS
        from nntoolkitcore_amd import capi
        # channel counts that are multiples of 8 but not of 16 take the flat-K kernel (conv1d_flatk.hip) at stride 1 unless conv_flatk = 0
        flatk = gemm_mode() != "exact-f32" and capi.get_option("conv_flatk") != 0 and cin % 8 == 0 and cin % 16 != 0 and wl.conv.cfg.stride == 1
        split_kernel = "conv1d_flatk_bf16x3_kernel" if flatk else "conv1d_mfma_bf16x3_kernel"
        traffic, traffic_source = pmc_traffic("conv1d_mfma_kernel" if gemm_mode() == "exact-f32" else split_kernel, B)
        if gemm_mode() == "exact-f32":
            return {"kernel": "conv1d_mfma_kernel<2,2,2,2>", "bound": "mfma", "achieved": ach, "peak": F32_MFMA_PEAK_TFLOPS,
                    "unit": "TFLOP/s", "frac": ach / F32_MFMA_PEAK_TFLOPS, "traffic": traffic, "traffic_source": traffic_source, "ms_per_launch": ms,
                    "algorithmic_flops": flops, "algorithmic_bytes": bytes_, "hbm_frac": hbm_frac}
        # split-bf16x3: six bf16 MFMA products per f32 product, so the MFMA ceiling in ALGORITHMIC flops is the dense
        # bf16 peak / 6 (still above the HBM ceiling's time here: 125 us vs 86 us at config 3)
        peak = BF16_MFMA_PEAK_TFLOPS / SPLIT_PRODUCTS
        return {"kernel": split_kernel + ("<2,true>" if flatk else "<2,2,2,2>"), "bound": "mfma", "achieved": ach, "peak": peak,
                "peak_note": "dense bf16 MFMA peak / 6 products per f32 product", "unit": "TFLOP/s", "frac": ach / peak,
                "traffic": traffic, "traffic_source": traffic_source, "ms_per_launch": ms, "algorithmic_flops": flops,
                "algorithmic_bytes": bytes_, "hbm_frac": hbm_frac, "frac_of_exact_f32_mfma_peak": ach / F32_MFMA_PEAK_TFLOPS}
    # recurrent step kernel: one launch = one timestep of hU = h[B,H] x U[H,G*H] + fused gates
    H, G = (512, 4) if wl.name == "stack" else (256, 3)
    ms = prof.get("rec_launch_ms", None)
    if ms is None:
        return None
    tpl = prof["rec_timesteps_per_launch"]
    last = prof.get("rec_kernel", "")
    if last.startswith("lstm_rr_kernel"):
        # register-resident split-bf16 LSTM: ONE launch does all T steps of [h | x_t] x [U ; W] (the input projection is
        # fused: no separate GEMM, no [T, B, 4H] tensor), six bf16 MFMA products per f32 product -> the MFMA ceiling in
        # ALGORITHMIC flops is the dense bf16 peak / 6
        n_in = 128
        flops = 2.0 * B * (H + n_in) * G * H * tpl
        ach = flops / (ms * 1e-3) / 1e12
        # the HF instantiation (",hf>"): the h part on two f16 images = THREE products per f32 product, the x part on three bf16 images = six:
        # the ceiling of the products actually issued is the dense 16-bit MFMA peak / the k-weighted mean of the two
        hf = last.endswith(",hf>")
        products = (3.0 * H + 6.0 * n_in) / (H + n_in) if hf else float(SPLIT_PRODUCTS)
        peak = BF16_MFMA_PEAK_TFLOPS / products
        # (the profile's own instantiation: the HF kernel and the six-product one move different bytes)
        traffic, traffic_source = pmc_traffic("lstm_rr_kernel<8, 2, false, true, true>" if hf else "lstm_rr_kernel<8, 2, false, true>", B)
        # products x 2 tiles x k steps per half, two halves, over four wavefronts: MFMA pipe cycles per wave and timestep
        mfma_cycles = int((3 if hf else 6) * 2 * (H // 16) // 4 * 2 * 32 + 6 * 2 * (n_in // 16) // 4 * 2 * 32)
        return {"kernel": last, "bound": "mfma", "achieved": ach, "peak": peak,
                "peak_note": ("dense f16 / bf16 MFMA peak / %.2f products per f32 product (h.U: two f16 images of h and U, three products; x.W: three bf16 "
                              "images, six products)" % products) if hf else
                             "dense bf16 MFMA peak / 6 products per f32 product (split-bf16 x 3 contraction)",
                "frac_of_six_product_ceiling": ach / (BF16_MFMA_PEAK_TFLOPS / SPLIT_PRODUCTS),
                "unit": "TFLOP/s", "frac": ach / peak, "frac_of_exact_f32_mfma_peak": ach / F32_MFMA_PEAK_TFLOPS,
                "traffic": traffic, "traffic_source": traffic_source, "ms_per_launch": ms, "algorithmic_flops": flops,
                "algorithmic_flops_note": "recurrent h x U AND the fused input projection x_t x W, all T steps of one launch",
                "timesteps_per_launch": tpl, "us_per_timestep": ms * 1e3 / tpl,
                "mfma_pipe_cycles_per_timestep": mfma_cycles,
                "launches_per_step": prof.get("rec_launches_per_step")}
    if (last.startswith("gru_rr_kernel") or last.startswith("gru_fk_kernel")) and wl.name == "gru":
        # the two stacked GRU-256 layers as two launches of the register-resident split-bf16 kernel (input projections fused):
        # rec_launch_ms is the AVERAGE of the two, so are the algorithmic flops ([h | x_t] x [U ; W], three gates, T steps)
        n_l = prof.get("rec_launches_per_step") or 2.0
        flops_l1, flops_l2 = 2.0 * B * (H + 128) * G * H * tpl, 2.0 * B * (H + H) * G * H * tpl
        flops = (flops_l1 + flops_l2) / 2
        ach = flops / (ms * 1e-3) / 1e12
        peak = BF16_MFMA_PEAK_TFLOPS / SPLIT_PRODUCTS
        # which kernel each layer takes is a property of the layer (GRUKernelPlan): by default the split-K kernel for the 128-wide
        # layer 1 and the full-K one for the 256-wide layer 2
        import re
        from nntoolkitcore_amd import capi
        names = []
        for g in (wl.g1, wl.g2):
            m = re.search(r"gru_(?:rr|fk)_kernel<[0-9,]+>", capi.load().GRUKernelPlan(g.h).decode())
            names.append(m.group(0) if m else last)
        traffic, traffic_source = pmc_traffic(tuple(sorted(set(n.split("<")[0] for n in names))), B)
        return {"kernel": "%s (layer 1) + %s (layer 2)" % tuple(names), "bound": "mfma", "achieved": ach, "peak": peak,
                "peak_note": "dense bf16 MFMA peak / 6 products per f32 product (split-bf16 x 3 contraction); one gate slot in four "
                             "multiplies a zero weight block (the GRU's candidate gate keeps its x and h parts apart), not counted as flops",
                "unit": "TFLOP/s", "frac": ach / peak, "frac_of_exact_f32_mfma_peak": ach / F32_MFMA_PEAK_TFLOPS,
                "traffic": traffic, "traffic_source": traffic_source, "ms_per_launch": ms, "algorithmic_flops": flops,
                "algorithmic_flops_note": "average of the two layer launches; recurrent h x U and the fused input projection x_t x W",
                "timesteps_per_launch": tpl, "us_per_timestep": ms * 1e3 / tpl * n_l,
                "us_per_timestep_note": "both layers", "launches_per_step": n_l}
    persistent = tpl > 1
    kern = ("rec_persistent_kernel" if persistent else "rec_step_kernel") + ("<4,LSTM>" if G == 4 else "<3,GRU>")
    flops = 2.0 * B * H * G * H * tpl          # algorithmic flops of ONE launch (tpl timesteps of h[B,H] x U[H,G*H])
    if wl.name == "gru" and persistent and abs(prof.get("rec_launches_per_step", 2.0) - 1.0) < 0.01:
        # fused two-layer launch: T + 1 iterations, three [B,H] x [H,3H] products per timestep (U1, W2, U2)
        kern = "gru2_persistent_kernel<8>"
        tpl = tpl - 1
        flops = 3.0 * 2.0 * B * H * G * H * tpl
    ach = flops / (ms * 1e-3) / 1e12
    traffic, traffic_source = (pmc_traffic(kern.split("<")[0], B) if persistent else (None, "per-timestep kernels: not profiled"))
    return {"kernel": kern, "bound": "mfma", "achieved": ach, "peak": F32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": ach / F32_MFMA_PEAK_TFLOPS, "traffic": traffic, "traffic_source": traffic_source,
            "ms_per_launch": ms, "algorithmic_flops": flops,
            "timesteps_per_launch": tpl, "us_per_timestep": ms * 1e3 / tpl,
            "launches_per_step": prof.get("rec_launches_per_step")}


def cpu_baseline(workload, weights, frames, seed):
    """Times the CPU oracle (restatement of the reference's scalar single-thread path) on a
    bounded sample: ONE utterance of the same per-utterance shape."""
    import oracle as O
    r = np.random.default_rng(seed)
    w = weights
    t0 = time.perf_counter()
    if workload == "spectrogram":
        n_utt = 12000
        x = (0.1 * r.standard_normal((n_utt, 16000))).astype(np.float32)
        t0 = time.perf_counter()
        out = O.spectrogram(x, O.window("hann", 400), 512, 240)
        nframes = out.shape[0] * out.shape[1]
        sample = "%d utterances x 16000 samples (98 frames each)" % n_utt
    elif workload == "conv":
        n_utt = 1000
        x = r.standard_normal((n_utt, frames, 40)).astype(np.float32)
        t0 = time.perf_counter()
        O.activation(O.ACT_RELU, O.batch_norm(O.conv1d(x, w["conv_W"], w["conv_b"], 1), w["bn_gamma"], w["bn_beta"],
                                              w["bn_mean"], w["bn_var"], 1e-3))
        nframes = n_utt * frames
        sample = "%d utterances x %d frames x 40" % (n_utt, frames)
    elif workload == "gru":
        n_utt, fr = 32, min(frames, 1000)
        x = r.standard_normal((n_utt, fr, 128)).astype(np.float32)
        t0 = time.perf_counter()
        h1 = O.gru(x, w["g1_W"], w["g1_U"], w["g1_bi"], w["g1_bh"])
        O.gru(h1, w["g2_W"], w["g2_U"], w["g2_bi"], w["g2_bh"])
        nframes = n_utt * fr
        sample = "%d utterances x %d frames x 128" % (n_utt, fr)
    else:
        # best of three passes over 6 utterances on ONE pinned core (a 3-utterance single pass on a shared 256-core host swung
        # 2.3x between runs); frames/s does not depend on the length of an utterance, so 250 frames each keep the leg at ~10-25 s
        n_utt, fr = 6, min(frames, 250)
        x = (0.1 * r.standard_normal((n_utt, 240 + 160 * fr))).astype(np.float32)
        old_aff = None
        try:
            old_aff = os.sched_getaffinity(0)
            os.sched_setaffinity(0, {sorted(old_aff)[len(old_aff) // 2]})
        except (AttributeError, OSError):
            pass
        passes = []
        for _ in range(3):
            t0 = time.perf_counter()
            s = O.spectrogram(x, O.window("hann", 400), 512, 240)
            c = O.activation(O.ACT_RELU, O.batch_norm(O.conv1d(s, w["conv_W"], w["conv_b"], 1), w["bn_gamma"], w["bn_beta"],
                                                      w["bn_mean"], w["bn_var"], 1e-3))
            h = O.lstm(c, w["lstm_W"], w["lstm_U"], w["lstm_bi"], w["lstm_bh"], v2=True)
            O.time_distributed_dense(h, w["tdd_W"], w["tdd_b"])
            passes.append(time.perf_counter() - t0)
        if old_aff is not None:
            try:
                os.sched_setaffinity(0, old_aff)
            except OSError:
                pass
        nframes = n_utt * fr
        sample = "best of 3 passes over %d utterances x %d frames of the same stack, one pinned core" % (n_utt, fr)
        t0 = time.perf_counter() - min(passes)
        spread = [round(nframes / p_, 1) for p_ in sorted(passes, reverse=True)]
    dt = time.perf_counter() - t0
    res = {"value": nframes / dt, "unit": "frames/s", "cores": 1, "kind": "port", "sample": sample,
           "seconds": round(dt, 2), "host_nproc": os.cpu_count()}
    if workload == "stack":
        res["passes_frames_per_s"] = spread                    # slowest .. fastest of the three passes
        fr = min(frames, 1000)
        # N independent workers, one utterance each (the reference's Linux build is serial --
        # core/loop.h:23 -- so the 1-thread figure above stays the faithful one; this is its embarrassingly
        # parallel upper bound on this host).  ctypes releases the GIL inside the oracle's C calls.
        from concurrent.futures import ThreadPoolExecutor
        n_thr = max(1, min(512, os.cpu_count() or 1))          # N = nproc; VERDICT r02: no cap at 16
        # bounded sample: ~25 k frames in all (256 workers x 1000 frames took 96 s -- the per-core rate drops 10x when every
        # core streams its own 5 MB of LSTM weights per timestep)
        fr = max(50, min(fr, 25600 // n_thr))
        xs = (0.1 * r.standard_normal((n_thr, 240 + 160 * fr))).astype(np.float32)

        def one(i):
            s_ = O.spectrogram(xs[i:i + 1], O.window("hann", 400), 512, 240)
            c_ = O.activation(O.ACT_RELU, O.batch_norm(O.conv1d(s_, w["conv_W"], w["conv_b"], 1), w["bn_gamma"],
                                                       w["bn_beta"], w["bn_mean"], w["bn_var"], 1e-3))
            h_ = O.lstm(c_, w["lstm_W"], w["lstm_U"], w["lstm_bi"], w["lstm_bh"], v2=True)
            O.time_distributed_dense(h_, w["tdd_W"], w["tdd_b"])

        t1 = time.perf_counter()
        with ThreadPoolExecutor(n_thr) as ex:
            list(ex.map(one, range(n_thr)))
        dt2 = time.perf_counter() - t1
        res.update({"threads": n_thr, "threads_value": n_thr * fr / dt2,
                    "threads_sample": "%d workers x 1 utterance x %d frames" % (n_thr, fr), "threads_seconds": round(dt2, 2)})
    return res


def dry_run(a, world, rank):
    """Launcher rehearsal (tests, CPU): rendezvous over gloo, all_gather of the rank ids, one barrier.  Prints no metric."""
    import torch
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    seen = [rank]
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        t = torch.tensor([rank], dtype=torch.int32)
        parts = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(parts, t)
        seen = [int(p.item()) for p in parts]
        dist.barrier()
    if rank == 0:
        print(json.dumps({"dry_run": True, "n_gpus": world, "ranks_seen": seen, "backend": "gloo"}), flush=True)
    if world > 1:
        dist.destroy_process_group()


def main():
    a = parse()
    if a.conv_stride != 1:
        os.environ["NNTK_BENCH_CONV_STRIDE"] = str(a.conv_stride)       # reaches Workload in this process and in self-launched ranks
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(a))          # parent: nothing below runs here, the GPU is never touched
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus != world:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d (run `python bench.py --gpus N` bare, or under "
                         "torch.distributed.run with --nproc-per-node N)" % (a.gpus, world))
    if a.dry_run:
        return dry_run(a, world, rank)
    import torch
    assert torch.cuda.is_available(), "bench.py needs a GPU: the HIP path has no CPU fallback"
    # one process per GPU.  (NNTK_BENCH_BACKEND=gloo is a rehearsal mode for a 1-GPU box: several ranks share
    # the card and the collectives run on the CPU; never used by the driver.)
    backend = os.environ.get("NNTK_BENCH_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    if backend == "nccl" and world > ndev:
        raise SystemExit("bench.py: %d ranks but only %d GPU(s) visible; RCCL needs one GPU per rank "
                         "(NNTK_BENCH_BACKEND=gloo rehearses several ranks on one card)" % (world, ndev))
    local = local % ndev
    torch.cuda.set_device(local)
    dist = None
    ranks_seen = [0]
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":             # "nccl" is RCCL on ROCm; bind the communicator to this rank's GPU
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        # every rank reports in through the communicator the bench uses: N distinct ids = N ranks really joined
        t = torch.tensor([rank], dtype=torch.int32, device="cuda" if backend == "nccl" else "cpu")
        parts = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(parts, t)
        ranks_seen = [int(p.item()) for p in parts]
        assert sorted(ranks_seen) == list(range(world)), ranks_seen

    from nntoolkitcore_amd import capi, layers as NL
    from nntoolkitcore_amd.sharding import broadcast_weights
    L = capi.load()
    assert L.nntk_hip_set_device(local) == 0, capi.last_error()
    NL.use_torch_stream()
    L.nntk_hip_profile_enable(1)

    defaults = {"stack": 512, "spectrogram": 256, "conv": 1024, "gru": 1024}
    B = a.batch_per_gpu or defaults[a.workload]
    frames = a.frames

    # rank 0 owns the weights; one RCCL broadcast of the packed blob over xGMI (off the timed path)
    parts = make_weights(a.workload, a.seed + 2)
    flat = pack(parts) if rank == 0 else np.zeros_like(pack(parts))
    flat = broadcast_weights(flat, torch, dist)
    weights = unpack(flat, parts)
    weights_crc = int(hashlib.sha256(flat.tobytes()).hexdigest()[:8], 16)

    wl = Workload(a.workload, B, frames, weights, torch, NL)

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            if backend == "nccl":
                dist.barrier(device_ids=[local])
            else:
                dist.barrier()
        torch.cuda.synchronize()

    def check_device_status(where):
        # surfaces asynchronous kernel-side failures (e.g. a timed-out hand-off of the persistent recurrent
        # kernel): a number measured on invalid results must never be printed
        if L.nntk_hip_synchronize() != 0:
            raise SystemExit("bench.py: device error %s: %s" % (where, capi.last_error()))

    for _ in range(a.warmup):
        wl.step()
    barrier()
    check_device_status("after warm-up")
    # per-phase HIP events on the launch stream.  A one-kernel workload is bracketed ONCE around all K launches (an event
    # pair around each 15-us launch costs about as much as the launch); the multi-kernel ones get per-phase events.
    single = {"spectrogram": "spectrogram", "conv": "conv_bn_relu"}.get(a.workload)
    t0 = time.perf_counter()
    events = []
    if single:
        r0, r1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        r0.record()
        for i in range(a.steps):
            wl.step()
        r1.record()
    else:
        for i in range(a.steps):
            events.append(wl.step(timed=True))
    torch.cuda.synchronize()
    dt_own = time.perf_counter() - t0          # this rank's own time for its K steps, before it waits for the others
    barrier()
    dt = time.perf_counter() - t0
    check_device_status("after the timed steps")
    if a.dump_outputs and rank == 0:
        dump_outputs(wl, a.dump_outputs, a.seed)
    crcs = [weights_crc]
    rank_ms = [dt_own / a.steps * 1e3]
    if dist is not None:
        on_gpu = dist.get_backend() == "nccl"
        t = torch.tensor([dt], device="cuda" if on_gpu else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        # per-rank step time: skew between the GPUs of a node is visible in the record
        o = torch.tensor([dt_own / a.steps * 1e3], device="cuda" if on_gpu else "cpu", dtype=torch.float64)
        os_ = [torch.zeros_like(o) for _ in range(world)]
        dist.all_gather(os_, o)
        rank_ms = [float(x.item()) for x in os_]
        # the broadcast really delivered rank 0's weights everywhere
        c = torch.tensor([weights_crc], device="cuda" if on_gpu else "cpu", dtype=torch.int64)
        cs = [torch.zeros_like(c) for _ in range(world)]
        dist.all_gather(cs, c)
        crcs = [int(x.item()) for x in cs]
        assert len(set(crcs)) == 1, "weight broadcast mismatch across ranks: %r" % crcs

    # per-phase HIP-event times (ms), averaged over the timed steps
    phase_ms = {}
    if single:
        phase_ms[single] = r0.elapsed_time(r1) / a.steps
    for ev in events:
        for (n0, e0), (n1, e1) in zip(ev[:-1], ev[1:]):
            phase_ms[n1] = phase_ms.get(n1, 0.0) + e0.elapsed_time(e1) / a.steps
    prof = {}
    ms = C.c_double()
    cnt, units = C.c_long(), C.c_long()
    if L.nntk_hip_profile_get(b"rec_step", C.byref(ms), C.byref(cnt), C.byref(units)) == 0 and cnt.value > 0:
        prof["rec_launch_ms"] = ms.value / cnt.value                 # average duration of one kernel launch
        prof["rec_timesteps_per_launch"] = units.value / cnt.value   # 1 = per-step kernels, T = persistent
        prof["rec_launches_per_step"] = cnt.value / max(1, a.steps + a.warmup)
        prof["rec_kernel"] = (L.nntk_hip_last_recurrent_kernel() or b"").decode()

    total_frames = world * B * wl.frames_per_utt * a.steps
    value = total_frames / dt
    out = {
        "metric": "audio frames/sec (whole node)", "value": value, "unit": "frames/s", "n_gpus": world,
        "steps": a.steps, "warmup": a.warmup, "ms_per_step": dt / a.steps * 1e3, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": {
            "stack": "BASELINE configs[4]: Spectrogram(400/160/512)->Conv1d(257->128,k=5)+BN+ReLU->LSTM(512,v2)->TDD(1000)",
            "spectrogram": "BASELINE configs[1]: Spectrogram(400/160/512) on batch x 16000",
            "conv": ("BASELINE configs[2]: Conv1d(40->128,k=5)+BN+ReLU on batch x frames x 40" if a.conv_stride == 1 else
                     "Conv1d(40->128,k=5,stride=%d)+BN+ReLU on batch x frames x 40 (NOT a BASELINE config: the sub-sampling variant of configs[2])" % a.conv_stride),
            "gru": "BASELINE configs[3]: 2-layer GRU(128->256->256) on batch x frames x 128"}[a.workload],
            "utterances_per_gpu": B, "frames_per_utterance": wl.frames_per_utt, "global_batch": B * world,
            "parallelism": "utterance shards, dp%d, no data-path collective" % world,
            "backend": ("rccl" if backend == "nccl" else backend) if world > 1 else None,
            "ranks_seen": ranks_seen,
            "conv_to_lstm": ("frag3 tensor written by the conv kernel's epilogue (Conv1dBatchNormActivationApplyDeviceFrag3; no pack pass); "
                             "bit-identical to the f32 route" if getattr(wl, "conv_f3_route", False) else
                             "f32 tensor, packed into frag3 form inside the LSTM call") if a.workload == "stack" else None,
            "lstm_to_tdd": ("f32 tensor" if getattr(wl, "f32_route", True) else
                            "frag2h tensor: h as two f16 images of h * 2^15 (|h| < 1; operands to 2^-23 relative at worst) -- the LSTM kernel's own hand-off buffer, "
                            "W as two f16 images of W * 2^q; the dense GEMM sums three products per k step (f32 accumulation); error vs f64 below the "
                            "frag3 route's (tests/test_gpu_frag2h.py, profiles/r05_gemm_f16x2_micro.log); NNTK_DENSE_F16X2=0 selects the frag3 route"
                            if getattr(wl, "h2_route", False) else
                            "frag3 tensor: the LSTM kernel's T-deep hand-off buffer (h already split into three bf16 images, MFMA fragment order) "
                            "is the dense GEMM's A operand; bit-identical to the f32 route") if a.workload == "stack" else None,
            "gemm": gemm_mode() + (" for conv; TDD on two f16 images of h and W, three products (dense_frag3_kernel<...,1>)"
                                   if getattr(wl, "h2_route", False) else " for conv / TDD") + (
                ("; LSTM: " + prof["rec_kernel"] + (" (recurrence h.U on two f16 images of h * 2^15 and U * 2^q, three products per k step; the fused input "
                                                   "projection x.W on three bf16 images, six products; NNTK_REC_HF=0: all six-product)"
                                                   if prof["rec_kernel"].endswith(",hf>") else
                                                   " (split-bf16x3 recurrence with the input projection fused into the step)"))
                if prof.get("rec_kernel", "").startswith("lstm_rr") else
                ("; GRU layers: register-resident split-bf16x3 recurrences with the input projections fused into the step (gru_rr_kernel: split-K over "
                 "four wavefronts; gru_fk_kernel: full K per wavefront); layer 1 hands h over in frag3 form")
                if prof.get("rec_kernel", "").startswith(("gru_rr", "gru_fk")) else
                ("; exact-f32 for the recurrent input projection and recurrences" if a.workload in ("stack", "gru") else "")),
            "gemm_accuracy": ("f32 results: error vs a float64 contraction <= the exact-f32 MFMA chain's on every BASELINE shape "
                              "(profiles/r02_split_error.log, tools/split_error.py); NNTK_GEMM_SPLIT_BF16=0 selects the exact chain")
                             if gemm_mode() != "exact-f32" else "exact-f32 MFMA chain"},
        "phase_ms": {k: round(v, 4) for k, v in phase_ms.items()},
        "rank_ms_per_step": {"min": round(min(rank_ms), 4), "max": round(max(rank_ms), 4), "per_rank": [round(v, 4) for v in rank_ms]},
    }
    if rank == 0:
        if a.full:
            out["roofline"] = roofline_for(wl, phase_ms, prof)
            if world == 1 and not a.no_cpu_baseline:
                out["cpu_baseline"] = cpu_baseline(a.workload, weights, frames, a.seed)
        print(json.dumps(out), flush=True)
    wl.destroy()
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
