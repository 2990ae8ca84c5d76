#!/usr/bin/env python3
"""What greedy transducer decoding costs (csrc/hip/rnnt_decode.hip), next to the host-driven loop it replaces:
python tools/rnnt_decode_time.py [repeats]      -> profiles/rnnt_decode_time.json and the same JSON line on stdout
Model E = H = J = 512, V = 1024, T = 200, tanh joiner, with the projection; batch 1, 16 and 256.  `decode_ms`: one
nntk_rnnt_greedy_decode_device call (timed by tools/timing.py).  `host_loop_ms`: the same decoding driven from the
host with the calls the library had before -- per decision, for the whole batch in lockstep: the joiner (T = U1 = 1), the vocabulary
Dense, an argmax with its read-back, and for the rows that emitted a one-step LSTMApplyDeviceVarLen (length 0 keeps a row's state) and
the projection Dense -- wall clock around the loop, median of the repeats.  Both numbers are reported as measured."""
import sys, time
import numpy as np
import torch
from timing import emit, open_device, timed
from nntoolkitcore_amd import layers as NL

E = H = J = 512
V, T, BLANK, MAX_SYMBOLS = 1024, 200, 0, 3
BATCHES = (1, 16, 256)
WARMUP = 1


def model(rng):
    u = lambda sc, *s: rng.uniform(-sc, sc, s).astype(np.float32)
    G = 4 * H
    bias = u(0.1, V)
    bias[1:] -= np.float32(3.0)                      # about one label in four decisions
    return dict(embed=u(1.0, V, E), W=u(2.0 * E ** -0.5, E, G), U=u(2.0 * H ** -0.5, H, G), b_i=u(0.1, G), b_h=u(0.1, G),
                Wp=u(2.0 * H ** -0.5, H, J), bp=u(0.1, J), Wo=u(3.0 * J ** -0.5, J, V), bo=bias)


def host_loop(m, layers, enc, embed_d):
    """the batch in lockstep, one read-back per decision -> (labels per row, decisions made)"""
    lstm, proj, voc = layers
    B = enc.shape[0]
    dev = enc.device
    rows = torch.arange(B, device=dev)
    h, c = torch.zeros((B, H), device=dev), torch.zeros((B, H), device=dev)
    t, s = np.zeros(B, np.int64), np.zeros(B, np.int64)
    labels = [[] for _ in range(B)]
    emit = np.ones(B, np.int32)                      # the start step on embed[blank]
    tokens = torch.full((B,), BLANK, dtype=torch.long, device=dev)
    g = torch.zeros((B, 1, J), device=dev)
    decisions = 0
    while True:
        if emit.any():
            _, h2, c2 = lstm.apply_device_varlen(embed_d[tokens].reshape(B, 1, E).contiguous(), lengths=emit, h0=h, c0=c, return_state=True)
            h, c = h2, c2
            gn = proj.apply_device(h.reshape(B, 1, H))
            mask = torch.from_numpy(emit.astype(bool)).to(dev)
            g = torch.where(mask[:, None, None], gn, g)
        live = t < T
        if not live.any():
            return labels, decisions
        tt = torch.from_numpy(np.minimum(t, T - 1)).to(dev)
        z = NL.rnnt_joint_device(enc[rows, tt].reshape(B, 1, J).contiguous(), g.contiguous(), "tanh")
        k = voc.apply_device(z.reshape(B, 1, J)).reshape(B, V).argmax(1).cpu().numpy()      # the read-back the next step waits for
        decisions += 1
        emit[:] = 0
        for b in range(B):
            if not live[b]:
                continue
            if k[b] == BLANK:
                t[b] += 1; s[b] = 0
            else:
                labels[b].append(int(k[b])); emit[b] = 1; s[b] += 1
                if s[b] == MAX_SYMBOLS:
                    t[b] += 1; s[b] = 0
        tokens = torch.from_numpy(np.where(emit == 1, k, BLANK)).to(dev)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    L = open_device()
    rng = np.random.default_rng(2024)
    m = model(rng)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    embed_d = d(m["embed"])
    dec = NL.RnntDecoder(embed_d, d(np.concatenate([m["W"].ravel(), m["U"].ravel(), m["b_i"], m["b_h"]])),
                         d(np.concatenate([m["Wp"].ravel(), m["bp"]])), d(np.concatenate([m["Wo"].ravel(), m["bo"]])), blank=BLANK,
                         joint_activation="tanh", max_symbols_per_frame=MAX_SYMBOLS)
    lstm = NL.LSTM(E, H, False, 1)
    lstm.set_weights(m["W"], m["U"], m["b_i"], m["b_h"])
    proj = NL.TimeDistributedDense(1, H, J); proj.set_weights(m["Wp"], m["bp"])
    voc = NL.TimeDistributedDense(1, J, V); voc.set_weights(m["Wo"], m["bo"])
    out = {"tool": "rnnt_decode_time", "repeats": repeats, "warmup": WARMUP, "source_hash": L.nntk_build_source_hash().decode(),
           "model": {"E": E, "H": H, "J": J, "V": V, "T": T, "max_symbols_per_frame": MAX_SYMBOLS}, "batches": []}
    for B in BATCHES:
        enc = d(rng.uniform(-1.5, 1.5, (B, T, J)).astype(np.float32))
        outs = dec._outputs(enc.device, B, MAX_SYMBOLS * T)
        ms, mm = timed(lambda: dec._decode(None, enc, None, MAX_SYMBOLS * T, outs), repeats, WARMUP).pair
        lengths = outs[2].cpu().numpy()
        labels = outs[0].cpu().numpy()
        hl = []
        for _ in range(WARMUP + repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_labels, decisions = host_loop(m, (lstm, proj, voc), enc, embed_d)
            torch.cuda.synchronize()
            hl.append(1e3 * (time.perf_counter() - t0))
        hl = hl[WARMUP:]
        same = sum(labels[b, :lengths[b]].tolist() == host_labels[b] for b in range(B))
        out["batches"].append({"batch": B, "decode_ms": ms, "decode_ms_min_max": mm,
                               "host_loop_ms": float(np.median(hl)), "host_loop_ms_min_max": [float(min(hl)), float(max(hl))],
                               "labels_total": int(lengths.sum()),
                               "host_loop_iterations": int(decisions), "rows_with_identical_labels": int(same),
                               "rows_per_workgroup": int(L.nntk_shim_rnnt_dec_rows_per_group(B, H, J, V))})
    emit(out, "rnnt_decode_time")


if __name__ == "__main__":
    main()
