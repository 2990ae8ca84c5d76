#!/usr/bin/env python3
"""What training the prediction network costs (csrc/hip/rnnt_pred.hip, csrc/host/rnnt_pred.c):
python tools/rnnt_predictor_time.py [repeats] [out.json]      -> profiles/rnnt_predictor_time.json (timed by tools/timing.py)
Per shape (B, max_label_len, V, E = H = J): the predictor handle's forward + backward next to the recipe a caller had to write before --
the lookup in numpy and an upload, the same device calls, a download of d_dX, np.add.at and an upload of d embed -- and the table
gradient alone on the transducer's id distribution (the start symbol once per batch row) and on uniform ids, each against the time to
write V E floats and read rows E floats at the HBM copy rate DESIGN.md uses (6.29 TB/s measured)."""
import ctypes as C
import json, os, sys
import numpy as np
import torch
from timing import ROOT, open_device, ragged, timed
from nntoolkitcore_amd import capi, layers as NL

SHAPES = ((64, 40, 1024, 512), (64, 40, 4096, 512))
WARMUP = 3
HBM_COPY_BYTES_PER_S = 6.29e12
DP = lambda t: C.c_void_p(t.data_ptr())


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    dest = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "rnnt_predictor_time.json")
    L = open_device()
    out = {"tool": "rnnt_predictor_time", "repeats": repeats, "warmup": WARMUP, "source_hash": L.nntk_build_source_hash().decode(),
           "hbm_copy_bytes_per_s": HBM_COPY_BYTES_PER_S, "shapes": []}
    for B, U, V, W in SHAPES:
        E = H = J = W
        U1 = U + 1
        rng = np.random.default_rng(V)
        u = lambda sc, *s: torch.from_numpy(rng.uniform(-sc, sc, s).astype(np.float32)).cuda()
        embed, lstm, proj = u(1.0, V, E), u(H ** -0.5, 4 * H * (E + H + 2)), u(H ** -0.5, (H + 1) * J)
        lab = rng.integers(1, V, (B, U)).astype(np.int32)
        ll = ragged(rng, U, B)
        dpred = u(1.0, B, U1, J)
        p = NL.RnntPredictor(V, E, H, J, B, U)
        p.load_weights(embed, lstm, proj)
        pred, dembed, dlstm, dproj = torch.empty((B, U1, J), device="cuda"), torch.empty_like(embed), torch.empty_like(lstm), torch.empty_like(proj)

        def handle():
            p.forward(lab, ll, pred=pred)
            p.backward(dpred, dembed=dembed, dlstm=dlstm, dproj=dproj)

        # the host-lookup recipe: what a caller does without the handle
        ids = np.full((B, U1), -1, np.int32)
        ids[:, 0] = 0
        for b in range(B):
            ids[b, 1:ll[b] + 1] = lab[b, :ll[b]]
        lens = (ll + 1).astype(np.int32)
        live = torch.from_numpy((ids >= 0).astype(np.float32)).cuda()[..., None]
        embed_h = embed.cpu().numpy()
        rl = NL.LSTM(E, H, True, U1, mini_batch=B)
        assert L.LSTMLoadWeightsDevice(rl.h, DP(lstm)) == 0, capi.last_error()
        tdd = L.TimeDistributedDenseCreateForTraining(L.TimeDistributedDenseConfigCreate(U1, L.DenseConfigCreate(H, J, None)), capi.ConvTrainingConfig(B))
        assert tdd and L.TimeDistributedDenseLoadWeightsDevice(tdd, DP(proj)) == 0, capi.last_error()
        h, r_pred, dh, dX = (torch.empty((B, U1, n), device="cuda") for n in (H, J, H, E))
        r_dlstm, r_dproj = torch.empty_like(lstm), torch.empty_like(proj)
        r_dembed = [None]

        def recipe():
            x = torch.from_numpy(np.where((ids >= 0)[..., None], embed_h[np.maximum(ids, 0)], np.float32(0))).cuda()
            assert L.LSTMApplyTrainingBatchDeviceVarLen(rl.h, DP(x), DP(h), lens.ctypes.data_as(capi.ip), None, None, None, None) == 0
            assert L.TimeDistributedDenseApplyTrainingBatchDevice(tdd, DP(h), DP(r_pred)) == 0
            dpm = dpred * live                                              # (finite here; a caller has to mask the padding rows)
            r_dlstm.zero_(); r_dproj.zero_()
            assert L.TimeDistributedDenseCalculateGradientDevice(tdd, DP(r_dproj), DP(dh), DP(dpm)) == 0
            assert L.LSTMCalculateGradientDeviceVarLen(rl.h, DP(r_dlstm), DP(dX), DP(dh), None, None, None, None) == 0
            g = np.zeros((V, E), np.float32)
            dx = dX.cpu().numpy().reshape(-1, E)
            np.add.at(g, ids.reshape(-1)[ids.reshape(-1) >= 0], dx[ids.reshape(-1) >= 0])
            r_dembed[0] = torch.from_numpy(g).cuda()

        t_h, t_r = timed(handle, repeats, WARMUP), timed(recipe, repeats, WARMUP)
        torch.cuda.synchronize()
        assert torch.equal(pred, r_pred) and torch.equal(dlstm, r_dlstm) and torch.equal(dproj, r_dproj)
        assert torch.allclose(dembed, r_dembed[0], rtol=1e-4, atol=1e-5)
        # the table gradient alone
        rows = B * U1
        ws = torch.empty(L.nntk_embedding_workspace_floats(rows, V, E), device="cuda")
        dout = u(1.0, rows, E)
        uniform = rng.integers(0, V, rows).astype(np.int32)
        t_hot = timed(lambda: NL.embedding_gradient_device(dout, ids, V, dtable=dembed, workspace=ws), repeats, WARMUP)
        t_uni = timed(lambda: NL.embedding_gradient_device(dout, uniform, V, dtable=dembed, workspace=ws), repeats, WARMUP)
        t_look = timed(lambda: NL.embedding_lookup_device(embed, ids, out=dX.view(rows, E)), repeats, WARMUP)
        bound_ms = 1e3 * 4.0 * (V * E + rows * E) / HBM_COPY_BYTES_PER_S
        out["shapes"].append({
            "B": B, "max_label_len": U, "V": V, "E": E, "H": H, "J": J, "rows": rows, "live_rows": int((ids >= 0).sum()),
            "handle_forward_backward_ms": t_h[0], "handle_ms_min_max": t_h[1:],
            "host_lookup_recipe_ms": t_r[0], "host_lookup_recipe_ms_min_max": t_r[1:], "recipe_over_handle": t_r[0] / t_h[0],
            "gradient_transducer_ids_ms": t_hot[0], "gradient_transducer_ids_ms_min_max": t_hot[1:],
            "gradient_uniform_ids_ms": t_uni[0], "gradient_uniform_ids_ms_min_max": t_uni[1:],
            "gradient_hot_over_uniform": t_hot[0] / t_uni[0],
            "gradient_memory_bound_ms": bound_ms, "gradient_transducer_fraction_of_bound": bound_ms / t_hot[0],
            "gradient_uniform_fraction_of_bound": bound_ms / t_uni[0], "lookup_ms": t_look[0], "lookup_ms_min_max": t_look[1:],
            "handle_device_bytes": p.device_bytes()})
        p.destroy(); rl.destroy(); L.TimeDistributedDenseDestroy(tdd)
        torch.cuda.empty_cache()
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
    with open(dest, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
