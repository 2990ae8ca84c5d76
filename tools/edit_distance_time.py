#!/usr/bin/env python3
"""What the error counts cost (csrc/hip/edit_distance.hip), next to the beam search that produces the list they are taken of:
python tools/edit_distance_time.py [repeats]      -> one JSON line, also written to profiles/edit_distance_time.json
batch 512 x n_hyp 8 (nntk_ctc_beam_decode_device, C = 40, beam_width 16, nbest 8) at T = 110 and T = 1000: hypotheses near 100 and
near 1000 tokens.  A row's reference is its best hypothesis with every tenth token redrawn, one in twenty dropped and one in twenty
doubled.  Per shape: the decode call, nntk_edit_distance_device in unit mode and in word mode (class 1 as the separator), the MWER
call on the counts, and cell updates per second = sum over the pairs of (m + 1)(n + 1) over the unit call's time.  The edit distance
call includes the stream-ordered copy of the host references.  Timed by tools/timing.py."""
import sys
import numpy as np
import torch
from timing import emit, open_device, timed
from nntoolkitcore_amd import layers as NL

B, C, W, NBEST, SEP = 512, 40, 16, 8, 1
FRAMES = (110, 1000)
WARMUP = 2


def references(rng, labels, lengths):
    refs = []
    for b in range(labels.shape[0]):
        r = []
        for t in labels[b, 0, :max(int(lengths[b, 0]), 0)].tolist():
            u = rng.random()
            if u < 0.05:
                continue
            r.append(int(rng.integers(1, C)) if u < 0.15 else t)
            if u > 0.95:
                r.append(t)
        refs.append(r[:4000])
    return refs


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    L = open_device()
    out = {"tool": "edit_distance_time", "repeats": repeats, "warmup": WARMUP, "source_hash": L.nntk_build_source_hash().decode(),
           "B": B, "n_hyp": NBEST, "C": C, "beam_width": W, "shapes": []}
    for T in FRAMES:
        g = torch.Generator(device="cuda").manual_seed(B + T + C)
        probs = torch.softmax(4 * torch.rand((B, T, C), device="cuda", generator=g) - 2, -1)
        ws = torch.empty(L.nntk_ctc_beam_workspace_floats(B, T, C, W, 0), device="cuda")
        lab = torch.empty((B, NBEST, T), dtype=torch.int32, device="cuda")
        n = torch.empty((B, NBEST), dtype=torch.int32, device="cuda")
        sc = torch.empty((B, NBEST), device="cuda")
        t_dec = timed(lambda: NL.ctc_beam_decode_device(probs, None, 0, W, 0, NBEST, labels_out=lab, out_lengths=n, scores=sc, workspace=ws),
                      repeats, WARMUP)
        torch.cuda.synchronize()
        h_lab, h_n = lab.cpu().numpy(), n.cpu().numpy()
        refs = references(np.random.default_rng(T), h_lab, h_n)
        ref_len = np.array([len(r) for r in refs], np.int32)
        ref = np.zeros((B, max(1, int(ref_len.max()))), np.int32)
        for b, r in enumerate(refs):
            ref[b, :len(r)] = r
        ews = torch.empty(L.nntk_edit_distance_workspace_floats(B, NBEST, T, ref.shape[1]), device="cuda")
        counts = torch.empty((B, NBEST, 4), dtype=torch.int32, device="cuda")
        units = torch.empty(B, dtype=torch.int32, device="cuda")
        risk, dlogp = torch.empty(B, device="cuda"), torch.empty((B, NBEST), device="cuda")
        row = {"T": T, "decode_ms": t_dec[0], "decode_ms_min_max": t_dec[1:], "mean_hyp_len": float(h_n[h_n >= 0].mean()),
               "mean_ref_len": float(ref_len.mean()), "max_ref_len": int(ref.shape[1])}
        for name, sep in (("unit", -1), ("word", SEP)):
            t = timed(lambda: NL.edit_distance_device(lab, n, ref, ref_len, sep=sep, counts=counts, ref_units=units, workspace=ews),
                      repeats, WARMUP)
            torch.cuda.synchronize()
            row[name + "_ms"], row[name + "_ms_min_max"] = t[0], t[1:]
            row[name + "_over_decode"] = t[0] / t_dec[0]
            row[name + "_error_rate"] = NL.error_rate(counts, units)
            row[name + "_mean_ref_units"] = float(units.float().mean())
            if sep < 0:
                cells = float(((np.maximum(h_n, 0) + 1.0) * (ref_len[:, None] + 1.0)).sum())
                row["cells"], row["cell_updates_per_s"] = cells, cells / (1e-3 * t[0])
                t_m = timed(lambda: NL.mwer_device(sc, counts, risk=risk, dlogp=dlogp), repeats, WARMUP)
                row["mwer_ms"], row["mwer_ms_min_max"] = t_m[0], t_m[1:]
                assert torch.isfinite(risk).all() and torch.isfinite(dlogp).all()
        out["shapes"].append(row)
        del probs, ws, ews, lab
        torch.cuda.empty_cache()
    emit(out, "edit_distance_time")


if __name__ == "__main__":
    main()
