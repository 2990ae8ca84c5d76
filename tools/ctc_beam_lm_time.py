#!/usr/bin/env python3
"""What language-model fusion costs in the CTC prefix beam search (csrc/hip/ctc_beam.hip, the LM instantiations):
python tools/ctc_beam_lm_time.py [--parent LIB] [repeats]      -> one JSON line, also written to profiles/ctc_beam_lm_time.json
(--parent LIB: the three calls of this library next to those of another build, the parent commit's, by the A/B protocol of
tools/timing.py; a child goes through this tree's Python layer with NNTK_LIB set)
One decoding-sized shape, B = 64, T = 500, C = 64, beam_width 32, no class cut, nbest 4; three calls on the same posteriors:
nntk_ctc_beam_decode_lm_device with a sparse random trigram of about 50 k arcs, the same call with the unit model (alpha = beta = 0: the
same walks, every factor one), and nntk_ctc_beam_decode_device.  Timed by tools/timing.py.
probes_per_frame: the 16-byte arc records a row's frame reads in its binary searches -- beam_width * (C - 1) extend cells plus
beam_width re-lookups, each the mean over the table's two-label states and all classes of the probes of one walk (a binary search
over k arcs costs floor(log2 k) + 1 probes on a miss)."""
import json, os, sys
import numpy as np
import torch
from timing import ab_children, ab_figures, emit, open_device, timed

B, T, CC, W, NBEST, BLANK = 64, 500, 64, 32, 4, 0
WARMUP = 2


def trigram(seed, per_state):
    """every one-label and two-label context over the C - 1 labels; state 0 and the one-label states hold every label, a two-label
    state per_state random ones"""
    rng = np.random.default_rng(seed)
    labels = np.array([c for c in range(CC) if c != BLANK])
    n1 = len(labels)
    idx = {int(c): i for i, c in enumerate(labels)}
    one = lambda a: 1 + idx[a]
    two = lambda a, b: 1 + n1 + idx[a] * n1 + idx[b]
    arc_begin, lab, nxt, bo = [0], [], [], []
    for s in range(1 + n1 + n1 * n1):
        if s == 0:
            mine, hist = labels, ()
        elif s <= n1:
            mine, hist = labels, (int(labels[s - 1]),)
        else:
            q = s - 1 - n1
            mine, hist = np.sort(rng.choice(labels, per_state, replace=False)), (int(labels[q // n1]), int(labels[q % n1]))
        for c in mine:
            h = (hist + (int(c),))[-2:]
            lab.append(int(c)); nxt.append(one(h[0]) if len(h) == 1 else two(*h))
        arc_begin.append(len(lab))
        bo.append(-1 if s == 0 else 0 if s <= n1 else one(hist[1]))
    na, ns = len(lab), len(bo)
    return dict(n_classes=CC, blank=BLANK, arc_begin=arc_begin, arc_label=lab, arc_logp=np.log(rng.uniform(0.02, 0.9, na)), arc_next=nxt,
                backoff_state=bo, backoff_logw=np.log(rng.uniform(0.2, 0.9, ns)) * (np.arange(ns) > 0), final_logp=None, start_state=0,
                unk_logp=float(np.log(1e-3)))


def probes_per_walk(per_state):
    n1 = CC - 1
    miss2, full = int(np.floor(np.log2(per_state))) + 1, int(np.floor(np.log2(n1))) + 1      # upper bounds of one search
    hit = per_state / n1
    return hit * miss2 + (1 - hit) * (miss2 + full)


def main():
    args = sys.argv[1:]
    child = bool(args) and args[0] == "--child"              # --child LIB repeats: the three medians of that build, for --parent
    parent = None
    if child:
        os.environ["NNTK_LIB"], args = args[1], args[2:]
    elif args and args[0] == "--parent":
        parent, args = os.path.abspath(args[1]), args[2:]
    repeats = int(args[0]) if args else 5
    vs_parent = None
    if parent:
        from nntoolkitcore_amd import capi                   # the children run before this process opens the device
        runs = ab_children(__file__, "--child", capi.LIB_PATH, parent, repeats)
        vs_parent = [{"form": form, **ab_figures(*([r[i] for r in runs[k]] for k in ("this", "parent")))}
                     for i, form in enumerate(("lm", "unit_lm", "acoustic"))]
    L = open_device()
    from nntoolkitcore_amd import layers as NL
    per_state = 12
    t = trigram(1, per_state)
    g = torch.Generator(device="cuda").manual_seed(B + T + CC)
    probs = torch.softmax(4 * torch.rand((B, T, CC), device="cuda", generator=g) - 2, -1)
    il = np.full(B, T, np.int32)
    ws = torch.empty(L.nntk_ctc_beam_lm_workspace_floats(B, T, CC, W, 0), device="cuda")
    lab = torch.empty((B, NBEST, T), dtype=torch.int32, device="cuda")
    n = torch.empty((B, NBEST), dtype=torch.int32, device="cuda")
    sc = torch.empty((B, NBEST), device="cuda")
    kw = dict(labels_out=lab, out_lengths=n, scores=sc, workspace=ws)
    lm = NL.NgramLm.from_arrays(alpha=0.5, beta=0.25, **t)
    unit = NL.NgramLm.from_arrays(alpha=0.0, beta=0.0, **t)
    t_lm = timed(lambda: NL.ctc_beam_decode_lm_device(probs, lm, il, BLANK, W, 0, NBEST, **kw), repeats, WARMUP)
    assert torch.isfinite(sc[:, 0]).all()
    t_unit = timed(lambda: NL.ctc_beam_decode_lm_device(probs, unit, il, BLANK, W, 0, NBEST, **kw), repeats, WARMUP)
    unit_sc = sc.clone()
    t_ac = timed(lambda: NL.ctc_beam_decode_device(probs, il, BLANK, W, 0, NBEST, **kw), repeats, WARMUP)
    assert torch.equal(unit_sc, sc), "the unit model must give the acoustic bits"
    if child:
        return print(json.dumps([t_lm.median, t_unit.median, t_ac.median]))
    walk = probes_per_walk(per_state)
    out = {"tool": "ctc_beam_lm_time", "repeats": repeats, "warmup": WARMUP, "source_hash": L.nntk_build_source_hash().decode(),
           "B": B, "T": T, "C": CC, "beam_width": W, "nbest": NBEST, "lm_arcs": len(t["arc_label"]), "lm_states": len(t["backoff_state"]),
           "lm_device_bytes": lm.device_bytes(), "lm_ms": t_lm[0], "lm_ms_min_max": t_lm[1:], "unit_lm_ms": t_unit[0],
           "unit_lm_ms_min_max": t_unit[1:], "acoustic_ms": t_ac[0], "acoustic_ms_min_max": t_ac[1:], "lm_over_acoustic": t_lm[0] / t_ac[0],
           "unit_over_acoustic": t_unit[0] / t_ac[0], "lm_over_unit": t_lm[0] / t_unit[0], "probes_per_walk": walk,
           "probes_per_frame": walk * (W * (CC - 1) + W), "us_per_frame": {"lm": 1e3 * t_lm[0] / T, "acoustic": 1e3 * t_ac[0] / T}}
    if vs_parent:
        out["vs_parent"] = vs_parent
    emit(out, "ctc_beam_lm_time")


if __name__ == "__main__":
    main()
