#!/usr/bin/env python3
"""What label timestamps cost the CTC prefix beam search (csrc/hip/ctc_beam.hip, the DETAIL instantiations), and that the calls
cost what they did:
python tools/ctc_beam_detail_time.py [--parent LIB [--rounds N]] [repeats]     -> one JSON line, also written to profiles/ctc_beam_detail_time.json
One-shot, at shapes of tools/ctc_beam_time.py: 512 x 250 x 40 with beam_width 16 and 64, 512 x 1000 x 1000 with beam_width 64 and
cutoff_top_n 40; nbest = 4.  The detail call next to the plain call of the same library, and the traffic detail adds (the gather of one
probability per reported label, two more [B][nbest][T] outputs written in full).  Stream: the shape of tools/ctc_beam_stream_time.py
(B 64, C 29, beam_width 16, nbest 1, max_labels 512, chunks of 10 and 50 frames), one push in the stream's later three quarters, with
and without detail (16 * max_labels more bytes of state per row and entry, half of them copied per push).
--parent LIB: the plain and the detail one-shot calls and one stream push (chunks of 10; plain and detail) of this library next to
those of another build (the parent commit's), by the A/B protocol of tools/timing.py.  A child goes through this tree's Python layer
with NNTK_LIB set: the C ABI of the two builds must be the same.  Timing as in tools/timing.py, repeats default 7."""
import json, os, sys
import numpy as np
import torch
from timing import ab_children, ab_figures, emit, open_device, ragged, timed, timed_marks

ONE_SHOT = ((512, 250, 40, 16, 0), (512, 250, 40, 64, 0), (512, 1000, 1000, 64, 40))     # B, T, C, beam_width, cutoff_top_n
NBEST = 4
SB, ST, SC, SW, SNBEST, SMAX_LABELS = 64, 1000, 29, 16, 1, 512
CHUNKS = (10, 50)
WARMUP = 2


def inputs(B, T, Cc):
    g = torch.Generator(device="cuda").manual_seed(B + T + Cc)
    probs = torch.softmax(4 * torch.rand((B, T, Cc), device="cuda", generator=g) - 2, -1)
    return probs, ragged(np.random.default_rng(T), T, B)


def one_shot(L, NL, shape, repeats):
    """-> (plain Timing, detail Timing, reported labels) of one shape; detail must leave labels, lengths and scores as they were"""
    B, T, Cc, W, cut = shape
    probs, il = inputs(B, T, Cc)
    ws = torch.empty(L.nntk_ctc_beam_workspace_floats(B, T, Cc, W, cut), device="cuda")
    lab = torch.empty((B, NBEST, T), dtype=torch.int32, device="cuda")
    n = torch.empty((B, NBEST), dtype=torch.int32, device="cuda")
    sc = torch.empty((B, NBEST), device="cuda")
    call = lambda **kw: NL.ctc_beam_decode_device(probs, il, 0, W, cut, NBEST, labels_out=lab, out_lengths=n, scores=sc, workspace=ws, **kw)
    plain = timed(call, repeats, WARMUP)
    assert torch.isfinite(sc[:, 0]).all()
    bits = (lab.cpu().numpy().tobytes(), n.cpu().numpy().tobytes(), sc.cpu().numpy().tobytes())
    detail = timed(lambda: call(detail=True), repeats, WARMUP)
    fr = call(detail=True)[3]
    assert bits == (lab.cpu().numpy().tobytes(), n.cpu().numpy().tobytes(), sc.cpu().numpy().tobytes())
    labels = int((fr >= 0).sum())
    del probs, ws
    torch.cuda.empty_cache()
    return plain, detail, labels


def stream_push(NL, probs, mf, detail, repeats):
    """-> the Timing of one push of mf frames in the stream's later three quarters"""
    blocks = [probs[:, t:t + mf].contiguous() for t in range(0, ST, mf)]
    nf, rows = np.full(SB, mf, np.int32), np.arange(SB, dtype=np.int32)
    dec = NL.CtcBeamStream(SB, mf, SC, 0, SW, 0, SNBEST, max_labels=SMAX_LABELS, detail=detail)

    def stream(events):
        dec.reset(rows)
        for i, x in enumerate(blocks):
            if events is not None:
                events[i][0].record()
            dec.push(x, nf)
            if events is not None:
                events[i][1].record()
    t = timed_marks(stream, len(blocks), repeats, len(blocks) // 4, WARMUP)
    dec.close()
    return t, len(blocks)


def ab_forms():
    return ["plain %d" % i for i in range(len(ONE_SHOT))] + ["detail %d" % i for i in range(len(ONE_SHOT))] + ["push plain", "push detail"]


def child(lib_path, repeats):
    """every form of ab_forms() on the build lib_path, in that order: a child process of --parent"""
    os.environ["NNTK_LIB"] = lib_path
    L = open_device()
    from nntoolkitcore_amd import layers as NL
    shots = [one_shot(L, NL, shape, repeats) for shape in ONE_SHOT]
    probs, _ = inputs(SB, ST, SC)
    pushes = [stream_push(NL, probs, CHUNKS[0], detail, repeats)[0] for detail in (False, True)]
    print(json.dumps([s[0].dict for s in shots] + [s[1].dict for s in shots] + [p.dict for p in pushes]))


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1], int(args[2]))
    parent = None
    if args and args[0] == "--parent":
        parent, args = os.path.abspath(args[1]), args[2:]
    rounds = 2
    if args and args[0] == "--rounds":                    # a re-measurement of --parent with more rounds than the protocol's two
        rounds, args = int(args[1]), args[2:]
    repeats = int(args[0]) if args else 7
    out = {"tool": "ctc_beam_detail_time", "repeats": repeats, "warmup": WARMUP, "nbest": NBEST}
    if parent:
        from nntoolkitcore_amd import capi                # the children run before this process opens the device
        runs = ab_children(__file__, "--child", capi.LIB_PATH, parent, repeats, rounds)
        out["vs_parent_rounds"] = rounds
        out["vs_parent"] = [{"form": form, **ab_figures(*([r[i]["median"] for r in runs[k]] for k in ("this", "parent")))}
                            for i, form in enumerate(ab_forms())]
    L = open_device()
    from nntoolkitcore_amd import layers as NL
    out["source_hash"] = L.nntk_build_source_hash().decode()
    out["one_shot"] = []
    for shape in ONE_SHOT:
        B, T, Cc, W, cut = shape
        plain, detail, labels = one_shot(L, NL, shape, repeats)
        out["one_shot"].append({"B": B, "T": T, "C": Cc, "beam_width": W, "cutoff_top_n": cut, "plain_ms": plain.dict, "detail_ms": detail.dict,
                                "detail_over_plain": detail.dict["median"] / plain.dict["median"], "reported_labels": labels,
                                "detail_bytes_written": 2 * 4 * B * NBEST * T, "detail_bytes_gathered": 4 * labels})

    probs, _ = inputs(SB, ST, SC)
    out["stream"] = {"B": SB, "T": ST, "C": SC, "beam_width": SW, "nbest": SNBEST, "max_labels": SMAX_LABELS, "chunks": []}
    for mf in CHUNKS:
        row = {"max_frames": mf}
        for detail in (False, True):
            key = "detail" if detail else "plain"
            t, row["pushes"] = stream_push(NL, probs, mf, detail, repeats)
            row[key + "_push_ms"] = t.dict
            row[key + "_state_bytes"] = int(L.nntk_ctc_beam_stream_state_bytes_opt(SB, mf, SC, SW, 0, SMAX_LABELS, 0, int(detail)))
        row["detail_over_plain"] = row["detail_push_ms"]["median"] / row["plain_push_ms"]["median"]
        row["detail_string_bytes_per_push_at_most"] = 2 * 8 * SB * SW * SMAX_LABELS      # read one half, write the other
        out["stream"]["chunks"].append(row)
    emit(out, "ctc_beam_detail_time")


if __name__ == "__main__":
    main()
