#!/usr/bin/env python3
"""What streaming CTC prefix beam search costs per push (csrc/hip/ctc_beam.hip, CtcBeamStream), next to the one-shot call in the same run:
python tools/ctc_beam_stream_time.py [repeats]      -> one JSON line, also written to profiles/ctc_beam_stream_time.json
B = 64 streams, C = 29, beam_width 16, nbest 1, a 1000-frame utterance per row, pushed in chunks of 10 and of 50 frames (a stack-like
chunk).  Three numbers per chunk size: the latency of one push in the middle of the stream (HIP events around a single push, median
of the repeats x pushes samples); the one-shot call on the whole utterance, as time per frame; and the sum over all pushes of one
stream (events around the whole stream, median of the repeats) against that one-shot call.  Warm-up: two whole streams / calls."""
import sys
import numpy as np
import torch
from timing import emit, open_device, timed, timed_marks
from nntoolkitcore_amd import layers as NL

B, T, CC, W, NBEST, MAX_LABELS = 64, 1000, 29, 16, 1, 512
CHUNKS = (10, 50)
WARMUP = 2


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    L = open_device()
    g = torch.Generator(device="cuda").manual_seed(B + T + CC)
    probs = torch.softmax(4 * torch.rand((B, T, CC), device="cuda", generator=g) - 2, -1)
    out = {"tool": "ctc_beam_stream_time", "repeats": repeats, "warmup": WARMUP, "source_hash": L.nntk_build_source_hash().decode(),
           "B": B, "T": T, "C": CC, "beam_width": W, "nbest": NBEST, "max_labels": MAX_LABELS, "chunks": []}

    ws = torch.empty(L.nntk_ctc_beam_workspace_floats(B, T, CC, W, 0), device="cuda")
    lab1 = torch.empty((B, NBEST, T), dtype=torch.int32, device="cuda")
    n1 = torch.empty((B, NBEST), dtype=torch.int32, device="cuda")
    sc1 = torch.empty((B, NBEST), device="cuda")
    one = lambda: NL.ctc_beam_decode_device(probs, None, 0, W, 0, NBEST, labels_out=lab1, out_lengths=n1, scores=sc1, workspace=ws)
    out["one_shot_ms"] = timed(one, repeats, WARMUP).dict
    out["one_shot_us_per_frame"] = 1e3 * out["one_shot_ms"]["median"] / T
    out["one_shot_workspace_bytes"] = 4 * ws.numel()

    for mf in CHUNKS:
        blocks = [probs[:, t:t + mf].contiguous() for t in range(0, T, mf)]
        nf = np.full(B, mf, np.int32)
        dec = NL.CtcBeamStream(B, mf, CC, 0, W, 0, NBEST, max_labels=MAX_LABELS)
        lab = torch.empty((B, NBEST, MAX_LABELS), dtype=torch.int32, device="cuda")
        n = torch.empty((B, NBEST), dtype=torch.int32, device="cuda")
        sc = torch.empty((B, NBEST), device="cuda")
        rows = np.arange(B, dtype=np.int32)

        def stream(events=None):
            dec.reset(rows)
            for i, x in enumerate(blocks):
                if events is not None:
                    events[i][0].record()
                dec.push(x, nf, labels_out=lab, out_lengths=n, scores=sc)
                if events is not None:
                    events[i][1].record()

        w = timed(stream, repeats, WARMUP).dict
        assert n.cpu().numpy().tobytes() == n1.cpu().numpy().tobytes() and sc.cpu().numpy().tobytes() == sc1.cpu().numpy().tobytes()
        pp = timed_marks(stream, len(blocks), repeats, len(blocks) // 4, 0).dict           # the stream's first quarter: short strings
        out["chunks"].append({"max_frames": mf, "pushes": len(blocks), "push_ms": pp, "push_us_per_frame": 1e3 * pp["median"] / mf,
                              "stream_ms": w, "stream_over_one_shot": w["median"] / out["one_shot_ms"]["median"],
                              "state_bytes": int(L.nntk_ctc_beam_stream_state_bytes(B, mf, CC, W, 0, MAX_LABELS))})
        dec.close()
    emit(out, "ctc_beam_stream_time")


if __name__ == "__main__":
    main()
