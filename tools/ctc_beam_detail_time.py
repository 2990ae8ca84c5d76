#!/usr/bin/env python3
"""What label timestamps cost the CTC prefix beam search (csrc/hip/ctc_beam.hip, the DETAIL instantiations), and that the calls
without them cost what they did:
python tools/ctc_beam_detail_time.py [--parent LIB] [repeats]     -> one JSON line, also written to profiles/ctc_beam_detail_time.json
One-shot, at shapes of tools/ctc_beam_time.py: 512 x 250 x 40 with beam_width 16 and 64, 512 x 1000 x 1000 with beam_width 64 and
cutoff_top_n 40; nbest = 4.  The detail call next to the plain call of the same library, and the traffic detail adds (the gather of one
probability per reported label, two more [B][nbest][T] outputs written in full).  Stream: the shape of tools/ctc_beam_stream_time.py
(B 64, C 29, beam_width 16, nbest 1, max_labels 512, chunks of 10 and 50 frames), one push in the stream's later three quarters, with
and without detail (16 * max_labels more bytes of state per row and entry, half of them copied per push).
--parent LIB: the plain one-shot calls of this library next to those of another build (the parent commit's), by the A/B protocol of
tools/timing.py; a child binds only what both libraries have.  Timing as in tools/timing.py, repeats default 7."""
import ctypes as C
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


def plain_only(lib_path, repeats):
    """the plain one-shot calls of any build, bound by hand: a child process of --parent"""
    lib = C.CDLL(lib_path)
    lib.nntk_ctc_beam_workspace_floats.restype = C.c_size_t
    vp = C.c_void_p
    lib.nntk_ctc_beam_decode_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    torch.cuda.set_device(0)
    out = []
    for B, T, Cc, W, cut in ONE_SHOT:
        probs, il = inputs(B, T, Cc)
        ws = torch.empty(lib.nntk_ctc_beam_workspace_floats(B, T, Cc, W, cut), device="cuda")
        lab = torch.empty((B, NBEST, T), dtype=torch.int32, device="cuda")
        n = torch.empty((B, NBEST), dtype=torch.int32, device="cuda")
        sc = torch.empty((B, NBEST), device="cuda")

        def call():
            rc = lib.nntk_ctc_beam_decode_device(probs.data_ptr(), B, T, Cc, il.ctypes.data, 0, W, cut, NBEST, lab.data_ptr(), n.data_ptr(),
                                                 sc.data_ptr(), ws.data_ptr())
            assert rc == 0
        out.append(timed(call, repeats, WARMUP).dict)
        assert torch.isfinite(sc[:, 0]).all()
        del probs, ws
        torch.cuda.empty_cache()
    print(json.dumps(out))


def main():
    args = sys.argv[1:]
    if args and args[0] == "--plain-only":
        return plain_only(args[1], int(args[2]))
    parent = None
    if args and args[0] == "--parent":
        parent, args = os.path.abspath(args[1]), args[2:]
    repeats = int(args[0]) if args else 7
    out = {"tool": "ctc_beam_detail_time", "repeats": repeats, "warmup": WARMUP, "nbest": NBEST}
    if parent:
        from nntoolkitcore_amd import capi                # the children run before this process opens the device
        runs = ab_children(__file__, "--plain-only", capi.LIB_PATH, parent, repeats)
        out["plain_vs_parent"] = [{"B": B, "T": T, "C": Cc, "beam_width": W, "cutoff_top_n": cut,
                                   **ab_figures(*([r[i]["median"] for r in runs[k]] for k in ("this", "parent")))}
                                  for i, (B, T, Cc, W, cut) in enumerate(ONE_SHOT)]
    L = open_device()
    from nntoolkitcore_amd import layers as NL
    out["source_hash"] = L.nntk_build_source_hash().decode()
    out["one_shot"] = []
    for B, T, Cc, W, cut in ONE_SHOT:
        probs, il = inputs(B, T, Cc)
        ws = torch.empty(L.nntk_ctc_beam_workspace_floats(B, T, Cc, W, cut), device="cuda")
        lab = torch.empty((B, NBEST, T), dtype=torch.int32, device="cuda")
        n = torch.empty((B, NBEST), dtype=torch.int32, device="cuda")
        sc = torch.empty((B, NBEST), device="cuda")
        plain = timed(lambda: NL.ctc_beam_decode_device(probs, il, 0, W, cut, NBEST, labels_out=lab, out_lengths=n, scores=sc, workspace=ws),
                      repeats, WARMUP).dict
        bits = (lab.cpu().numpy().tobytes(), n.cpu().numpy().tobytes(), sc.cpu().numpy().tobytes())
        detail = timed(lambda: NL.ctc_beam_decode_device(probs, il, 0, W, cut, NBEST, labels_out=lab, out_lengths=n, scores=sc, workspace=ws,
                                                         detail=True), repeats, WARMUP).dict
        fr = NL.ctc_beam_decode_device(probs, il, 0, W, cut, NBEST, labels_out=lab, out_lengths=n, scores=sc, workspace=ws, detail=True)[3]
        assert bits == (lab.cpu().numpy().tobytes(), n.cpu().numpy().tobytes(), sc.cpu().numpy().tobytes())
        labels = int((fr >= 0).sum())
        out["one_shot"].append({"B": B, "T": T, "C": Cc, "beam_width": W, "cutoff_top_n": cut, "plain_ms": plain, "detail_ms": detail,
                                "detail_over_plain": detail["median"] / plain["median"], "reported_labels": labels,
                                "detail_bytes_written": 2 * 4 * B * NBEST * T, "detail_bytes_gathered": 4 * labels})
        del probs, ws
        torch.cuda.empty_cache()

    probs, _ = inputs(SB, ST, SC)
    out["stream"] = {"B": SB, "T": ST, "C": SC, "beam_width": SW, "nbest": SNBEST, "max_labels": SMAX_LABELS, "chunks": []}
    rows = np.arange(SB, dtype=np.int32)
    for mf in CHUNKS:
        blocks = [probs[:, t:t + mf].contiguous() for t in range(0, ST, mf)]
        nf = np.full(SB, mf, np.int32)
        row = {"max_frames": mf, "pushes": len(blocks)}
        for detail in (False, True):
            dec = NL.CtcBeamStream(SB, mf, SC, 0, SW, 0, SNBEST, max_labels=SMAX_LABELS, detail=detail)

            def stream(events):
                dec.reset(rows)
                for i, x in enumerate(blocks):
                    if events is not None:
                        events[i][0].record()
                    dec.push(x, nf)
                    if events is not None:
                        events[i][1].record()
            key = "detail" if detail else "plain"
            row[key + "_push_ms"] = timed_marks(stream, len(blocks), repeats, len(blocks) // 4, WARMUP).dict
            row[key + "_state_bytes"] = int(L.nntk_ctc_beam_stream_state_bytes_opt(SB, mf, SC, SW, 0, SMAX_LABELS, 0, int(detail)))
            dec.close()
        row["detail_over_plain"] = row["detail_push_ms"]["median"] / row["plain_push_ms"]["median"]
        row["detail_string_bytes_per_push_at_most"] = 2 * 8 * SB * SW * SMAX_LABELS      # read one half, write the other
        out["stream"]["chunks"].append(row)
    emit(out, "ctc_beam_detail_time")


if __name__ == "__main__":
    main()
