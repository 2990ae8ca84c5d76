#!/usr/bin/env python3
"""What streaming the token-and-duration beam search costs (csrc/hip/rnnt_tdt_beam.hip, the STREAM instantiations) over the one-shot call:
python tools/rnnt_tdt_beam_stream_time.py [repeats]      -> profiles/rnnt_tdt_beam_stream_time.json and the same JSON line on stdout
The model and shape of tools/rnnt_tdt_beam_time.py (E = H = J = 512, V = 1024, T = 100, durations 0 .. 4, max_symbols_per_frame 3).  Per
beam_width (4, 8) and batch (1, 16): the milliseconds of the one-shot call on the whole rows (tools/timing.py), timed twice -- the
spread of its two medians is the margin for the ratios -- and of a whole stream, a reset and T frames pushed in chunks of 4, 16 and 64,
with `stream_over_one_shot` next to the expected bound 1 + (Dmax - 1) / chunk: a push runs its last Dmax - 1 frames a second time, and
copies the row's block once.  A launch lasts as long as its slowest row, so next to the times stand the kernel's own counters (frames
joined, LSTM steps), summed over the pushes for the slowest row of each push, and the one-shot call's for its slowest row.  The last
push's outputs are checked against the one-shot call's bits.  Reported as measured."""
import sys
import numpy as np
import torch
from timing import emit, open_device, timed
from nntoolkitcore_amd import layers as NL
from rnnt_tdt_beam_time import T, WARMUP, WIDTHS, BATCHES
from rnnt_tdt_decode_time import BLANK, DURATIONS, E, H, J, MAX_SYMBOLS, V, model

CHUNKS = (4, 16, 64)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    L = open_device()
    rng = np.random.default_rng(2024)
    m = model(rng)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tdt = NL.RnntDecoder(d(m["embed"]), d(np.concatenate([m["W"].ravel(), m["U"].ravel(), m["b_i"], m["b_h"]])),
                         d(np.concatenate([m["Wp"].ravel(), m["bp"]])),
                         d(np.concatenate([np.concatenate([m["Wo"], m["Wd"]], 1).ravel(), m["bo"], m["bd"]])), blank=BLANK,
                         joint_activation="tanh", max_symbols_per_frame=MAX_SYMBOLS, durations=DURATIONS)
    out = {"tool": "rnnt_tdt_beam_stream_time", "repeats": repeats, "warmup": WARMUP, "source_hash": L.nntk_build_source_hash().decode(),
           "model": {"E": E, "H": H, "J": J, "V": V, "T": T, "max_symbols_per_frame": MAX_SYMBOLS, "durations": list(DURATIONS)}, "runs": []}
    ML, dmax = MAX_SYMBOLS * T, max(DURATIONS)
    for B in BATCHES:
        enc = d(rng.uniform(-1.5, 1.5, (B, T, J)).astype(np.float32))
        for W in WIDTHS:
            want, ws = tdt._tdt_beam(enc, None, W, W, ML)
            one_shot = lambda: tdt._tdt_beam(enc, None, W, W, ML, ws)
            a = timed(one_shot, repeats, WARMUP)
            stat = lambda w: w[(B + 3) // 4 * 4:(B + 3) // 4 * 4 + 2 * B].view(torch.int32).cpu().numpy().reshape(B, 2)   # joined | LSTM steps
            run = {"batch": B, "beam_width": W, "one_shot_ms": a.median, "one_shot_ms_min_max": [a.min, a.max],
                   "one_shot_frames_joined_slowest_row": int(stat(ws)[:, 0].max()),
                   "one_shot_lstm_steps_slowest_row": int(stat(ws)[:, 1].max()), "streams": []}
            stream = NL.RnntTdtBeamStream(tdt, B, W, ML)
            for chunk in CHUNKS:
                parts = [enc[:, t:t + chunk].contiguous() for t in range(0, T, chunk)]

                def pushes():
                    stream.reset()
                    for p in parts:
                        got = stream.push(p, None, W)
                    return got
                s = timed(pushes, repeats, WARMUP)
                torch.cuda.synchronize()
                same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(pushes(), want))
                stream.reset()
                joined = []                                                          # untimed: every row's frames joined | LSTM steps, per push
                for p in parts:
                    stream.push(p, None, W)
                    joined.append(stat(stream.ws))
                run["streams"].append({"chunk": chunk, "pushes": len(parts), "stream_ms": s.median, "stream_ms_min_max": [s.min, s.max],
                                       "stream_over_one_shot": s.median / a.median, "expected_bound": 1 + (dmax - 1) / chunk,
                                       "last_push_is_one_shot_bits": bool(same),
                                       "frames_joined_slowest_row_of_each_push": int(sum(j[:, 0].max() for j in joined)),
                                       "lstm_steps_slowest_row_of_each_push": int(sum(j[:, 1].max() for j in joined)),
                                       "lstm_steps_mean_row": float(sum(j[:, 1].sum() for j in joined) / B)})
            again = timed(one_shot, repeats, WARMUP)
            run.update(one_shot_again_ms=again.median, one_shot_spread=abs(a.median - again.median) / (0.5 * (a.median + again.median)),
                       state_mib=float(L.nntk_rnnt_tdt_beam_state_bytes(tdt.h, B, W, ML, 0, 0) / 2 ** 20))
            stream.close()
            out["runs"].append(run)
    emit(out, "rnnt_tdt_beam_stream_time")


if __name__ == "__main__":
    main()
