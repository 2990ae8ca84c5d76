"""What the tools/*_time.py scripts share: event timing, the device preamble, ragged lengths, the JSON line, and the protocol that
measures this build of the library against another one (the parent commit's).  Nothing here knows a feature, and importing it does no
device work.

The A/B protocol: every measurement runs in a fresh child process; the children run before the calling process
opens the device; this and parent alternate, this first, `rounds` (2) times each; the spread of one library's medians over its rounds is
its run-to-run noise, the yardstick for the ratio of the two means."""
import json, os, subprocess, sys
from typing import NamedTuple
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)                                  # the tools import nntoolkitcore_amd from the tree they stand in


class Timing(NamedTuple):
    """median, min, max in ms; the tuple itself is the triple some tools emit (t[0], t[1:])"""
    median: float
    min: float
    max: float

    @classmethod
    def of(cls, ms):
        return cls(float(np.median(ms)), float(min(ms)), float(max(ms)))

    @property
    def dict(self):
        return self._asdict()

    @property
    def pair(self):
        return self.median, [self.min, self.max]


def _event():
    return torch.cuda.Event(enable_timing=True)


def timed(fn, repeats, warmup=2, inner=1):
    """`warmup` calls, then `repeats` event pairs, each around `inner` back-to-back calls of fn -> Timing of the ms per call"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = _event(), _event()
        a.record()
        for _ in range(inner):
            fn()
        b.record(); b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return Timing.of(ms)


def timed_marks(run, marks, repeats, skip=0, warmup=2):
    """run(pairs) records pairs[i][0] and pairs[i][1] around its i-th mark, run(None) records nothing.  `warmup` runs without events,
    then `repeats` runs with `marks` event pairs each -> Timing over the marks of all runs, the first `skip` of each run left out"""
    for _ in range(warmup):
        run(None)
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        pairs = [(_event(), _event()) for _ in range(marks)]
        run(pairs)
        torch.cuda.synchronize()
        ms.extend(a.elapsed_time(b) for a, b in pairs[skip:])
    return Timing.of(ms)


def open_device():
    """device 0, the library loaded and on torch's stream -> the library; no GPU is an error"""
    assert torch.cuda.is_available(), "needs the GPU"
    from nntoolkitcore_amd import capi, layers
    torch.cuda.set_device(0); lib = capi.load(); layers.use_torch_stream()
    return lib


def ragged(rng, n, B):
    """B int32 lengths uniform in [n // 2, n], the first one n: one draw from rng"""
    x = rng.integers(n // 2, n + 1, B).astype(np.int32)
    x[0] = n
    return x


def emit(out, profile=None):
    """print `out` as one JSON line; with `profile` also write that line to profiles/<profile>.json"""
    line = json.dumps(out)
    if profile:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", profile + ".json"), "w") as fh:
            fh.write(line + "\n")
    print(line)


def ab_children(script, child_flag, this_lib, parent_lib, repeats, rounds=2, timeout=300):
    """`python script child_flag LIB repeats` once per measurement, each in a fresh process, this / parent alternating
    -> {"this": [...], "parent": [...]}: per round the JSON of the child's last stdout line.  A child that fails or overruns raises."""
    runs = {"this": [], "parent": []}
    for _ in range(rounds):
        for key, lib in (("this", this_lib), ("parent", parent_lib)):
            res = subprocess.run([sys.executable, os.path.abspath(script), child_flag, lib, str(repeats)], stdout=subprocess.PIPE,
                                 text=True, timeout=timeout, check=True)
            runs[key].append(json.loads(res.stdout.strip().splitlines()[-1]))
    return runs


def ab_figures(this_ms, parent_ms):
    """the per-round medians of the two libraries -> the fields a tool reports: spread = |m0 - m1| / mean, ratio = mean / mean"""
    mean_this, mean_parent = float(np.mean(this_ms)), float(np.mean(parent_ms))
    return {"this_ms": list(this_ms), "parent_ms": list(parent_ms),
            "this_spread": (max(this_ms) - min(this_ms)) / mean_this, "parent_spread": (max(parent_ms) - min(parent_ms)) / mean_parent,
            "this_over_parent": mean_this / mean_parent}
