"""tools/timing.py on the host: the A/B arithmetic and its child processes, the ragged lengths, the JSON line, the result type's views,
and that the timing loop lives nowhere else under tools/."""
import glob, json, os, py_compile, subprocess, sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)
import timing

# tools outside the timing module's scope that keep an event pair of their own: the diagnostics-build probes (the overlap probes time
# several streams at once), and the two stamp dumps whose single pair only brackets the stamped launch
OWN_EVENTS = {"conv_probe.py", "gemm_probe.py", "rec_probe.py", "spec_probe.py", "overlap_probe.py", "overlap_probe_gru.py",
              "overlap_probe_2gru.py", "fk_stamps.py", "rr_stamps.py"}


@pytest.mark.parametrize("this, parent", [((2.0, 2.0), (2.0, 2.0)),            # equal libraries
                                          ((3.0, 3.0), (2.0, 2.0)),            # a known ratio
                                          ((1.9, 2.1), (4.0, 4.4))])           # known spreads
def test_ab_figures(this, parent):
    got = timing.ab_figures(list(this), list(parent))
    mean_t, mean_p = (this[0] + this[1]) / 2, (parent[0] + parent[1]) / 2
    assert set(got) == {"this_ms", "parent_ms", "this_spread", "parent_spread", "this_over_parent"}
    assert got["this_ms"] == list(this) and got["parent_ms"] == list(parent)
    assert got["this_spread"] == pytest.approx(abs(this[0] - this[1]) / mean_t, rel=1e-15, abs=0)
    assert got["parent_spread"] == pytest.approx(abs(parent[0] - parent[1]) / mean_p, rel=1e-15, abs=0)
    assert got["this_over_parent"] == pytest.approx(mean_t / mean_p, rel=1e-15)
    json.dumps(got)


def test_ab_figures_fixed_values():
    assert timing.ab_figures([2.0, 2.0], [2.0, 2.0]) == {"this_ms": [2.0, 2.0], "parent_ms": [2.0, 2.0], "this_spread": 0.0,
                                                         "parent_spread": 0.0, "this_over_parent": 1.0}
    got = timing.ab_figures([3.0, 5.0], [1.0, 1.0])
    assert got["this_spread"] == 0.5 and got["parent_spread"] == 0.0 and got["this_over_parent"] == 4.0


STUB = """import json, os, sys, time
flag, lib, repeats = sys.argv[1:4]
log = os.path.join(os.path.dirname(os.path.abspath(__file__)), "calls")
with open(log, "a") as fh:
    fh.write(lib + "\\n")
if lib == "fails":
    sys.exit(3)
if lib == "hangs":
    time.sleep(60)
print("some noise first")
print(json.dumps({"flag": flag, "lib": lib, "repeats": int(repeats), "pid": os.getpid(), "count": len(open(log).readlines())}))
"""


@pytest.fixture
def stub(tmp_path):
    path = tmp_path / "stub_child.py"
    path.write_text(STUB)
    return str(path)


def test_ab_children_order_processes_and_parsing(stub):
    assert "torch" not in STUB and "nntoolkitcore" not in STUB
    runs = timing.ab_children(stub, "--child", "THIS", "PARENT", 3)
    assert list(runs) == ["this", "parent"] and [len(v) for v in runs.values()] == [2, 2]
    assert all(r == {"flag": "--child", "lib": lib, "repeats": 3, "pid": r["pid"], "count": r["count"]}
               for key, lib in (("this", "THIS"), ("parent", "PARENT")) for r in runs[key])
    assert [r["count"] for r in runs["this"]] == [1, 3] and [r["count"] for r in runs["parent"]] == [2, 4]       # this, parent, this, parent
    pids = [r["pid"] for v in runs.values() for r in v]
    assert len(set(pids)) == 4 and os.getpid() not in pids
    assert len(timing.ab_children(stub, "--child", "A", "B", 1, rounds=3)["parent"]) == 3


def test_ab_children_failure_and_timeout_raise(stub):
    with pytest.raises(subprocess.CalledProcessError):
        timing.ab_children(stub, "--child", "THIS", "fails", 1)
    with pytest.raises(subprocess.TimeoutExpired):
        timing.ab_children(stub, "--child", "hangs", "PARENT", 1, timeout=0.5)


@pytest.mark.parametrize("seed", [0, 7])
@pytest.mark.parametrize("n, B", [(1000, 512), (41, 3)])
def test_ragged_is_the_old_idiom(seed, n, B):
    old_rng, new_rng = np.random.default_rng(seed), np.random.default_rng(seed)
    old = old_rng.integers(n // 2, n + 1, B).astype(np.int32); old[0] = n
    new = timing.ragged(new_rng, n, B)
    assert new.dtype == np.int32 and new.shape == (B,) and np.array_equal(new, old)
    assert new[0] == n and new.min() >= n // 2 and new.max() <= n
    assert np.array_equal(new_rng.integers(0, 2 ** 31, 8), old_rng.integers(0, 2 ** 31, 8))       # exactly one draw taken


def test_emit(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(timing, "ROOT", str(tmp_path))
    out = {"tool": "x", "ms": [1.5, 2.0], "nested": {"ok": True}}
    timing.emit(out)
    assert capsys.readouterr().out == json.dumps(out) + "\n" and os.listdir(tmp_path) == []
    timing.emit(out, "x_time")
    printed = capsys.readouterr().out
    assert os.listdir(tmp_path) == ["profiles"] and os.listdir(tmp_path / "profiles") == ["x_time.json"]
    assert (tmp_path / "profiles" / "x_time.json").read_text() == printed == json.dumps(out) + "\n"


@pytest.mark.parametrize("ms, median", [([3.0, 1.0, 2.0], 2.0), ([4.0, 1.0, 2.0, 3.0], 2.5)])
def test_timing_views(ms, median):
    t = timing.Timing.of(ms)
    assert all(type(v) is float for v in t)
    assert tuple(t) == (median, 1.0, max(ms)) and t[0] == median and t[1:] == (1.0, max(ms))
    assert t.dict == {"median": median, "min": 1.0, "max": max(ms)} and list(t.dict) == ["median", "min", "max"]
    assert t.pair == (median, [1.0, max(ms)])
    assert json.dumps(t) == json.dumps([median, 1.0, max(ms)]) and json.dumps(t[1:]) == json.dumps([1.0, max(ms)])


def test_tools_compile_and_time_in_one_place(tmp_path):
    files = sorted(glob.glob(os.path.join(TOOLS, "*.py")))
    assert os.path.join(TOOLS, "timing.py") in files
    for f in files:
        py_compile.compile(f, cfile=str(tmp_path / (os.path.basename(f) + "c")), doraise=True)
    holders = {os.path.basename(f) for f in files if any(s in open(f).read() for s in ("def timed", "Event(enable_timing=True)"))}
    assert holders == OWN_EVENTS | {"timing.py"}
