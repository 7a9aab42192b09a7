"""bench.py's two kinds of run: a plain run measures only the headline steps; --full adds the extras and the CPU baseline.

CPU tier: --full is an option of its own.
GPU tier: bench.py itself at a small size, plain and --full; the plain line carries none of the extras, the --full line does."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--steps", "2", "--warmup", "1", "--contigs", "60", "--recs", "150"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline", "phase_ms", "graph", "setup", "library")
FULL_ONLY = ("step_with_fetch_ms", "k10000", "c3_heavy_tail", "c3_dup3", "c3_shuffled", "e2e", "weak", "cpu_baseline")


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_bench_knows_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--steps must be" in r.stderr and "unrecognized" not in r.stderr


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_full_adds_the_extras():
    plain = _bench(SMALL)
    assert all(k in plain for k in HEADLINE)
    assert plain["metric"] == "contigs_per_sec" and plain["steps"] == 2 and plain["value"] > 0
    assert not [k for k in FULL_ONLY if k in plain]
    full = _bench(SMALL + ["--full", "--cpu-sample", "60"])
    assert all(k in full for k in HEADLINE)
    assert full["graph"] == plain["graph"]                     # the same seeded batch, the same timed path
    assert full["step_with_fetch_ms"] > 0 and full["k10000"]["max_paths"] == 10000 and full["k10000"]["contigs"] == 60
    assert full["cpu_baseline"]["kind"] == "port" and full["cpu_baseline"]["value"] > 0
