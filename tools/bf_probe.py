"""aasm_sssp_bellman_ford beside aasm_sssp_dijkstra on the same non-negative graphs: the C3 generator's contig DAGs (as
tools/ksw_probe.py extracts them, source V - 2) and a batch of random cyclic graphs.  One JSON line per input:
  dijkstra_ms      minimum over --reps of the whole entry, wall clock (host checks, uploads, the kernel, downloads)
  bf_ms            the same for aasm_sssp_bellman_ford, its list walk taken 64 edges at a time (the shipped form)
  bf_edgewise_ms   the same from the comparison build, libalignasm_amd_bf_edgewise.so (make -C alignasm_amd/csrc
                   ../libalignasm_amd_bf_edgewise.so: -DAASM_BF_EDGEWISE, one edge per step), run in a child process; its d5, prev and
                   status must equal the shipped form's bit for bit
  same_keys        the two algorithms' distances agree in every key of the order (score sum, anom, mapq ratio); among equal
                   distances the two may keep different representatives, as their relaxation orders differ
The first call of each configuration is a warm-up and is not counted."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import alignasm_amd as A  # noqa: E402
from alignasm_amd import api  # noqa: E402
import ksw_cases as KC  # noqa: E402
import ksw_cyclic_cases as CC  # noqa: E402

EDGEWISE = os.path.join(ROOT, "alignasm_amd", "libalignasm_amd_bf_edgewise.so")

ap = argparse.ArgumentParser()
ap.add_argument("--contigs", type=int, default=1000)
ap.add_argument("--recs", type=int, default=1000)
ap.add_argument("--seed", type=int, default=21)
ap.add_argument("--random", type=int, default=4000, help="random cyclic graphs in the second input")
ap.add_argument("--nmax", type=int, default=200, help="... of up to this many vertices")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--child", default="", help="(internal) write this build's bellman_ford results and times to the given .npz")
a = ap.parse_args()


def inputs():
    paf = A.Paf.synth(a.contigs, a.recs, a.seed, no_cs=True)
    hb = paf.batch(); paf.close()
    db = A.DeviceBatch(hb)
    res = db.solve(max_paths=4, keep_debug=True)
    batch, _, _ = KC.pipeline_batch(res, hb, 4)
    res.close(); db.close()
    yield "c3_contig_dags", batch
    gs = CC.random_graphs(a.seed, a.random, kinds=("scalar", "mixed"), nmax=a.nmax)
    yield "random_cyclic", KC.make_batch(gs)


def timed(fn, *args):
    out, wall = None, []
    for r in range(a.reps + 1):
        t = time.perf_counter()
        out = fn(*args)
        if r:
            wall.append((time.perf_counter() - t) * 1e3)
    return out, round(min(wall), 2)


def keys(d):
    tot = np.where(d[:, 4] == 0, 1, d[:, 4])
    return d[:, 0] + d[:, 1], d[:, 2], d[:, 3], tot


if a.child:
    out = {}
    for name, b in inputs():
        (d, prev, status, _), ms = timed(api.sssp_bellman_ford, b["g_voff"], b["rowptr"], b["col"], b["w"], b["src"])
        out.update({f"{name}_d": d, f"{name}_prev": prev, f"{name}_status": status, f"{name}_ms": np.array(ms)})
    np.savez(a.child, **out)
    sys.exit(0)

edge = None
if os.path.exists(EDGEWISE):
    with tempfile.TemporaryDirectory() as tmpdir:
        tmp = os.path.join(tmpdir, "bf_probe_edgewise.npz")
        argv = [sys.executable, os.path.abspath(__file__), "--child", tmp] + [f"--{k}={getattr(a, k)}" for k in ("contigs", "recs", "seed", "random", "nmax", "reps")]
        subprocess.run(argv, env=dict(os.environ, AASM_LIB_OVERRIDE=EDGEWISE), check=True, timeout=900)      # a fresh process: one library per process
        with np.load(tmp) as z:
            edge = {k: z[k] for k in z.files}
for name, b in inputs():
    args = (b["g_voff"], b["rowptr"], b["col"], b["w"], b["src"])
    (dd, _), dj_ms = timed(api.sssp_dijkstra, *args)
    (d, prev, status, _), bf_ms = timed(api.sssp_bellman_ford, *args)
    (s0, a0, n0, t0), (s1, a1, n1, t1) = keys(dd), keys(d)
    same = bool(not status.any() and np.array_equal(s0, s1) and np.array_equal(a0, a1) and np.array_equal(n0 * t1, n1 * t0))
    row = {"input": name, "graphs": len(b["src"]), "V": int(b["g_voff"][-1]), "E": int(b["rowptr"][-1]),
           "max_degree": int(np.diff(b["rowptr"]).max()), "dijkstra_ms": dj_ms, "bf_ms": bf_ms, "same_keys": same}
    if edge is not None:
        row["bf_edgewise_ms"] = float(edge[f"{name}_ms"])
        row["edgewise_same_bits"] = bool(np.array_equal(edge[f"{name}_d"], d) and np.array_equal(edge[f"{name}_prev"], prev) and
                                         np.array_equal(edge[f"{name}_status"], status))
    print(json.dumps(row), flush=True)
