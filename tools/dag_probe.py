"""aasm_sssp_dag, its list walk taken 64 edges at a time, beside the comparison build that takes one edge per step, on two inputs:
the C3 generator's contig DAGs (as tools/ksw_probe.py extracts them, source V - 2) and a batch of wide random DAGs with hubs whose
out-degree is in the thousands.  One JSON line per input:
  dag_ms           minimum over --reps of the whole entry, wall clock (host checks, uploads, one launch, downloads), order included
  topo_ms          the same for aasm_topology_sort alone
  dag_edgewise_ms  aasm_sssp_dag from the comparison build, libalignasm_amd_dag_edgewise.so (make -C alignasm_amd/csrc
                   ../libalignasm_amd_dag_edgewise.so: -DAASM_DAG_EDGEWISE, one edge per step; --edgewise names a copy elsewhere, such
                   as one under variants/), run in a child process; its d5, prev, order and status must equal the shipped form's
                   bit for bit
  same_keys        (contig DAGs) the distances agree with aasm_sssp_bellman_ford's in every key of the order
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

ap = argparse.ArgumentParser()
ap.add_argument("--contigs", type=int, default=1000)
ap.add_argument("--recs", type=int, default=1000)
ap.add_argument("--seed", type=int, default=21)
ap.add_argument("--random", type=int, default=128, help="wide random DAGs in the second input")
ap.add_argument("--n", type=int, default=6000, help="... of this many vertices")
ap.add_argument("--hubs", type=int, default=4, help="... with this many hubs each")
ap.add_argument("--hub-degree", type=int, default=3000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--edgewise", default=os.path.join(ROOT, "alignasm_amd", "libalignasm_amd_dag_edgewise.so"))
ap.add_argument("--child", default="", help="(internal) write this build's results and times to the given .npz")
a = ap.parse_args()


def wide_dag(rng, n, hubs, hub_degree):
    """Vertices in a random topological order; two edges out of every vertex, and `hubs` vertices among the first with hub_degree
    edges each, heads repeating; lists shuffled."""
    rank = rng.permutation(n)
    order = np.argsort(rank)
    tails = [np.repeat(order[:n - 1], 2)] + [np.full(hub_degree, order[i]) for i in range(hubs)]
    tails = np.concatenate(tails)
    lo = rank[tails] + 1
    heads = order[(lo + (rng.random(len(tails)) * (n - lo)).astype(np.int64)).clip(max=n - 1)]
    perm = rng.permutation(len(tails))
    tails, heads = tails[perm], heads[perm]
    by_tail = np.argsort(tails, kind="stable")
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(tails, minlength=n))
    E = len(tails)
    w = np.stack([rng.integers(-50, 200, E), rng.integers(0, 100, E), rng.integers(0, 3, E), rng.integers(0, 2, E), rng.integers(0, 2, E)], 1)
    return KC.graph(n, rowptr, heads[by_tail], w, int(order[0]), int(order[-1]))


def inputs():
    paf = A.Paf.synth(a.contigs, a.recs, a.seed, no_cs=True)
    hb = paf.batch(); paf.close()
    db = A.DeviceBatch(hb)
    res = db.solve(max_paths=4, keep_debug=True)
    batch, _, _ = KC.pipeline_batch(res, hb, 4)
    res.close(); db.close()
    yield "c3_contig_dags", batch
    rng = np.random.default_rng(a.seed)
    yield "wide_random_dags", KC.make_batch([wide_dag(rng, a.n, a.hubs, a.hub_degree) for _ in range(a.random)])


def timed(fn, *args, **kw):
    out, wall = None, []
    for r in range(a.reps + 1):
        t = time.perf_counter()
        out = fn(*args, **kw)
        if r:
            wall.append((time.perf_counter() - t) * 1e3)
    return out, round(min(wall), 2)


def keys(d):
    tot = np.where(d[:, 4] == 0, 1, d[:, 4])
    return d[:, 0] + d[:, 1], d[:, 2], d[:, 3], tot


if a.child:
    out = {}
    for name, b in inputs():
        (d, prev, status, order), ms = timed(api.sssp_dag, b["g_voff"], b["rowptr"], b["col"], b["w"], b["src"], order=True)
        out.update({f"{name}_d": d, f"{name}_prev": prev, f"{name}_status": status, f"{name}_order": order, f"{name}_ms": np.array(ms)})
    np.savez(a.child, **out)
    sys.exit(0)

edge = None
if os.path.exists(a.edgewise):
    with tempfile.TemporaryDirectory() as tmpdir:
        tmp = os.path.join(tmpdir, "dag_probe_edgewise.npz")
        argv = [sys.executable, os.path.abspath(__file__), "--child", tmp] + [f"--{k.replace('_', '-')}={getattr(a, k)}" for k in
                                                                              ("contigs", "recs", "seed", "random", "n", "hubs", "hub_degree", "reps")]
        subprocess.run(argv, env=dict(os.environ, AASM_LIB_OVERRIDE=a.edgewise), check=True, timeout=900)      # a fresh process: one library per process
        with np.load(tmp) as z:
            edge = {k: z[k] for k in z.files}
for name, b in inputs():
    args = (b["g_voff"], b["rowptr"], b["col"], b["w"], b["src"])
    (d, prev, status, order), dag_ms = timed(api.sssp_dag, *args, order=True)
    (order2, status2), topo_ms = timed(api.topology_sort, *args[:3])
    row = {"input": name, "graphs": len(b["src"]), "V": int(b["g_voff"][-1]), "E": int(b["rowptr"][-1]), "max_degree": int(np.diff(b["rowptr"]).max()),
           "dag_ms": dag_ms, "topo_ms": topo_ms, "acyclic": bool(not status.any()), "sort_same": bool(np.array_equal(order, order2) and np.array_equal(status, status2))}
    if name == "c3_contig_dags":
        bd, _, bst, _ = api.sssp_bellman_ford(*args)
        (s0, a0, n0, t0), (s1, a1, n1, t1) = keys(bd), keys(d)
        row["same_keys"] = bool(not bst.any() and np.array_equal(s0, s1) and np.array_equal(a0, a1) and np.array_equal(n0 * t1, n1 * t0))
    if edge is not None:
        row["dag_edgewise_ms"] = float(edge[f"{name}_ms"])
        row["edgewise_same_bits"] = bool(all(np.array_equal(edge[f"{name}_{k}"], v) for k, v in (("d", d), ("prev", prev), ("status", status), ("order", order))))
    print(json.dumps(row), flush=True)
