"""aasm_k_shortest_walks on the C3 generator's contig DAGs, beside the pipeline's own K6-K8 phases on the same contigs and the
CPU oracle.  One JSON line per (contigs, K):
  ksw_ms       minimum over --reps of the whole entry, wall clock (host checks, uploads, the five kernels, downloads; walks=False)
  ksw_cyc_ms   with --cycles: the same with cycles=True (the tree of dijkstra() from the sink, the solver's is_dag = false), from the
               same run; n_found and the distances' first keys (score sum, anom) must equal the default mode's
  pipe_ms      minimum over --reps of the pipeline's sptree + heap_prep + heap + enum phases (HIP events, timing=True)
  oracle_ms    the CPU oracle (oracle_generic_kwalks, one thread) on --oracle-sample graphs, scaled to all of them
With --negative the contigs are overhang contigs (tests/overhang_cases.py, mode --overhang: records run to or past the query's end,
so dest edges and walk sums are negative) and every aasm_k_shortest_walks call passes negative=True (AASM_KSW_NEGATIVE; with
--cycles the tree is then bellman_ford()'s).
The first call of each configuration is a warm-up and is not counted.  Checks n_found / heap_nodes against the pipeline."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import alignasm_amd as A  # noqa: E402
from alignasm_amd import api  # noqa: E402
import aasm_testlib as T  # noqa: E402
import ksw_cases as KC  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--contigs", default="1000,5000")
ap.add_argument("--k", default="4,10000")
ap.add_argument("--recs", type=int, default=1000)
ap.add_argument("--seed", type=int, default=21)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--oracle-sample", type=int, default=40)
ap.add_argument("--cycles", action="store_true", help="time cycles=True beside the default mode")
ap.add_argument("--negative", action="store_true", help="overhang contigs, negative=True")
ap.add_argument("--overhang", default="longest", help="tests/overhang_cases.py's mode for --negative")
a = ap.parse_args()

for nc in (int(x) for x in a.contigs.split(",")):
    paf = A.Paf.synth(nc, a.recs, a.seed, no_cs=True)
    hb = paf.batch(); paf.close()
    if a.negative:
        import overhang_cases as OC
        hb = OC.overhang(hb, a.overhang, a.seed)
    db = A.DeviceBatch(hb)
    for K in (int(x) for x in a.k.split(",")):
        res = db.solve(max_paths=K, keep_debug=True)
        batch, contigs, want = KC.pipeline_batch(res, hb, K)
        res.close()
        pipe = []
        for r in range(a.reps + 1):
            res = db.solve(max_paths=K, timing=True)
            ph = res.stats()["phase_ms"]
            res.close()
            if r:
                pipe.append(sum(ph.get(p, 0.0) for p in ("sptree", "heap_prep", "heap", "enum")))
        args = (batch["g_voff"], batch["rowptr"], batch["col"], batch["w"], batch["src"], batch["sink"], K)
        wall = []
        for r in range(a.reps + 1):
            t = time.perf_counter()
            got = api.k_shortest_walks(*args, walks=False, tree=False, negative=a.negative)
            if r:
                wall.append((time.perf_counter() - t) * 1e3)
        ok = bool(np.array_equal(got["n_found"], want["kfound"]) and np.array_equal(got["heap_nodes"], want["h_cnt"]))
        cyc = {}
        if a.cycles:
            wall_c = []
            for r in range(a.reps + 1):
                t = time.perf_counter()
                got_c = api.k_shortest_walks(*args, walks=False, tree=False, cycles=True, negative=a.negative)
                if r:
                    wall_c.append((time.perf_counter() - t) * 1e3)
            same = bool(np.array_equal(got_c["n_found"], got["n_found"]) and not got_c["status"].any() and
                        np.array_equal(got_c["dist"][:, :, :2].sum(2), got["dist"][:, :, :2].sum(2)) and
                        np.array_equal(got_c["dist"][:, :, 2], got["dist"][:, :, 2]))
            cyc = {"ksw_cyc_ms": round(min(wall_c), 2), "cycles_same_keys": same}
        rng = np.random.default_rng(1)
        pick = rng.choice(len(contigs), min(a.oracle_sample, len(contigs)), replace=False)
        t = time.perf_counter()
        for i in pick:
            v0, v1 = int(batch["g_voff"][i]), int(batch["g_voff"][i + 1])
            rp = batch["rowptr"][v0:v1 + 1]
            g = KC.graph(v1 - v0, rp - rp[0], batch["col"][rp[0]:rp[-1]], batch["w"][rp[0]:rp[-1]], v1 - v0 - 2, v1 - v0 - 1)
            T.generic_run(T.oracle(), "oracle_", g["n"], g["rowptr"], g["col"], np.ascontiguousarray(g["w"].reshape(-1)), g["src"], g["sink"], K,
                          with_paths=False)
        oracle_ms = (time.perf_counter() - t) * 1e3 * len(contigs) / max(1, len(pick))
        print(json.dumps({"contigs": nc, "graphs": len(contigs), "K": K, "V": int(batch["g_voff"][-1]), "E": int(batch["rowptr"][-1]),
                          "negative_edges": int((batch["w"][:, 0] + batch["w"][:, 1] < 0).sum()),
                          "ksw_ms": round(min(wall), 2), **cyc, "pipe_ms": round(min(pipe), 3), "oracle_ms": round(oracle_ms, 1),
                          "walks": int(got["n_found"].sum()), "heap_nodes": int(got["heap_nodes"].sum()), "equal_to_pipeline": ok}), flush=True)
    db.close()
