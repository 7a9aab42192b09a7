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
With --resident the same graphs are put into a GraphBatch once (not timed; sources and sinks as device tensors) and solved there:
  res_solve_ms / res_export_ms   GraphBatch.ksw_solve (returns when the sizes are final) and ksw_export + a device synchronize, wall
                                 clock, each the part of the run with the smallest sum res_ms; res_equal: n_found, heap_nodes, status
                                 and the packed distances equal the host entry's of this run
  work_mb                        device memory the first resident solve took (free memory before - after): the handle's working memory
  ksw_runs_ms   (always printed) the host entry's --reps runs one by one: their spread is the margin res_ms is held against
With --walks-row a row with walks=True (host entry and resident) is added for the first contig count at the first K.
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
ap.add_argument("--resident", action="store_true", help="time GraphBatch.ksw_solve / ksw_export on the same graphs")
ap.add_argument("--walks-row", action="store_true", help="one more row with walks=True")
a = ap.parse_args()


def resident(batch, K, walks, got):
    """GraphBatch solve + export on a batch the host entry has just solved as `got` -> the row's res_* figures."""
    import torch
    dev = torch.device("cuda", 0)
    free0 = torch.cuda.mem_get_info(dev)[0]
    gb = api.GraphBatch.upload(batch["g_voff"], batch["rowptr"], batch["col"], w5=batch["w"])
    src, sink = torch.from_numpy(batch["src"]).to(dev), torch.from_numpy(batch["sink"]).to(dev)
    torch.cuda.synchronize(dev)
    free1 = torch.cuda.mem_get_info(dev)[0]
    runs, work = [], 0
    for r in range(a.reps + 1):
        t0 = time.perf_counter()
        sz = gb.ksw_solve(src, sink, K, walks=walks, negative=a.negative)
        t1 = time.perf_counter()
        if r == 0:
            work = free1 - torch.cuda.mem_get_info(dev)[0]
        out = gb.ksw_export(sz)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        if r:
            runs.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
        if r < a.reps:
            del out
    o = api.torch_to_numpy(out)
    nf = got["n_found"]
    same = bool(np.array_equal(o["n_found"], nf) and np.array_equal(o["heap_nodes"], got["heap_nodes"]) and np.array_equal(o["status"], got["status"]) and
                all(np.array_equal(o["dist5"][o["found_off"][g]:o["found_off"][g + 1]], got["dist"][g, :nf[g]]) for g in range(len(nf))))
    if walks:
        k_ = got["dist"].shape[1]
        same = same and bool(np.array_equal(o["walk_edges"], got["walk_edges"]) and
                             all(np.array_equal(o["walk_off"][o["found_off"][g]:o["found_off"][g + 1]], got["walk_off"][g * k_:g * k_ + nf[g]]) for g in range(len(nf))))
    gb.close()
    best = min(runs)
    return {"res_ms": round(best[0], 2), "res_solve_ms": round(best[1], 2), "res_export_ms": round(best[2], 2), "res_equal": same,
            "work_mb": round(work / 2**20, 1), "upload_mb": round((free0 - free1) / 2**20, 1)}


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
        res = dict(resident(batch, K, False, got) if a.resident else {}, ksw_runs_ms=[round(x, 2) for x in wall])
        if a.walks_row:
            a.walks_row = False
            ww = []
            for r in range(a.reps + 1):
                t = time.perf_counter()
                got_w = api.k_shortest_walks(*args, walks=True, tree=False, negative=a.negative)
                if r:
                    ww.append((time.perf_counter() - t) * 1e3)
            print(json.dumps({"contigs": nc, "K": K, "walks": True, "walk_edges": int(got_w["walk_off"][-1]), "ksw_ms": round(min(ww), 2),
                              "ksw_runs_ms": [round(x, 2) for x in ww], **(resident(batch, K, True, got_w) if a.resident else {})}), flush=True)
            del got_w
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
                          "ksw_ms": round(min(wall), 2), **cyc, **res, "pipe_ms": round(min(pipe), 3), "oracle_ms": round(oracle_ms, 1),
                          "walks": int(got["n_found"].sum()), "heap_nodes": int(got["heap_nodes"].sum()), "equal_to_pipeline": ok}), flush=True)
    db.close()
