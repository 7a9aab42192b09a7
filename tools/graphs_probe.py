"""Resident graph batches beside the host-pointer entries on the C3 generator's contig DAGs (as tools/dag_probe.py extracts them), with
--sources source vectors per graph: the question is what a caller pays who asks many sources on the same graphs.  One JSON line per
entry (dag, bellman_ford, topology_sort, dial, and dijkstra where no edge has a negative score sum):
  host_ms       the host entry called --sources times, wall clock (each call: host checks, uploads, one launch, downloads, repacking)
  upload_ms     GraphBatch.upload once, wall clock (host checks, the arrays' upload)
  resident_ms   --sources resident calls on that batch and one wait at their end, wall clock; the sources are uploaded before the clock
                starts, the results stay on the device
  call_event_ms one resident call between two HIP events on its stream (minimum over the sources): the source check with its one-word
                read-back, the solve kernel, the kernels behind it - no upload and no download
  same          every resident result equals the host entry's for the same sources
Times are minima over --reps; the first round of each configuration is a warm-up and is not counted."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import alignasm_amd as A  # noqa: E402
from alignasm_amd import api  # noqa: E402
import graphs_resident_cases as GR  # noqa: E402
import ksw_cases as KC  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--contigs", type=int, default=1000)
ap.add_argument("--recs", type=int, default=1000)
ap.add_argument("--seed", type=int, default=21)
ap.add_argument("--sources", type=int, default=8)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()

paf = A.Paf.synth(a.contigs, a.recs, a.seed, no_cs=True)
hb = paf.batch(); paf.close()
db = A.DeviceBatch(hb)
res = db.solve(max_paths=4, keep_debug=True)
b, _, _ = KC.pipeline_batch(res, hb, 4)
res.close(); db.close()
b = GR.with_cost(b)
sizes = np.diff(b["g_voff"])
rng = np.random.default_rng(a.seed)
srcs = [b["src"]] + [(rng.integers(0, 1 << 30, len(sizes)) % sizes).astype(np.int32) for _ in range(a.sources - 1)]
dev_srcs = [torch.from_numpy(s).to("cuda:0") for s in srcs]
call = GR.api_call(api)
entries = ["dag", "bellman_ford", "topology_sort", "dial"] + (["dijkstra"] if not (b["w"][:, 0] + b["w"][:, 1] < 0).any() else [])


def best(fn):
    out, wall = None, []
    for r in range(a.reps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        if r:
            wall.append((time.perf_counter() - t) * 1e3)
    return out, round(min(wall), 2)


def resident(gb, entry):
    run = getattr(gb, entry)
    out = [run() if entry == "topology_sort" else run(s, **({"order": True} if entry == "dag" else {})) for s in dev_srcs]
    torch.cuda.synchronize()
    return out


def event_ms(gb, entry):
    run, ms = getattr(gb, entry), []
    for s in dev_srcs:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run() if entry == "topology_sort" else run(s)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(min(ms), 3)


for entry in entries:
    host, host_ms = best(lambda: [GR.host_results(call, dict(b, src=s), entry) for s in srcs])
    gb, upload_ms = best(lambda: api.GraphBatch.upload(b["g_voff"], b["rowptr"], b["col"], w5=b["w"], cost=b["cost"], lim=b["lim"]))
    got, resident_ms = best(lambda: resident(gb, entry))
    row = {"entry": entry, "graphs": len(sizes), "V": int(b["g_voff"][-1]), "E": int(b["rowptr"][-1]), "sources": a.sources, "host_ms": host_ms,
           "upload_ms": upload_ms, "resident_ms": resident_ms, "call_event_ms": event_ms(gb, entry),
           "same": bool(all(GR.same(api.torch_to_numpy(g), h) == [] for g, h in zip(got, host)))}
    gb.close()
    print(json.dumps(row), flush=True)
