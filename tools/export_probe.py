"""Times of the device-side export against the host fetch, one JSON line per config.

    python tools/export_probe.py [--config c3_k4|c3_k10000|c5_share|all] [--reps N]

solve_ms: wall time of DeviceBatch.solve (ends in a stream synchronize); sizes_ms: wall time of aasm_result_sizes (ends in its
read-back); export_ms: HIP events around aasm_result_export on the torch stream, into buffers allocated once; fetch_ms: wall time of
aasm_result_fetch (the host pack, into malloc'ed arrays); to_torch_ms: wall time of a fresh solve's DeviceResult.to_torch() up to
a stream synchronize (torch.empty of the eight arrays + sizes + export: what a torch caller pays per batch).  Minima over --reps
runs after one warm-up of each.  The exported arrays are compared with the fetched ones once per config.  Needs an MI355X: no
device, no numbers.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {
    "c3_k4": dict(n=5000, recs=1000, seed=21, K=4, dense=False),
    "c3_k10000": dict(n=5000, recs=1000, seed=21, K=10000, dense=False),
    "c5_share": dict(n=1250, recs=1000, seed=31, K=16, dense=True),   # the per-GPU share of C5 on 8 GPUs
}


def probe(name, reps):
    import torch
    import alignasm_amd as A
    from alignasm_amd._abi import DevOut, OutSizes
    cfg = CONFIGS[name]
    paf = A.Paf.synth(cfg["n"], cfg["recs"], cfg["seed"], dense=cfg["dense"], no_cs=True)
    db = A.DeviceBatch(paf)
    stream = torch.cuda.current_stream(0)
    t_solve, t_sizes, t_export, t_fetch, t_torch = [], [], [], [], []
    bufs = None
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        res = db.solve(max_paths=cfg["K"])
        t1 = time.perf_counter()
        sz = res.sizes()
        t2 = time.perf_counter()
        if bufs is None:                                             # (every solve of the batch has the same sizes)
            d = res.to_torch()
            stream.synchronize()
            got = A.torch_to_numpy(d)
            want = res.fetch()
            for k in ("main_off", "alt_off", "all_path_off", "all_elem_off", "main", "alt", "all", "status"):
                assert got[k].tobytes() == want[k].tobytes(), (name, k)
            bufs = d
        ptr = lambda t: t.data_ptr() if t.numel() else None   # noqa: E731
        dst = DevOut(ptr(bufs["main_off"]), ptr(bufs["alt_off"]), ptr(bufs["all_path_off"]), ptr(bufs["all_elem_off"]),
                     ptr(bufs["main"]), ptr(bufs["alt"]), ptr(bufs["all"]), ptr(bufs["status"]))
        ev0.record(stream)
        assert res.export_raw(OutSizes(*(sz[n] for n, _ in OutSizes._fields_)), dst, stream.cuda_stream) == 0
        ev1.record(stream)
        ev1.synchronize()
        t3 = time.perf_counter()
        raw = res.fetch_raw()
        t4 = time.perf_counter()
        A.api.free_out(raw)
        res.close()
        res = db.solve(max_paths=cfg["K"])
        t5 = time.perf_counter()
        d = res.to_torch()
        stream.synchronize()
        t6 = time.perf_counter()
        del d
        res.close()
        if rep > 0:
            t_solve.append((t1 - t0) * 1e3); t_sizes.append((t2 - t1) * 1e3)
            t_export.append(ev0.elapsed_time(ev1)); t_fetch.append((t4 - t3) * 1e3); t_torch.append((t6 - t5) * 1e3)
    out = {"config": name, "contigs": cfg["n"], "K": cfg["K"], "reps": reps, **sz,
           "solve_ms": round(min(t_solve), 3), "sizes_ms": round(min(t_sizes), 3), "export_ms": round(min(t_export), 3),
           "fetch_ms": round(min(t_fetch), 3), "to_torch_ms": round(min(t_torch), 3),
           "export_bytes": 40 * (sz["n_main"] + sz["n_alt"] + sz["n_all_elems"]) + 8 * (3 * (sz["n_contigs"] + 1) + sz["n_all_paths"] + 1) + 4 * sz["n_contigs"]}
    db.close(); paf.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="all", choices=["all"] + list(CONFIGS))
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    for name in (CONFIGS if a.config == "all" else [a.config]):
        print(json.dumps(probe(name, a.reps)), flush=True)


if __name__ == "__main__":
    main()
