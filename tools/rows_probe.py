"""Times of the device rows on the C3 file (5 000 contigs x 1 000 records, seed 21), one JSON line per K.

    python tools/rows_probe.py [--k 4] [--contigs 5000] [--dir DIR] [--reps 3]

sizes_ms: wall time of aasm_rows_sizes_device (length pass, three scans, one read-back; the call waits);
fill_ms / fill_GBps: HIP events around aasm_rows_format_device of the whole main list on the torch stream, into a buffer allocated
once, minimum of `reps` after a warm-up, and the bytes written per second; rows / bytes: the three lists' rows and text bytes.
host_write_s / device_write_s: wall times of Paf.write_outputs (aasm_writer_append, the walking writer on the host threads) and of
Paf.write_outputs_device (aasm_writer_append_device: format in pieces, copy back through pinned staging, write) writing the same
three files into --dir, alternating, `reps` runs each after a warm-up pair; minimum and median.  The two sets of files are compared
once.  Needs an MI355X: no device, no numbers.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def probe(paf, db, K, out_dir, reps):
    import torch
    import alignasm_amd as A
    from alignasm_amd._abi import DevRows, RowsInfo
    from alignasm_amd.api import _dev_structs, rows_format_raw, rows_sizes_raw
    dev = torch.device("cuda", db.device)
    stream = torch.cuda.current_stream(dev)
    res = db.solve(max_paths=K)
    d = res.to_torch(cuts=db)
    stream.synchronize()
    csz, dst, dc = _dev_structs(d)
    cols = db.row_cols()
    n = {"main": d["main"].shape[0], "alt": d["alt"].shape[0], "all": d["all"].shape[0]}
    off = {k: torch.empty(v + 1, dtype=torch.int64, device=dev) for k, v in n.items()}
    ro, info = DevRows(*(off[k].data_ptr() for k in ("main", "alt", "all"))), RowsInfo()
    t_sizes = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        assert rows_sizes_raw(db.dev_view, cols, csz, dst, dc, ro, info, 0, db.device, stream.cuda_stream) == 0
        if rep > 0:
            t_sizes.append((time.perf_counter() - t0) * 1e3)
    assert info.n_flagged == 0, (info.n_flagged, info.bad_list, info.bad_elem, info.bad_flags)
    text = torch.empty(int(info.bytes[0]), dtype=torch.uint8, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t_fill = []
    for rep in range(reps + 1):
        ev[0].record(stream)
        assert rows_format_raw(db.dev_view, cols, csz, dst, dc, ro, info, 0, 0, n["main"], text.data_ptr(), 0, db.device, stream.cuda_stream) == 0
        ev[1].record(stream)
        ev[1].synchronize()
        if rep > 0:
            t_fill.append(ev[0].elapsed_time(ev[1]))
    del text
    bo = res.fetch_raw()
    paths = {w: [os.path.join(out_dir, f"{w}{s}") for s in (".aln.paf", ".aln.alt.paf", ".aln.all.paf")] for w in ("host", "device")}
    t = {"host": [], "device": []}
    same = None
    for rep in range(reps + 1):                                      # (the first pair is the warm-up: page cache, writer buffers, staging)
        for w in ("host", "device"):
            t0 = time.perf_counter()
            if w == "host":
                paf.write_outputs(bo, *paths[w])
            else:
                paf.write_outputs_device(db, d, *paths[w])
            if rep > 0:
                t[w].append(time.perf_counter() - t0)
        if same is None:
            same = all(open(a, "rb").read() == open(b, "rb").read() for a, b in zip(paths["host"], paths["device"]))
    for p in paths["host"] + paths["device"]:
        os.unlink(p)
    A.api.free_out(bo)
    res.close()
    assert same, "the device writer's files differ"
    return {"K": K, "contigs": int(d["n_contigs"]), "rows": n, "bytes": [int(b) for b in info.bytes], "files_equal": same,
            "sizes_ms": round(min(t_sizes), 3), "fill_ms": round(min(t_fill), 3), "fill_ms_median": round(statistics.median(t_fill), 3),
            "fill_GBps": round(int(info.bytes[0]) / min(t_fill) / 1e6, 1),
            "host_write_s": round(min(t["host"]), 4), "host_write_s_median": round(statistics.median(t["host"]), 4),
            "device_write_s": round(min(t["device"]), 4), "device_write_s_median": round(statistics.median(t["device"]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[4])
    ap.add_argument("--contigs", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the output files are written (default: a temporary directory)")
    a = ap.parse_args()
    import alignasm_amd as A
    if A.device_count() < 1:
        sys.exit("rows_probe needs a HIP device: no device, no numbers")
    paf = A.Paf.synth(a.contigs, 1000, 21)
    db = A.DeviceBatch(paf, cs_only=True)                            # the cs text goes to the device, as from a file read with device ranges
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        for K in a.k:
            print(json.dumps(probe(paf, db, K, tmp, a.reps)), flush=True)
    db.close(); paf.close()


if __name__ == "__main__":
    main()
