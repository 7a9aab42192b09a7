"""Times of the cut plans on the C3 file (5 000 contigs x 1 000 records, seed 21), one JSON line per K.

    python tools/cut_probe.py [--k 4 10000] [--contigs 5000] [--dir DIR]

cut_ms: HIP events around aasm_cut_plans_device on the torch stream, into buffers allocated once, minimum of 10 after a warm-up;
export_ms: the same around aasm_result_export, for scale.  elements / recut / recut_tag_bytes: the result's elements, those that do
not span their record, and the bytes of the tags these span (what the host writer walks, and the kernel at most).
walk_write_s / plan_write_s: wall times of Paf.write_outputs without and with the plans (aasm_writer_append against
aasm_writer_append_cuts, both through open + append + close) writing the same three files into --dir, alternating, 5 runs each
in this one process; minimum and median.  The two sets of files are compared once.  Needs an MI355X: no device, no numbers.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def probe(paf, db, K, out_dir):
    import numpy as np
    import torch
    import alignasm_amd as A
    from alignasm_amd._abi import DevCuts, DevOut, OutSizes, _np_from
    stream = torch.cuda.current_stream(0)
    res = db.solve(max_paths=K)
    d = res.to_torch(cuts=db)
    stream.synchronize()
    sz = res.sizes()
    csz = OutSizes(*(sz[n] for n, _ in OutSizes._fields_))
    ptr = lambda t: t.data_ptr() if t.numel() else None   # noqa: E731
    dst = DevOut(*(ptr(d[k]) for k in ("main_off", "alt_off", "all_path_off", "all_elem_off", "main", "alt", "all", "status")))
    dc = DevCuts(ptr(d["main_cut"]), ptr(d["alt_cut"]), ptr(d["all_cut"]))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t_cut, t_exp = [], []
    for rep in range(11):
        ev[0].record(stream)
        assert res.export_raw(csz, dst, stream.cuda_stream) == 0
        ev[1].record(stream)
        assert A.api.cut_plans_raw(db.dev_view, csz, dst, dc, 0, stream.cuda_stream) == 0
        ev[2].record(stream)
        ev[2].synchronize()
        if rep > 0:
            t_exp.append(ev[0].elapsed_time(ev[1])); t_cut.append(ev[1].elapsed_time(ev[2]))
    plans = A.cuts_to_numpy(d)
    out = A.torch_to_numpy(d)
    # the tags the re-cut elements span
    v = paf.view()
    cs_off = _np_from(v.rec_cs_off, int(v.n_records) + 1, np.int64)
    rec_off = _np_from(v.ctg_rec_off, int(v.n_contigs) + 1, np.int64)
    tag_len = np.diff(cs_off)
    c_of = {"main": np.repeat(np.arange(out["n_contigs"]), np.diff(out["main_off"])), "alt": np.repeat(np.arange(out["n_contigs"]), np.diff(out["alt_off"]))}
    path_c = np.repeat(np.arange(out["n_contigs"]), np.diff(out["all_path_off"]))
    c_of["all"] = np.repeat(path_c, np.diff(out["all_elem_off"])) if len(path_c) else np.zeros(0, np.int64)
    n_el = n_cut = n_bytes = n_odd = 0
    for k in ("main", "alt", "all"):
        cut = (plans[k]["flags"] & 1) != 0
        rec = rec_off[c_of[k]] + out[k]["ctg_index"]
        n_el += len(cut); n_cut += int(cut.sum()); n_bytes += int(tag_len[rec[cut]].sum()); n_odd += int(((plans[k]["flags"] & ~1) != 0).sum())
    # the two writers, alternating
    bo = res.fetch_raw()
    paths = {w: [os.path.join(out_dir, f"{w}{s}") for s in (".aln.paf", ".aln.alt.paf", ".aln.all.paf")] for w in ("walk", "plan")}
    t = {"walk": [], "plan": []}
    same = None
    for rep in range(6):                                             # (the first pair is the warm-up: page cache, writer buffers)
        for w in ("walk", "plan"):
            t0 = time.perf_counter()
            paf.write_outputs(bo, *paths[w], cuts=plans if w == "plan" else None)
            if rep > 0:
                t[w].append(time.perf_counter() - t0)
        if same is None:
            same = all(open(a, "rb").read() == open(b, "rb").read() for a, b in zip(paths["walk"], paths["plan"]))
    size = sum(os.path.getsize(p) for p in paths["walk"])
    for p in paths["walk"] + paths["plan"]:
        os.unlink(p)
    A.api.free_out(bo)
    res.close()
    assert same, "the planned writer's files differ"
    return {"K": K, "contigs": sz["n_contigs"], "elements": n_el, "recut": n_cut, "recut_tag_bytes": n_bytes, "irregular_or_error": n_odd,
            "cut_ms": round(min(t_cut), 4), "cut_ms_median": round(statistics.median(t_cut), 4), "export_ms": round(min(t_exp), 4),
            "output_bytes": size, "files_equal": same,
            "walk_write_s": round(min(t["walk"]), 4), "walk_write_s_median": round(statistics.median(t["walk"]), 4),
            "plan_write_s": round(min(t["plan"]), 4), "plan_write_s_median": round(statistics.median(t["plan"]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[4, 10000])
    ap.add_argument("--contigs", type=int, default=5000)
    ap.add_argument("--dir", default=None, help="where the output files are written (default: a temporary directory)")
    a = ap.parse_args()
    import alignasm_amd as A
    if A.device_count() < 1:
        sys.exit("cut_probe needs a HIP device: no device, no numbers")
    paf = A.Paf.synth(a.contigs, 1000, 21)
    db = A.DeviceBatch(paf, cs_only=True)                            # the cs text goes to the device, as from a file read with device ranges
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        for K in a.k:
            print(json.dumps(probe(paf, db, K, tmp)), flush=True)
    db.close(); paf.close()


if __name__ == "__main__":
    main()
