"""Times of the device reader beside the host reader's on one PAF file, the C3 file by default (5 000 contigs x 1 000 records,
seed 21).

    python tools/read_probe.py [--contigs 5000] [--recs 1000] [--paf FILE] [--dir DIR] [--reps 3]

Host reader: Paf.read(file, device_ranges=True) under AASM_IO_TIMING (its stages: index, allocate, parse + copy).  Device reader:
Paf.read_device(file) under AASM_READ_TIMING, which waits on the stream around every launch and stage, so the kernels' times are
wall times of a launch alone and the run is slower than an untimed one; the untimed wall time is measured in runs of its own.
Prints the library's lines as they come, then one JSON line: wall times (minimum of --reps), per-kernel ms of the last timed run,
GB/s of the row-start kernels (text bytes read) and of the packing kernel (tag bytes read + written).  Needs an MI355X.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(path, mode, reps):
    import alignasm_amd as A
    for _ in range(reps):
        t = time.time()
        if mode == "host":
            paf = A.Paf.read(path, device_ranges=True)
            cs = 0
        else:
            paf, db = A.Paf.read_device(path)
            v = paf.view()
            cs = int(A._abi._np_from(v.rec_cs_off, int(v.n_records) + 1, "int64")[-1])
            db.close()
        print("probe wall %s %.4f %d" % (mode, time.time() - t, cs), file=sys.stderr, flush=True)
        paf.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=5000); ap.add_argument("--recs", type=int, default=1000); ap.add_argument("--seed", type=int, default=21)
    ap.add_argument("--paf", default=None); ap.add_argument("--dir", default="/tmp/aasm_e2e"); ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.paf, a.child, a.reps)
    path = a.paf
    if path is None:
        import alignasm_amd as A
        os.makedirs(a.dir, exist_ok=True)
        path = os.path.join(a.dir, "probe_%d_%d_%d.paf" % (a.contigs, a.recs, a.seed))
        if not os.path.exists(path):
            A.Paf.synth(a.contigs, a.recs, a.seed).save(path)
    size = os.path.getsize(path)
    out = {"file_bytes": size}
    for mode, env in (("host", {"AASM_IO_TIMING": "1"}), ("device", {}), ("device", {"AASM_READ_TIMING": "1"})):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--paf", path, "--child", mode, "--reps", str(a.reps)], env=dict(os.environ, **env),
                           capture_output=True, text=True)
        sys.stdout.write(r.stderr)
        if r.returncode != 0:
            raise SystemExit("read_probe: the %s reader failed (%d)" % (mode, r.returncode))
        walls = [(float(m.group(1)), int(m.group(2))) for m in re.finditer(r"probe wall \w+ ([0-9.]+) (\d+)", r.stderr)]
        key = mode + ("_timed" if env.get("AASM_READ_TIMING") else "")
        out[key + "_wall_s"] = min(w for w, _ in walls)
        if env.get("AASM_READ_TIMING"):
            last = r.stderr.rsplit("aasm read stage: upload", 1)[-1] if "aasm read stage: upload" in r.stderr else r.stderr
            kern = {m.group(1): float(m.group(2)) for m in re.finditer(r"aasm read kernel: (\w+)\s+([0-9.]+) ms", r.stderr)}   # (later runs overwrite: the last one)
            out["kernel_ms"] = kern
            out["stage_ms"] = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"aasm read stage: ([\w ]+?)\s+([0-9.]+) ms", last)}
            cs = walls[-1][1]
            out["cs_bytes"] = cs
            gbs = lambda b, ms: round(b / 1e9 / (ms / 1e3), 1) if ms > 0 else None   # noqa: E731
            out["gbps"] = {"aasm_read_count": gbs(size, kern.get("aasm_read_count", 0)), "aasm_read_starts": gbs(size, kern.get("aasm_read_starts", 0)),
                           "aasm_read_rows": gbs(size, kern.get("aasm_read_rows", 0)), "aasm_read_pack": gbs(2 * cs, kern.get("aasm_read_pack", 0))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
