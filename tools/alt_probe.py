"""Times of the --alt merge on the device, and of the command line with and without --device-alt, on a synthetic main file with an
alt file cut from it.

    python tools/alt_probe.py [--contigs 500] [--recs 1000] [--every 4] [--k 4] [--dir DIR] [--reps 3] [--exe-b OTHER_ALIGNASM]

The alt file: every --every'th row of the main file as a row of a piece "<contig>:1-<qry_total>" of its own contig, rows of one
contig adjacent, aln_len / qry_total on both sides of the 0.5 baseline, no group without a positive ratio.
Stages: DeviceBatch.merge_alt under AASM_READ_TIMING, which waits on the stream at every stage's end (be.stage names of
alt_merge_run and of the reader's front), so the stages are wall times and the run is slower than an untimed one; the untimed merge
is timed in runs of its own, beside the host route (Paf.parse + merge_alt on the container).
Command line: `alignasm main.paf -a alt.paf --device-reader --device-writer --max-paths K --timing` with and without --device-alt,
alternating, --reps times each; --exe-b: another build's binary (the parent commit's) for the run without the flag, same files,
same box.  Prints the library's lines, then one JSON line.  Needs an MI355X.
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
SUFFIXES = (".aln.paf", ".aln.alt.paf", ".aln.all.paf")


def make_files(d, contigs, recs, seed, every):
    import alignasm_amd as A
    os.makedirs(d, exist_ok=True)
    main = os.path.join(d, "altprobe_%d_%d_%d.paf" % (contigs, recs, seed))
    alt = main[:-4] + "_alt%d.paf" % every
    if not (os.path.exists(main) and os.path.exists(alt)):
        A.Paf.synth(contigs, recs, seed).save(main)
        with open(main) as f, open(alt, "w") as out:
            for i, line in enumerate(f):
                if i % every:
                    continue
                c = line.split("\t", 11)
                qtot = int(c[1])
                c[0] = "%s:1-%d" % (c[0], qtot)
                c[10] = str(max(1, qtot * (1 + (i // every) % 9) // 10))          # ratio 0.1 .. 0.9
                out.write("\t".join(c))
    return main, alt


def child(main, alt, mode, reps):
    import alignasm_amd as A
    text = open(alt, "rb").read()
    for _ in range(reps):
        if mode == "host":
            paf = A.Paf.read(main, device_ranges=True)
            t = time.time()
            paf.merge_alt(text, 0.5)
            dt = time.time() - t
            n = int(paf.view().n_records)
            paf.close()
        else:
            _, db = A.Paf.read_device(main, container=False)
            print("probe merge begins", file=sys.stderr, flush=True)
            t = time.time()
            merged = db.merge_alt(text, 0.5)
            dt = time.time() - t
            n = merged.n_records
            merged.close(); db.close()
        print("probe wall %s %.4f %d" % (mode, dt, n), file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=500); ap.add_argument("--recs", type=int, default=1000); ap.add_argument("--seed", type=int, default=21)
    ap.add_argument("--every", type=int, default=4); ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--dir", default="/tmp/aasm_e2e"); ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--exe-b", default=None, help="another build's alignasm for the run without --device-alt")
    ap.add_argument("--child", default=None); ap.add_argument("--main", default=None); ap.add_argument("--alt", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.main, a.alt, a.child, a.reps)
    main_p, alt_p = make_files(a.dir, a.contigs, a.recs, a.seed, a.every)
    out = {"main_bytes": os.path.getsize(main_p), "alt_bytes": os.path.getsize(alt_p)}
    for mode, env in (("host", {}), ("device", {}), ("device", {"AASM_READ_TIMING": "1"})):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--main", main_p, "--alt", alt_p, "--child", mode, "--reps", str(a.reps)],
                           env=dict(os.environ, **env), capture_output=True, text=True)
        if r.returncode != 0:
            sys.stdout.write(r.stderr)
            return r.returncode
        key = mode + ("_timed" if env else "")
        walls = [float(m.group(1)) for m in re.finditer(r"probe wall \w+ ([0-9.]+)", r.stderr)]
        out[key + "_merge_s"] = min(walls)
        out["merged_records"] = int(re.findall(r"probe wall \w+ [0-9.]+ (\d+)", r.stderr)[-1])
        if env:
            last = r.stderr.rsplit("probe merge begins", 1)[1]
            sys.stdout.write(last)
            out["stages_ms"] = {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"aasm read stage: (.+?)\s+([0-9.]+) ms", last)}
    exe = os.path.join(ROOT, "alignasm_amd", "alignasm")
    base = [main_p, "-a", alt_p, "--max-paths", str(a.k), "--timing", "--device-reader", "--device-writer"]
    runs = {"device_alt": [], "host_alt": []}
    for rep in range(a.reps):
        for key, cmd in (("host_alt", [a.exe_b or exe] + base), ("device_alt", [exe] + base + ["--device-alt"])):
            for s in SUFFIXES:                                            # to NEW files (replacing a big file frees its page cache inside rename())
                if os.path.exists(main_p[:-4] + s):
                    os.remove(main_p[:-4] + s)
            t = time.time()
            r = subprocess.run(cmd, capture_output=True, text=True)
            wall = time.time() - t
            line = next((ln for ln in r.stderr.splitlines() if ln.startswith("alignasm timing")), "")
            print("%s run %d: rc=%d wall %.3f s | %s" % (key, rep, r.returncode, wall, line), flush=True)
            m = re.search(r"read_s ([0-9.e-]+) .* total_s ([0-9.e-]+) container (\d)", line)
            if r.returncode == 0 and m:
                runs[key].append({"wall_s": round(wall, 4), "read_s": float(m.group(1)), "total_s": float(m.group(2)), "container": int(m.group(3))})
    out["cli"] = runs
    out["cli_host_alt_exe"] = a.exe_b or exe
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
