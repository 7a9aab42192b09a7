"""bench.py --dump-outputs: what the timed path computed in its last step, as DIR/<name>.npy (float64, <= 64 MB).

CPU tier: the writer on oracle outputs (every contig; a seeded contig sample under a small limit; pieces of one file joined).
GPU tier: bench.py itself at a small size; the dump equals the oracle's answer for the same seeded batch."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("aasm_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in os.listdir(d) if n.endswith(".npy")}


def _check_against(B, z, want):
    """Every dumped array equals the corresponding slice of `want` (a fetched output) for the contigs named in contigs.npy."""
    assert all(a.dtype == np.float64 for a in z.values())
    mo, ao, po, eo = want["main_off"], want["alt_off"], want["all_path_off"], want["all_elem_off"]
    assert np.array_equal(z["contig_table"], np.stack([want["status"], np.diff(mo), np.diff(ao), np.diff(po)], axis=1))
    for j, c in enumerate(z["contigs"].astype(np.int64)):
        for key, off in (("main", mo), ("alt", ao)):
            got = z[key][int(z[key + "_off"][j]):int(z[key + "_off"][j + 1])]
            assert np.array_equal(got, B.records_f64(want[key][off[c]:off[c + 1]])), (key, c)
        p0, p1 = int(z["all_path_off"][j]), int(z["all_path_off"][j + 1])
        got = z["all"][int(z["all_elem_off"][p0]):int(z["all_elem_off"][p1])]
        assert np.array_equal(got, B.records_f64(want["all"][eo[po[c]]:eo[po[c + 1]]])), ("all", c)
        assert np.array_equal(np.diff(z["all_elem_off"][p0:p1 + 1]), np.diff(eo[po[c]:po[c + 1] + 1]))


def test_dump_writes_every_contig_when_it_fits(T, tmp_path):
    import alignasm_amd as A
    B = _bench_module()
    paf = A.Paf.synth(40, 200, 21, no_cs=True)
    want = T.oracle_solve(paf.batch(), 4)
    info = B.dump_outputs(want, str(tmp_path))
    z = _load(str(tmp_path))
    assert info["contigs_dumped"] == 40 and np.array_equal(z["contigs"], np.arange(40))
    assert len(z["main"]) == len(want["main"]) and len(z["all"]) == len(want["all"])
    _check_against(B, z, want)
    paf.close()


def test_dump_samples_contigs_under_the_limit_and_repeats_itself(T, tmp_path):
    import alignasm_amd as A
    B = _bench_module()
    paf = A.Paf.synth(40, 200, 21, no_cs=True)
    want = T.oracle_solve(paf.batch(), 4)
    limit = 20000
    B.dump_outputs(want, str(tmp_path / "a"), limit=limit)
    B.dump_outputs(want, str(tmp_path / "b"), limit=limit)
    za, zb = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sum(os.path.getsize(str(tmp_path / "a" / n)) for n in os.listdir(str(tmp_path / "a"))) <= limit
    assert 0 < len(za["contigs"]) < 40 and np.all(np.diff(za["contigs"]) > 0)
    assert za.keys() == zb.keys() and all(np.array_equal(za[k], zb[k]) for k in za)
    _check_against(B, za, want)
    paf.close()


def test_pieces_of_one_file_join_to_the_whole(T):
    import alignasm_amd as A
    from alignasm_amd._abi import HostBatch
    B = _bench_module()
    paf = A.Paf.synth(40, 200, 21, no_cs=True)
    whole = T.oracle_solve(paf.batch(), 4)
    cat = B.concat_outputs([T.oracle_solve(HostBatch.from_view_range(paf.view(), a, b), 4) for a, b in ((0, 15), (15, 16), (16, 40))])
    assert cat["n_contigs"] == 40
    for k in ("main_off", "alt_off", "all_path_off", "all_elem_off", "status"):
        assert np.array_equal(cat[k], whole[k]), k
    for k in ("main", "alt", "all"):
        for f in ("qs", "qe", "rs", "re", "is_alt"):
            assert np.array_equal(cat[k][f], whole[k][f]), (k, f)
    paf.close()


def test_bench_rejects_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_bench_dump_outputs_equal_the_oracle(T, tmp_path):
    """bench.py at a small C3-shaped size (seed 21, K 4): the line reports the steps asked for, and the dump is the oracle's
    answer for the same seeded batch."""
    import alignasm_amd as A
    B = _bench_module()
    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--contigs", "60", "--recs", "150",
                        "--no-extras", "--no-cpu-baseline", "--dump-outputs", d], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 3 and line["dump_outputs"]["contigs_dumped"] == 60
    paf = A.Paf.synth(60, 150, 21, no_cs=True)
    _check_against(B, _load(d), T.oracle_solve(paf.batch(), 4))
    paf.close()
