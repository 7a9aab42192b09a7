"""GPU tier at BASELINE.json's full sizes -- C3 (5 000 contigs x 1 000 records, sparse, K = 4) and
the per-GPU share of C5 (10 000 dense contigs on 8 GPUs = 1 250 x 1 000, K = 16): size-independent
properties of the result + exact comparison with the oracle on a sample of contigs (the oracle needs
seconds per hundred sparse contigs and ~0.1 s per dense one, not per thousands)."""
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the contigs compared with the oracle change from run to run (seeds 3 / 5 sampled the same 48 / 20 contigs every time);
# AASM_TEST_SEED reproduces a run - the seed is printed (pytest shows it with -s or on failure)
SAMPLE_SEED = int(os.environ.get("AASM_TEST_SEED", "0")) or (int(time.time()) ^ os.getpid()) & 0x7fffffff


@pytest.fixture(scope="module")
def c3(T):
    api = T.api()
    paf = api.Paf.synth(5000, 1000, 21, no_cs=True)
    db = api.DeviceBatch(paf)
    res = db.solve(max_paths=4, timing=True)
    out = res.fetch()
    st = res.stats()
    yield paf, db, out, st
    res.close(); db.close(); paf.close()


def _chain_properties(paf, out, st, NC):
    assert (out["status"] == 0).all() and st["n_internal_errors"] == 0 and st["n_unconnectable"] == 0
    view = paf.view()
    from alignasm_amd._abi import _np_from
    rec_off = _np_from(view.ctg_rec_off, NC + 1, np.int64)
    qs_in = _np_from(view.qry_str, int(view.n_records), np.int64)
    qe_in = _np_from(view.qry_end, int(view.n_records), np.int64)
    m, off = out["main"], out["main_off"]
    assert (np.diff(off) >= 1).all()
    ctg = np.repeat(np.arange(NC), np.diff(off))
    rec = rec_off[ctg] + m["ctg_index"]
    # every element stays inside its record and keeps at least one base
    assert (m["ctg_index"] >= 0).all() and (rec < rec_off[ctg + 1]).all()
    assert (qs_in[rec] <= m["qs"]).all() and (m["qs"] <= m["qe"]).all() and (m["qe"] <= qe_in[rec]).all()
    # chain: strictly increasing, non-overlapping query intervals inside a contig (clipping worked)
    same = ctg[1:] == ctg[:-1]
    assert (m["qe"][:-1][same] < m["qs"][1:][same]).all()
    # main path elements were all seen on the un-upgraded path or flagged as alternative
    assert set(np.unique(m["is_alt"])) <= {0, 1}
    # alt list: either empty or a valid chain too
    a, aoff = out["alt"], out["alt_off"]
    actg = np.repeat(np.arange(NC), np.diff(aoff))
    asame = actg[1:] == actg[:-1]
    assert (a["qe"][:-1][asame] < a["qs"][1:][asame]).all()


def test_c3_chain_properties(T, c3):
    paf, db, out, st = c3
    _chain_properties(paf, out, st, 5000)


def test_c4_file_through_the_sharded_path_equals_one_device(T, c3):
    """C4 = the C3 file contig-sharded over 8 GPUs (BASELINE configs[3]; alignasm.cpp:346-361): the SAME 5 000-contig file
    through aasm_solve_batch_multi(n_devices = 8), device ordinals wrapped around the devices of this box - byte for byte
    the one-device result; the cuts are contiguous, cover the file, and the per-shard cost spread is within 2 % of even."""
    from alignasm_amd import shard
    api = T.api()
    paf, db, out, st = c3
    cuts = shard.partition_contigs(paf, 8)
    assert cuts[0] == 0 and cuts[-1] == 5000 and all(b > a for a, b in zip(cuts, cuts[1:]))
    cost = shard.contig_costs(paf)
    loads = np.array([cost[a:b].sum() for a, b in zip(cuts, cuts[1:])])
    assert loads.max() <= 1.02 * loads.mean(), loads
    assert max(b - a for a, b in zip(cuts, cuts[1:])) <= 700
    got = api.solve_batch(paf, max_paths=4, n_devices=8, wrap_devices=True)
    assert T.diff_outputs(out, got, stats=False) == []
    for k in ("n_vertices", "n_edges", "n_heap_nodes", "n_paths_found", "n_pairs", "n_paths_converted"):
        assert st[k] == got["stats"][k], k


def test_c3_idempotent_and_deterministic(T, c3):
    paf, db, out, st = c3
    res2 = db.solve(max_paths=4)
    out2 = res2.fetch(); res2.close()
    assert T.diff_outputs(out, out2, stats=False) == []


def test_c3_whole_batch_matches_oracle(T, c3):
    """All 5 000 contigs against the oracle, every OUT_KEYS array (main, alt, .all, the four offset arrays, status)."""
    paf, db, out, st = c3
    want = T.oracle_solve(paf.batch(), 4, threads=os.cpu_count() or 4)
    assert T.diff_outputs(want, out, stats=False) == []


# ---- C5: the per-GPU share of BASELINE configs[4] (10 000 dense contigs x 1 000 records, K = 16, 8 GPUs)
@pytest.fixture(scope="module")
def c5(T):
    api = T.api()
    paf = api.Paf.synth(1250, 1000, 31, dense=True, no_cs=True)
    db = api.DeviceBatch(paf)
    res = db.solve(max_paths=16, timing=True)
    out = res.fetch()
    st = res.stats()
    yield paf, db, out, st
    res.close(); db.close(); paf.close()


def test_c5_share_chain_properties(T, c5):
    paf, db, out, st = c5
    _chain_properties(paf, out, st, 1250)
    assert st["n_edges"] > 40 * st["n_vertices"] / 3          # the high-multiplicity graph it is meant to be (E/V ~ 20)


def test_c5_share_idempotent(T, c5):
    paf, db, out, st = c5
    res2 = db.solve(max_paths=16)
    out2 = res2.fetch(); res2.close()
    assert T.diff_outputs(out, out2, stats=False) == []


def test_c5_share_whole_batch_matches_oracle(T, c5):
    """All 1 250 dense contigs against the oracle, every OUT_KEYS array (the oracle takes about 0.1 s of one core per contig)."""
    paf, db, out, st = c5
    want = T.oracle_solve(paf.batch(), 16, threads=os.cpu_count() or 4)
    assert T.diff_outputs(want, out, stats=False) == []


def test_c5_file_itself_through_the_sharded_path(T, c5):
    """BASELINE configs[4] as it is defined: the ONE 10 000-contig dense file (10 M records, K = 16), cut by aasm_partition_contigs(8)
    and solved by aasm_solve_batch_multi(n_devices = 8) - device ordinals wrapped around the devices of this box, so the eight
    shards take turns on it (alignasm.cpp:346-361: contigs are independent tasks).  Checked: the cuts are contiguous, cover the
    file and balance the cost model within 3 %; chain properties of the whole result; shard 0 byte for byte against the
    one-device solve of the same contigs generated on their own (aasm_synth_paf_range: what a rank of `bench.py --workload c5
    --gpus 8` holds - the `c5` fixture's 1 250-contig share when the cut falls there); windows of a randomly chosen shard
    against the oracle."""
    from alignasm_amd import shard
    from alignasm_amd._abi import HostBatch
    api = T.api()
    NC = 10000
    whole = api.Paf.synth(NC, 1000, 31, dense=True, no_cs=True)
    cuts = shard.partition_contigs(whole, 8)
    assert cuts[0] == 0 and cuts[-1] == NC and len(cuts) == 9 and all(b > a for a, b in zip(cuts, cuts[1:]))
    ro = api.Paf.synth(NC, 1000, 31, dense=True, records_only=True)
    assert shard.partition_contigs(ro, 8) == cuts                     # what a rank cuts from (no ranges) gives the same blocks
    ro.close()
    cost = shard.contig_costs(whole)
    loads = np.array([cost[a:b].sum() for a, b in zip(cuts, cuts[1:])])
    assert loads.max() <= 1.03 * loads.mean(), loads
    assert max(b - a for a, b in zip(cuts, cuts[1:])) <= 1400
    got = api.solve_batch(whole, max_paths=16, n_devices=8, wrap_devices=True)
    assert got["n_contigs"] == NC
    _chain_properties(whole, got, got["stats"], NC)
    assert got["stats"]["n_edges"] > 40 * got["stats"]["n_vertices"] / 3
    # shard 0 = the contigs a rank generates for itself, solved on one device
    n0 = cuts[1]
    mine = api.Paf.synth(NC, 1000, 31, dense=True, no_cs=True, first=0, count=n0)
    if n0 == 1250:
        paf5, db5, out5, st5 = c5                                     # ... which IS the per-GPU share the other C5 tests solve
        one = out5
    else:
        one = api.solve_batch(mine, max_paths=16)
    mo, ao, po, eo = got["main_off"], got["alt_off"], got["all_path_off"], got["all_elem_off"]
    assert np.array_equal(one["main"], got["main"][:mo[n0]]) and np.array_equal(one["main_off"], mo[:n0 + 1])
    assert np.array_equal(one["alt"], got["alt"][:ao[n0]]) and np.array_equal(one["alt_off"], ao[:n0 + 1])
    assert np.array_equal(one["all"], got["all"][:eo[po[n0]]]) and np.array_equal(one["all_path_off"], po[:n0 + 1])
    mine.close()
    # windows of one of the other shards against the oracle
    print("sample seed (AASM_TEST_SEED reproduces it):", SAMPLE_SEED)
    rng = np.random.default_rng(SAMPLE_SEED + 2)
    sh = int(rng.integers(1, 8))
    for c0 in sorted(int(x) for x in rng.choice(np.arange(cuts[sh], cuts[sh + 1] - 3), size=4, replace=False)):
        hb = HostBatch.from_view_range(whole.view(), c0, c0 + 3)
        want = T.oracle_solve(hb, 16)
        assert np.array_equal(want["main"], got["main"][mo[c0]:mo[c0 + 3]]), (SAMPLE_SEED, sh, c0)
        assert np.array_equal(want["alt"], got["alt"][ao[c0]:ao[c0 + 3]]), (SAMPLE_SEED, sh, c0)
        assert np.array_equal(want["all"], got["all"][eo[po[c0]]:eo[po[c0 + 3]]]), (SAMPLE_SEED, sh, c0)
        assert np.array_equal(want["main_off"], mo[c0:c0 + 4] - mo[c0]), (SAMPLE_SEED, sh, c0)
    whole.close()


def test_two_devices_match_oracle(T):
    """aasm_solve_batch_multi over two GPUs (skipped on a one-GPU box): contig-sharded, no collective."""
    api = T.api()
    if api.device_count() < 2:
        pytest.skip("needs two HIP devices")
    hb = T.synth(64, 150, 9, heavy_tail=True, dup_every=5)
    want = T.oracle_solve(hb, 16)
    got = api.solve_batch(hb, max_paths=16, n_devices=2)
    assert T.diff_outputs(want, got, stats=False) == []


def test_multi_device_entry_equals_single(T):
    """aasm_solve_batch_multi with one device is the plain path; with n > available devices it
    must fail loudly rather than fall back."""
    api = T.api()
    hb = T.synth(12, 80, 5, heavy_tail=True)
    a = api.solve_batch(hb, max_paths=16)
    b = api.solve_batch(hb, max_paths=16, n_devices=1)
    assert T.diff_outputs(a, b, stats=False) == []
    if api.device_count() == 1:
        with pytest.raises(api.AlignasmError):
            api.solve_batch(hb, max_paths=16, n_devices=2)


def _mixed_file(T):
    """Heavy-tailed sparse contigs with a block of dense ones in the middle: contig costs spread over three orders of magnitude."""
    from alignasm_amd._abi import HostBatch
    parts = [T.synth(40, 120, 9, heavy_tail=True, dup_every=5), T.synth(5, 260, 31, dense=True), T.synth(50, 90, 13, heavy_tail=True)]
    a = parts[0].arrays
    mixed = {k: np.concatenate([p.arrays[k] for p in parts]) for k in a if k not in ("ctg_rec_off", "rec_rng_off")}
    for key in ("ctg_rec_off", "rec_rng_off"):
        acc, off = [parts[0].arrays[key]], parts[0].arrays[key][-1]
        for p in parts[1:]:
            acc.append(p.arrays[key][1:] + off)
            off += p.arrays[key][-1]
        mixed[key] = np.concatenate(acc)
    return HostBatch(mixed)


@pytest.mark.parametrize("n_dev", [2, 3, 4, 8])
def test_in_process_multi_device_path_on_the_devices_that_exist(T, n_dev):
    """aasm_solve_batch_multi with n_devices > 1 (alignasm.cpp:351-359: one task per contig -> one thread + stream per device
    block): the thread-per-shard path, the cost-balanced cuts and the concatenation, with device ordinals wrapped around the
    devices of this box (AASM_H2_WRAP_DEVICES), against the oracle on a heavy-tailed + mixed dense / sparse file."""
    api = T.api()
    hb = _mixed_file(T)
    want = T.oracle_solve(hb, 16)
    got = api.solve_batch(hb, max_paths=16, n_devices=n_dev, wrap_devices=True)
    assert T.diff_outputs(want, got, stats=False) == []
    for k in ("n_vertices", "n_edges", "n_heap_nodes", "n_paths_found", "n_pairs"):
        assert want["stats"][k] == got["stats"][k], k


def test_cli_gpus_4_writes_the_same_bytes(T, tmp_path):
    """`alignasm --gpus 4` (shards wrapped around the devices that exist: AASM_TEST_WRAP_DEVICES=1) against `--gpus 1`."""
    import os, subprocess
    api = T.api()
    exe = os.path.join(T.ROOT, "alignasm_amd", "alignasm")
    paf = api.Paf.synth(37, 150, 5, heavy_tail=True, dup_every=4)
    outs = {}
    for g in (1, 4):
        d = tmp_path / ("g%d" % g)
        d.mkdir()
        paf.save(str(d / "x.paf"))
        r = subprocess.run([exe, str(d / "x.paf"), "--gpus", str(g), "--max-paths", "32"], capture_output=True, text=True,
                           env=dict(os.environ, AASM_TEST_WRAP_DEVICES="1"))
        assert r.returncode == 0, r.stderr
        outs[g] = [(d / ("x" + s)).read_bytes() for s in (".aln.paf", ".aln.alt.paf", ".aln.all.paf")]
    assert outs[1] == outs[4] and len(outs[1][0]) > 10000


# ---- the C3 variants real PAFs look like: heavy-tailed contig sizes; duplicated records (multi-mapping)
@pytest.mark.parametrize("variant", ["heavy_tail", "dup3"])
def test_c3_variants_at_full_size(T, variant):
    """5 000 contigs / 5 M records with log-normal contig sizes (1 ... 8 000 records), and with every third record duplicated on
    another chromosome (equal sort keys -> the std::sort replay; tied path scores -> tie runs of conversions): chain properties
    of the whole result, the longest contigs and a random sample against the oracle, all three lists."""
    from alignasm_amd._abi import HostBatch
    api = T.api()
    kw = {"heavy_tail": True} if variant == "heavy_tail" else {"dup_every": 3}
    paf = api.Paf.synth(5000, 1000, 21, no_cs=True, **kw)
    db = api.DeviceBatch(paf)
    res = db.solve(max_paths=4, timing=True)
    out, st = res.fetch(), res.stats()
    if variant == "heavy_tail":
        _chain_properties(paf, out, st, 5000)
    else:                                                            # duplicates: two records may share a query interval, the chain is non-decreasing
        assert (out["status"] == 0).all() and st["n_internal_errors"] == 0
    sizes = np.diff(paf.batch().arrays["ctg_rec_off"])
    print("sample seed (AASM_TEST_SEED reproduces it):", SAMPLE_SEED)
    rng = np.random.default_rng(SAMPLE_SEED + 3)
    pick = set(int(c) for c in np.argsort(-sizes)[:2]) | set(int(c) for c in rng.choice(5000, size=24, replace=False))
    if variant == "heavy_tail":
        assert sizes.max() > 5000 and sizes.min() <= 20
    for c0 in sorted(pick):
        hb = HostBatch.from_view_range(paf.view(), c0, c0 + 1)
        want = T.oracle_solve(hb, 4)
        mo, ao, po, eo = out["main_off"], out["alt_off"], out["all_path_off"], out["all_elem_off"]
        assert np.array_equal(want["main"], out["main"][mo[c0]:mo[c0 + 1]]), (variant, c0)
        assert np.array_equal(want["alt"], out["alt"][ao[c0]:ao[c0 + 1]]), (variant, c0)
        assert np.array_equal(want["all"], out["all"][eo[po[c0]]:eo[po[c0 + 1]]]), (variant, c0)
    res.close(); db.close(); paf.close()


# ---- bench.py --gpus N (the driver's SCALE runs; VERDICT r3: a bare `python bench.py --gpus 8` ran ONE rank)
def _bench(args, env=None):
    import json, os, subprocess, sys
    r = subprocess.run([sys.executable, os.path.join(T_ROOT(), "bench.py")] + args, capture_output=True, text=True, env=dict(os.environ, **(env or {})), timeout=900)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return r, (json.loads(line[-1]) if line else None)


def T_ROOT():
    import os
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_gpus_2_launches_two_ranks_by_itself():
    """`python bench.py --gpus 2` with no launcher and no WORLD_SIZE: bench.py starts torch.distributed.run itself.  On this
    one-GPU box the two ranks share the device (AASM_BENCH_BACKEND=gloo rehearsal); the line says n_gpus 2, strong scaling,
    the whole file's contigs, both blocks of the partition."""
    r, line = _bench(["--gpus", "2", "--steps", "2", "--warmup", "1", "--contigs", "600", "--recs", "300", "--no-extras", "--no-cpu-baseline"],
                     {"AASM_BENCH_BACKEND": "gloo"})
    assert r.returncode == 0, r.stderr[-2000:]
    assert "without a launcher" in r.stderr
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["config"]["contigs_total"] == 600
    assert 0 < line["config"]["contigs_on_fullest_rank"] < 600 and line["value"] > 0


def test_bench_gpus_n_fails_loudly_without_n_devices(T):
    """One rank per GPU is the contract: with fewer devices than ranks the RCCL path must not quietly run fewer ranks."""
    if T.api().device_count() >= 2:
        pytest.skip("this box has the devices")
    r, line = _bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--contigs", "100", "--recs", "100", "--no-extras", "--no-cpu-baseline"])
    assert r.returncode != 0 and line is None
    assert "HIP device(s) visible" in r.stderr or "invalid device ordinal" in r.stderr
