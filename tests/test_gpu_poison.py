"""GPU tier under poisoned working memory.  The allocators of device working memory never clear it: the pipeline's arena hands
the same bytes out solve after solve, the generic graph entries and the device reader take plain hipMalloc blocks.  A kernel that
reads a cell nobody wrote meets zero in a fresh process, the right value after an identical solve, a plausible small integer
after another one - whatever pytest ran before.  With api.debug_poison(byte) every such cell holds the byte instead (0xA5: the
host emulation's; 0xFF: -1, the project's "none"), so "every cell is written before it is read" shows as equality with the
oracle under both bytes.  The one-lane emulation poisons its memory too (tests/host_emul) but never runs the code that exists
only on the card: the sorted-front K8 kernels, the grouped sweeps, the 16-lane and whole-wave row fills, the multi-lane ring
refills, the several-waves heap kernels, the chain class's three roles beside each other, Dial's ballot compaction and its
spill path, the reader's multi-block grids.  Every launch form of those runs here.

All comparisons are exact, on the cells the kernels own.  A HIP error under poison ends the run (poison_testlib.guarded)."""
import functools
import os

import numpy as np
import pytest

import capacity_cases as CC
import cuts_testlib as XC
import ksw_cases as KC
import ksw_cyclic_cases as KY
import read_cases as RC
import read_fuzz as RF
import read_testlib as XR
import rows_testlib as W
import test_dial as DL
import test_dijkstra as DJ
from alignasm_amd import _abi
from poison_testlib import BYTE_IDS, BYTES, cached, guarded, oracle_contigs, oracle_outputs, poisoned, solve_checked
from test_capacity_edges import HEAP_FORMS, RING_FORMS, expected_gb
from test_export_cpu import CASE_IDS as EXPORT_IDS, CASES as EXPORT_CASES
from test_gpu_export import _same
from test_gpu_parity import CASES, _id

pytestmark = pytest.mark.gpu

both_bytes = pytest.mark.parametrize("byte", BYTES, ids=BYTE_IDS)


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("the GPU tier needs torch to see the device")
    return torch


def _synth(T, case):
    nc, nr, seed, K, dense, dup, shuf, heavy, nsl = case
    return T.synth(nc, nr, seed, dense=dense, dup_every=dup, shuffle=shuf, heavy_tail=heavy), K, nsl


# ---- a. the switch is live ------------------------------------------------------------------------------------------------------
def test_arena_padding_reads_the_poison_byte(T):
    """`perm` is an A(...) array of R int32: 4 000 bytes in a 4 096-byte allocation at R = 1 000.  The 96 bytes behind it are the
    allocator's padding, nobody's cells: under the switch they read the byte, while the owned cells equal the oracle's.  With the
    switch back at 0 the next solve equals the oracle again (nothing is said about its padding).
    The two other allocators (the graph entries', the reader's) hand nothing back but owned cells - the results, each written
    whole - so their fill cannot be read back by a test; the graph and reader tests below rely on the results alone."""
    api = T.api()
    hb, K, nsl = _synth(T, CASES[0])
    R = len(hb.arrays["qry_str"])
    assert R == 1000 and (4 * R) % 256 != 0
    want = oracle_outputs(T, _id(CASES[0]), hb, K, nsl)
    db = api.DeviceBatch(hb)
    for byte in BYTES:
        with poisoned(api, byte):
            res = guarded(api, db.solve, max_paths=K, keep_debug=True)
            raw = res.debug("perm", np.uint8)
            assert len(raw) == 4096
            assert (raw[4 * R:] == byte).all(), (hex(byte), raw[4 * R:])
            assert T.diff_intermediates(hb, res.debug, K, nsl) == []
            got = res.fetch()
            assert T.diff_outputs(want, got) == []
            res.close()
        assert api.debug_poison(0) == 0
        res = db.solve(max_paths=K, keep_debug=True)
        got = res.fetch()
        assert T.diff_outputs(want, got) == [] and T.diff_intermediates(hb, res.debug, K, nsl) == []
        res.close()
    db.close()


# ---- b. the pipeline in every launch form -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_default_form_outputs(T, case):
    """Every case of test_gpu_parity.py, the giants included: only they reach the chunked sort replay and the long-tail chain
    class by shape."""
    hb, K, nsl = _synth(T, case)
    for byte in BYTES:
        solve_checked(T, _id(case), hb, K, byte, nsl, intermediates=False)


FORMS = [dict(chain=c, chain_own_queue=q) for c in ("none", "half", "all") for q in (False, True)] + [
    dict(chain="all", test_small_root_ring=True),
    dict(heap_waves="all", heap_block_waves=4), dict(heap_waves="all", heap_block_waves=8), dict(heap_waves="all", heap_block_waves=16),
    dict(heap_waves="all", heap_input_order=True), dict(heap_waves="none"), dict(sequential_select=True), dict(graph_launches=True),
    dict(grid_order=True), dict(non_skip_linkable=True), dict(sort_depth_test=1)]


def check_heap_sorted(T, key, hb, K, nsl, byte, db):
    """sort_depth_test=1 - no partition level, K1's replay goes straight to its heap sort - leaves the oracle's order only where
    keys are distinct: std::sort is not stable, and the oracle's is the one with the real depth limit.  A batch without duplicate
    keys is checked as every other form.  Otherwise `perm`, the array the hook acts on, is compared with std::partial_sort itself
    (the oracle library's oracle_std_sort_perm, what test_sort_replay.py pins the fallback to) for every contig, and the contigs
    without duplicate keys with the oracle in every intermediate."""
    from test_sort_replay import _std
    api = T.api()
    off, qs, qe = hb.arrays["ctg_rec_off"], hb.arrays["qry_str"], hb.arrays["qry_end"]
    keys = lambda c: (np.ascontiguousarray(qs[off[c]:off[c + 1]]), np.ascontiguousarray(qe[off[c]:off[c + 1]]))   # noqa: E731
    distinct = [c for c in range(hb.n_contigs) if len(set(zip(*(k.tolist() for k in keys(c))))) == off[c + 1] - off[c]]
    if len(distinct) == hb.n_contigs:
        solve_checked(T, key, hb, K, byte, nsl, db=db, sort_depth_test=1)
        return
    with poisoned(api, byte):
        res = guarded(api, db.solve, max_paths=K, non_skip_linkable=nsl, keep_debug=True, sort_depth_test=1)
        perm = res.debug("perm", np.int32)
        for c in range(hb.n_contigs):
            if off[c + 1] - off[c] > 1:
                assert np.array_equal(perm[off[c]:off[c + 1]], cached(("heap sorted", key, c), lambda: _std(T, *keys(c), heap_only=1))), (hex(byte), key, c)
        assert T.diff_intermediates(hb, res.debug, K, nsl, contigs=distinct, expect=oracle_contigs(T, key, hb, K, nsl)) == []
        res.close()


@both_bytes
@pytest.mark.parametrize("case", [CASES[0], CASES[3], CASES[5], CASES[8], CASES[9], CASES[13]], ids=_id)
def test_launch_forms_outputs_and_intermediates(T, case, byte):
    hb, K, nsl = _synth(T, case)
    db = T.api().DeviceBatch(hb)
    for form in FORMS:
        hooks = dict(form)
        nsl_f = bool(hooks.pop("non_skip_linkable", nsl))
        if hooks.get("sort_depth_test"):
            check_heap_sorted(T, _id(case), hb, K, nsl_f, byte, db)
        else:
            solve_checked(T, _id(case), hb, K, byte, nsl_f, db=db, **hooks)
    db.close()


@both_bytes
@pytest.mark.parametrize("shape", [(3, 1000, 21, False), (2, 400, 31, True)], ids=["sparse", "dense"])
def test_enumeration_queue_forms(T, shape, byte):
    """K8's three queues (the 64-entry sorted front, the 40-entry one, the d-ary heap) at K = 32 and K = 10 000: kfound and every
    popped distance against the oracle (diff_intermediates), and the outputs."""
    nc, nr, seed, dense = shape
    hb = T.synth(nc, nr, seed, dense=dense)
    db = T.api().DeviceBatch(hb)
    for K in (32, 10000):
        for hooks in ({}, dict(enum_small=True), dict(enum_heap=True)):
            solve_checked(T, ("enum",) + shape, hb, K, byte, db=db, **hooks)
    db.close()


@functools.lru_cache(maxsize=None)
def _crafted(bn):
    B = cached("crafted batches", CC.batches)
    return CC.batch(B[bn])


@both_bytes
@pytest.mark.parametrize("bn,hooks,kernels", RING_FORMS, ids=["chain_class", "one_wave", "grouped"])
def test_sweep_ring_edges(T, bn, hooks, kernels, byte):
    names, hb = _crafted(bn)
    f = solve_checked(T, bn, hb, 4, byte, **hooks)
    assert (f["chain_flag"] == (1 if bn == "ring" and not hooks else 0)).all()


@both_bytes
@pytest.mark.parametrize("bn,hooks", [("rows_sparse", {}), ("rows_sparse", dict(graph_launches=True)), ("rows_dense", {}),
                                      ("rows_dense", dict(graph_launches=True))], ids=["sparse", "sparse_launches", "dense", "dense_launches"])
def test_row_split_edges(T, bn, hooks, byte):
    names, hb = _crafted(bn)
    f = solve_checked(T, bn, hb, 4, byte, **hooks)
    assert (f["gb_flag"] == (1 if bn == "rows_sparse" and not hooks else 0)).all(), f["gb_flag"]


@both_bytes
@pytest.mark.parametrize("hooks,kernel", HEAP_FORMS, ids=["one_wave", "chain_order_wave", "chain_own_queue", "mw4", "mw8", "mw16"])
def test_heap_staging_slot_edges(T, hooks, kernel, byte):
    names, hb = _crafted("heap")
    for K in (4, 10000):
        f = solve_checked(T, "heap", hb, K, byte, **hooks)
        assert (f["mw_flag"] == (1 if hooks.get("heap_waves") == "all" else 0)).all()
        assert (f["chain_flag"] == (1 if hooks.get("chain") == "all" else 0)).all()


@both_bytes
@pytest.mark.parametrize("launches", [False, True], ids=["default", "graph_launches"])
def test_graph_build_limits(T, launches, byte):
    names, hb = _crafted("gb")
    f = solve_checked(T, "gb", hb, 4, byte, graph_launches=launches)
    want, counts = expected_gb(names, launches)
    assert np.array_equal(f["gb_flag"], want), list(f["gb_flag"])
    assert [int(x) for x in f["counters"][18:21]] == counts


@both_bytes
@pytest.mark.parametrize("v", CC.REV_ORD_V)
def test_dense_rev_fill_forms(T, v, byte):
    names, hb = _crafted(f"rev_ord_{v}")
    f = solve_checked(T, f"rev_ord_{v}", hb, 4, byte)
    assert (f["gb_flag"] == 0).all() and (f["chain_flag"] == 0).all()


@both_bytes
@pytest.mark.parametrize("t", [0, 1])
def test_sparse_dense_switch(T, t, byte):
    names, hb = _crafted(f"ratio_{t}")
    f = solve_checked(T, f"ratio_{t}", hb, 4, byte)
    c = names.index(f"ratio_{t}")
    assert f["gb_flag"][c] == f["chain_flag"][c] == (1 if t == 0 else 0)
    if t:
        assert (f["gb_flag"] == 0).all() and (f["chain_flag"] == 0).all()


@both_bytes
def test_several_waves_class_and_long_tail_edges(T, byte):
    names, hb = _crafted("mw")
    f = solve_checked(T, "mw", hb, 4, byte)
    assert list(f["mw_flag"]) == [int(v >= 128 and i >= 6 * v) for v, i in CC.MW_VI] == [0, 0, 0, 1]
    names, hb = _crafted("tail")
    f = solve_checked(T, "tail", hb, 4, byte)
    flag = f["chain_flag"]
    assert [int(flag[names.index(f"tail_{n}")]) for n in CC.TAIL_N] == [0, 1] and int(flag.sum()) == 1
    assert int(f["counters"][17]) == 1


@both_bytes
def test_device_cs_form(T, byte):
    """DeviceBatch(paf, cs_only=True): K0 (KN_CS_RANGES) writes the match ranges into the `rng_rec` A(...) array.  The ranges
    against the container's own, the solve against the host-range solve and the oracle."""
    api = T.api()
    paf = cached("cs paf", lambda: api.Paf.synth(40, 200, 9, dup_every=4, shuffle=True))
    hb = cached("cs hb", paf.batch)
    want = oracle_outputs(T, "cs", hb, 16)
    db = api.DeviceBatch(paf, cs_only=True)
    with poisoned(api, byte):
        res = guarded(api, db.solve, max_paths=16, keep_debug=True)
        n = int(hb.arrays["rec_rng_off"][-1])
        k0 = T.k0_ranges(res.debug)
        for name, key in (("rql_w", "rng_qry_l"), ("rqr_w", "rng_qry_r"), ("rrl_w", "rng_ref_l")):
            assert np.array_equal(k0[name][:n], hb.arrays[key]), name
        got = res.fetch()
        res.close()
        host = guarded(api, api.solve_batch, hb, max_paths=16)
    db.close()
    assert T.diff_outputs(want, got) == [] and T.diff_outputs(want, host) == [] and T.diff_outputs(host, got) == []


@both_bytes
def test_ranges_split_and_concatenated(T, byte):
    """test_max_contigs=7 on 30 contigs: every part is a solve of its own on a re-poisoned arena."""
    api = T.api()
    hb, K, nsl = _synth(T, CASES[10])
    assert hb.n_contigs == 30
    want = oracle_outputs(T, _id(CASES[10]), hb, K, nsl)
    n0 = api.debug_counter("range_splits")
    with poisoned(api, byte):
        got = guarded(api, api.solve_batch, hb, max_paths=K, non_skip_linkable=nsl, test_max_contigs=7)
    assert api.debug_counter("range_splits") - n0 >= 3
    assert T.diff_outputs(want, got, stats=False) == []
    for k in ("n_vertices", "n_edges", "n_heap_nodes", "n_paths_found", "n_pairs"):
        assert want["stats"][k] == got["stats"][k], k


@both_bytes
def test_shape_after_shape_on_one_context(T, byte):
    """A dense 4 x 600 solve, then 200 heavy-tailed contigs, then five contigs of one record, each on the arena the one before
    used - and each on poison, not on what that one left."""
    for case in (CASES[3], CASES[9], CASES[11]):
        hb, K, nsl = _synth(T, case)
        solve_checked(T, _id(case), hb, K, byte, nsl, intermediates=False)


# ---- c. what reads the arena after the solve: the export's scratch is allocated behind the solve's arrays, on poison ------------
@both_bytes
@pytest.mark.parametrize("side", [False, True], ids=["default_stream", "side_stream"])
@pytest.mark.parametrize("case", [EXPORT_CASES[4], EXPORT_CASES[7]], ids=[EXPORT_IDS[4], EXPORT_IDS[7]])
def test_exports_plans_and_rows(T, torch, case, side, byte, tmp_path):
    api = T.api()
    nc, nr, seed, K, dense, dup, shuf, heavy, nsl = case
    paf = api.Paf.synth(nc, nr, seed, dense=dense, heavy_tail=heavy, dup_every=dup, shuffle=shuf)
    db = api.DeviceBatch(paf, cs_only=True)
    stream = torch.cuda.Stream(0) if side else torch.cuda.current_stream(0)
    with poisoned(api, byte):
        res = guarded(api, db.solve, max_paths=K, non_skip_linkable=nsl)
        kw = dict(stream=stream) if side else {}
        plain = guarded(api, res.to_torch, **kw)
        with_cuts = guarded(api, res.to_torch, cuts=db, **kw)
        with_rows = guarded(api, res.to_torch, cuts=db, rows=True, **kw)
        stream.synchronize()
        want = res.fetch()
        bo = res.fetch_raw()
        try:
            files = XC.write_three(paf, bo, tmp_path, "walk")
        finally:
            api.free_out(bo)
        with torch.cuda.stream(stream):
            outs = [api.torch_to_numpy(d) for d in (plain, with_cuts, with_rows)]
            plans = [api.cuts_to_numpy(d) for d in (with_cuts, with_rows)]
            texts = [with_rows[k + "_text"].cpu().numpy().tobytes() for k in W.LISTS]
            offs = {k: with_rows[k + "_row_off"].cpu().numpy() for k in W.LISTS}
        res.close()
    for out in outs:
        _same(want, out, hex(byte))
    n = XC.check_against_host(T, XC.view_arrays(paf.view()), outs[1], plans[0])
    assert n["elements"] == len(want["main"]) + len(want["alt"]) + len(want["all"]) > 0 and n["errors"] == 0 and n["cut"] > 0
    for k in XC.LISTS:
        assert plans[0][k].tobytes() == plans[1][k].tobytes(), k
    assert texts == files and len(files[0]) > 0
    W.check_offsets(offs, texts)
    db.close(); paf.close()


# ---- d. the generic graph entries and the reader: plain hipMalloc blocks -----------------------------------------------------------
@both_bytes
def test_dijkstra(T, byte):
    """The recorded cyclic graphs as one batch; the heap-retry graph alone and in a batch (the retry allocates a second, larger
    heap - poisoned as the first) against the oracle bit for bit."""
    from test_sssp_cpu import batch, heap_retry_graph
    api = T.api()
    z = np.load(os.path.join(T.GOLDEN, "ref_algos.npz"))
    gs = [(int(z[f"dj{i}_meta"][0]), z[f"dj{i}_rowptr"], z[f"dj{i}_col"], z[f"dj{i}_w"], int(z[f"dj{i}_meta"][1])) for i in range(int(z["n_dj"][0]))]
    retry = heap_retry_graph()
    small = cached("dijkstra cases", DJ.cases)[:4]
    mixed = small + [retry] + small[:2]
    with poisoned(api, byte):
        voff, rowptr, col, w, src = batch(gs)
        d, prev = guarded(api, api.sssp_dijkstra, voff, rowptr, col, w, src)
        for i in range(len(gs)):
            assert np.array_equal(d[voff[i]:voff[i + 1]], z[f"dj{i}_d"]) and np.array_equal(prev[voff[i]:voff[i + 1]], z[f"dj{i}_prv"]), i
        n, rp, cl, ww, s = retry
        do, po = cached("retry oracle", lambda: DJ.run(T.oracle(), "oracle_", n, rp, cl, ww, s))
        d, prev = guarded(api, api.sssp_dijkstra, [0, n], rp, cl, ww, [s])
        assert np.array_equal(d, do) and np.array_equal(prev, po)
        voff, rowptr, col, w, src = batch(mixed)
        d, prev = guarded(api, api.sssp_dijkstra, voff, rowptr, col, w, src)
        for i, (n1, rp1, c1, w1, s1) in enumerate(mixed):
            do1, po1 = cached(("dj oracle", i), lambda: DJ.run(T.oracle(), "oracle_", n1, rp1, c1, w1, s1))
            assert np.array_equal(d[voff[i]:voff[i + 1]], do1) and np.array_equal(prev[voff[i]:voff[i + 1]], po1), i


@both_bytes
def test_dial(T, byte):
    """Every recorded case alone and the lim = 2 ones as a batch against ref_dial.npz: the 1 500 / 2 500-vertex fans spill the
    256-entry LDS rings into the `spill` block and refill from it.  One more graph with lim = 7 - eight stacks in play - against
    the oracle's restatement."""
    api = T.api()
    z = np.load(DL.GOLD)
    cs = cached("dial cases", DL.cases)

    def wide():
        rng = np.random.default_rng(20261019)
        rp, col, cost = DL.random_digraph(rng, 1500, 0.002, 7, fan=900)
        return rp, col, cost, DL.run(T.oracle(), "oracle_", 1500, rp, col, cost, 0, 7)
    wrp, wcol, wcost, (wd, wp) = cached("dial wide", wide)
    assert int((wd >= 0).sum()) > 600 and len(set(wcost.tolist())) == 8
    with poisoned(api, byte):
        lim2 = [c for c in cs if c[5] == 2]
        voff = np.concatenate([[0], np.cumsum([c[0] for c in lim2])])
        rps = np.concatenate([[0]] + [c[1][1:] + sum(len(h[2]) for h in lim2[:i]) for i, c in enumerate(lim2)])
        dist, pre = guarded(api, api.sssp_dial, voff, rps, np.concatenate([c[2] for c in lim2]), np.concatenate([c[3] for c in lim2]), np.array([c[4] for c in lim2]), lim=2)
        k = 0
        for i, (n, rp, col, cost, src, lim) in enumerate(cs):
            d1, p1 = guarded(api, api.sssp_dial, np.array([0, n]), rp, col, cost, np.array([src]), lim=lim)
            assert np.array_equal(d1, z[f"c{i}_dist"]) and np.array_equal(p1, z[f"c{i}_pre"]), ("alone", i)
            if lim == 2:
                a, b = voff[k], voff[k + 1]
                assert np.array_equal(dist[a:b], z[f"c{i}_dist"]) and np.array_equal(pre[a:b], z[f"c{i}_pre"]), ("batch", i)
                k += 1
        assert k == len(lim2)
        d1, p1 = guarded(api, api.sssp_dial, np.array([0, 1500]), wrp, wcol, wcost, np.array([0]), lim=7)
        assert np.array_equal(d1, wd) and np.array_equal(p1, wp)


@both_bytes
def test_k_shortest_walks_on_dags(T, byte):
    """The recorded reference runs and mixed random DAGs (a cycle among them), walks and tree: distances, walks, d / best, heap
    roots and node counts against the recorded numbers and the oracle; the arena word for word where the real header is built."""
    api = T.api()
    gold = cached("ksw golden", KC.golden_graphs)
    rand = cached("ksw random", lambda: KC.random_graphs(505, 120))
    wants = cached("ksw random oracle", lambda: [KC.checker_run(T, T.oracle(), "oracle_", g, 5) for g in rand])
    gs, ws = list(rand), list(wants)
    gs.insert(17, KC.cycle_graph()); ws.insert(17, None)
    ref = T.ref(True)
    with poisoned(api, byte):
        b = KC.make_batch(gold)
        got = guarded(api, KC.gpu_run, api, b, 300)
        assert KC.compare(b, gold, [g["want"] for g in gold], got, 300) == []
        b = KC.make_batch(gs)
        assert KC.compare(b, gs, ws, guarded(api, KC.gpu_run, api, b, 5), 5) == []
        if ref is not None:                                          # (as test_gpu_ksw.py: the real header on the monotonic allocator)
            sub = gold[:6] + rand[:12]
            b = KC.make_batch(sub)
            got = guarded(api, KC.gpu_run, api, b, 50)
            off = np.concatenate([[0], np.cumsum(got["heap_nodes"])])
            for gi, g in enumerate(sub):
                w = KC.checker_run(T, ref, "ref_", g, 50)
                nodes = int(w["hcount"][0])
                if w["nd"] == 0:
                    continue
                arena = np.zeros(10 * max(nodes, 1), np.int64)
                ref.ref_generic_heap(arena.ctypes.data_as(T._i64p), T.C.c_int64(nodes))
                assert got["heap_nodes"][gi] == nodes and np.array_equal(got["hook_arena"][off[gi]:off[gi + 1]].reshape(-1), arena[:10 * nodes]), gi


@both_bytes
def test_k_shortest_walks_with_cycles(T, byte):
    """cycles=True: the recorded runs of the real reference (arena included) and mixed cyclic graphs against the plain-Python
    checker, arena node for node."""
    api = T.api()
    gold = cached("kswc golden", KY.golden_graphs)
    rand = cached("kswc random", lambda: KY.random_graphs(705, 120))
    wants = cached("kswc random checker", lambda: [KY.checker_run(g, 5) for g in rand])
    assert all(w is not None for w in wants)
    z = np.load(KY.GOLDEN)
    with poisoned(api, byte):
        b = KC.make_batch(gold)
        got = guarded(api, KY.gpu_run, api, b, 60)
        assert KC.compare(b, gold, [KY.first_walks(g["want"], 60) for g in gold], got, 60) == []
        for gi, g in enumerate(gold):
            if g["want"]["nd"]:
                assert np.array_equal(KY.arena_words(got, gi), z[f"g{gi}_arena"].reshape(-1, 10)), g["name"]
        b = KC.make_batch(rand)
        got = guarded(api, KY.gpu_run, api, b, 5)
        assert KC.compare(b, rand, wants, got, 5) == []
        off = np.concatenate([[0], np.cumsum(got["heap_nodes"])])
        for gi, w in enumerate(wants):
            assert np.array_equal(got["hook_arena"][off[gi]:off[gi + 1]], np.array(w["arena"], np.int64).reshape(-1, 10)), gi


FUZZ = {"fuzz_shaped": 0, "fuzz_long_rows": 3, "fuzz_shaped_solved": 1417, "fuzz_long_rows_solved": 1309}


@pytest.fixture(scope="module")
def read_texts(T):
    """The hand-made texts of tests/read_cases.py and four structured texts of tests/read_fuzz.py: one whose rows all fit a tile and
    one with a row longer than a tile - dozens of rows, but numbers far outside the solver's domain, as nearly all of that corpus -
    and one of each kind with every coordinate inside it, which are solved as well."""
    cases = RC.valid_cases(T.api().Paf.synth(200, 50, 11, dup_every=9, shuffle=True).to_text())
    longest = lambda t: max(len(ln) for _, ln in RF.lines(t))        # noqa: E731
    for name, i in FUZZ.items():
        text = RF.structured_text(i)[0]
        assert (longest(text) > RC.TILE) == ("long_rows" in name) and text.count(b"\n") >= 7
        cases.append(RC.case(name, text, oracle=False, slow=RF.expected_slow(text)))
    return {c["name"]: c for c in cases}


def _read_ids():
    from test_read_cpu import _case_ids
    return _case_ids() + list(FUZZ)


def in_solver_domain(hb):
    """The solver's documented input domain (coordinates in [0, 2^40)): outside it the product refuses the contig, which the
    oracle does not model."""
    return all(((hb.arrays[k] >= 0) & (hb.arrays[k] < (1 << 40))).all() for k in ("qry_str", "qry_end", "ref_str", "ref_end", "qry_total"))


@pytest.mark.parametrize("name", _read_ids())
def test_device_reader_and_solve_of_the_resident_batch(T, read_texts, name):
    """Paf.parse_device under both bytes and the three grid / hash forms: container and resident batch equal the host reader's
    and an uploaded host-read batch field for field; then a poisoned solve of the resident batch against the oracle.
    (`cs_device_tag_list` is the case that found K8's sorted-front queue ending a contig's enumeration after 2 of 15 walks: its
    records run past the query's length, the walks' score sums are negative, and the queue kept them as unsigned words.)"""
    api = T.api()
    fetch = XR.hip_fetcher(api)
    case = read_texts[name]
    text = case["text"]
    host, want, want_text = XR.host_read(api, text)
    up = api.DeviceBatch(host)
    want_dev = XR.view_arrays(up.dev_view, fetch)
    hb = api.Paf.parse(text).batch()                                 # the host reader's match ranges: what the oracle solves
    want_out = T.oracle_solve(hb, 16) if in_solver_domain(hb) else None
    assert want_out is not None or name in ("negative_and_18_digits", "slow_numbers", "fuzz_shaped", "fuzz_long_rows")
    checked_io = False
    for byte in BYTES:
        for flags in (0, _abi.AASM_READ_H_FEW_BLOCKS, _abi.AASM_READ_H_WEAK_HASH):
            with poisoned(api, byte):
                before = api.debug_counter("read_host_fallbacks")
                paf, db = guarded(api, api.Paf.parse_device, text, _flags=flags)
                assert api.debug_counter("read_host_fallbacks") == before and api.debug_counter("read_slow_rows") == case["slow"]
                got_dev = XR.view_arrays(db.dev_view, fetch)
                got_paf, got_text = XR.view_arrays(paf.view()), paf.to_text()
                assert XR.diff_views(want, got_paf) == [] and got_text == want_text, (hex(byte), flags)
                assert XR.diff_views(want, got_dev) == [] and XR.diff_views(want_dev, got_dev) == [], (hex(byte), flags)
                if case["oracle"] and not checked_io:
                    XR.check_against_oracle(T, text, got_paf, got_text)
                    checked_io = True
                if flags == 0 and want_out is not None:
                    res = guarded(api, db.solve, max_paths=16)
                    got = res.fetch()
                    res.close()
                    assert T.diff_outputs(want_out, got) == [], hex(byte)
                db.close(); paf.close()
    up.close()
