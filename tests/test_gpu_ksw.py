"""GPU tier of aasm_k_shortest_walks (row ★K) on the MI355X: the real reference's recorded numbers, the oracle on random DAGs
in big mixed batches, the PAF pipeline's own K6-K8 results on its contig graphs, and - where oracle/_ref is built - the heap
arena word for word against the real header's."""
import numpy as np
import pytest

import ksw_cases as KC

pytestmark = pytest.mark.gpu


def test_gpu_equals_reference_golden(T):
    api = T.api()
    gs = KC.golden_graphs()
    for g in gs:
        b = KC.make_batch([g])
        assert KC.compare(b, [g], [g["want"]], KC.gpu_run(api, b, g["K"]), g["K"]) == []
    b = KC.make_batch(gs)
    assert KC.compare(b, gs, [g["want"] for g in gs], KC.gpu_run(api, b, 300), 300) == []


@pytest.mark.parametrize("K", [1, 5, 64, 2000])
def test_gpu_equals_oracle_mixed_batch(T, K):
    """Hundreds of mixed graphs in one call (cycles among them), each against its own oracle run."""
    api = T.api()
    gs = KC.random_graphs(500 + K, 400)
    wants = [KC.checker_run(T, T.oracle(), "oracle_", g, K) for g in gs]
    for i in (17, 200, 399):
        gs.insert(i, KC.cycle_graph()); wants.insert(i, None)
    b = KC.make_batch(gs)
    got = KC.gpu_run(api, b, K)
    assert KC.compare(b, gs, wants, got, K) == []


def test_gpu_equals_emulation_bitwise(T):
    api = T.api()
    lib = KC.build_emul()
    b = KC.make_batch(KC.random_graphs(77, 150))
    rc, want = KC.emul_run(lib, b, 37)
    assert rc == 0
    got = KC.gpu_run(api, b, 37)
    for key in want:
        assert np.array_equal(want[key], got[key]), key


@pytest.mark.parametrize("case", [(40, 150, 3, False, 0, 4), (40, 150, 3, False, 0, 16), (12, 120, 5, True, 0, 16), (30, 200, 9, False, 7, 4),
                                  (10, 120, 11, True, 5, 10000), (25, 180, 13, False, 0, 10000)],
                         ids=lambda c: "c%d_r%d_s%d_%s_dup%d_K%d" % (c[0], c[1], c[2], "dense" if c[3] else "sparse", c[4], c[5]))
def test_gpu_equals_pipeline_on_contig_graphs(T, case):
    """The contig DAGs of the synthetic generator (src = V - 2, sink = V - 1): n_found, dist5, d5, best and heap_nodes equal
    the pipeline's kfound, kd, sp_d, sp_best and h_cnt of the same solve - the already-pinned K6-K8."""
    nc, nr, seed, dense, dup, K = case
    api = T.api()
    hb = T.synth(nc, nr, seed, dense=dense, dup_every=dup)
    db = api.DeviceBatch(hb)
    res = db.solve(max_paths=K, keep_debug=True)
    batch, contigs, want = KC.pipeline_batch(res, hb, K)
    res.close(); db.close()
    assert len(contigs) > 0
    got = api.k_shortest_walks(batch["g_voff"], batch["rowptr"], batch["col"], batch["w"], batch["src"], batch["sink"], K, walks=True, tree=True)
    assert KC.compare_pipeline(batch, want, got, K) == []
    # every reported walk runs source -> sink over its graph's edges and sums to its distance
    wo, we, w = got["walk_off"], got["walk_edges"], batch["w"]
    tail = np.repeat(np.arange(int(batch["g_voff"][-1])), np.diff(batch["rowptr"]))
    for g in range(0, len(contigs), max(1, len(contigs) // 5)):
        vb = int(batch["g_voff"][g])
        for i in range(int(got["n_found"][g])):
            e = we[wo[g * K + i]:wo[g * K + i + 1]]
            assert tail[e[0]] - vb == batch["src"][g] and batch["col"][e[-1]] == batch["sink"][g]
            assert np.all(batch["col"][e[:-1]] == tail[e[1:]] - vb)
            assert np.array_equal(w[e].sum(0), got["dist"][g, i])


def test_gpu_heap_arena_equals_reference_header(T):
    """The heap arena, node by node ({rank, key, u, v, left, right}), against ref_generic_heap of the real header built on the
    monotonic allocator; skipped where oracle/_ref was not built."""
    ref = T.ref(True)
    if ref is None:
        pytest.skip("oracle/_ref not built (no reference sources on the build machine)")
    api = T.api()
    gs = KC.golden_graphs()[:6] + KC.random_graphs(5, 12)
    b = KC.make_batch(gs)
    got = KC.gpu_run(api, b, 50)
    off = np.concatenate([[0], np.cumsum(got["heap_nodes"])])
    for gi, g in enumerate(gs):
        w = KC.checker_run(T, ref, "ref_", g, 50)
        nodes = int(w["hcount"][0])
        if w["nd"] == 0:
            continue
        assert got["heap_nodes"][gi] == nodes
        arena = np.zeros(10 * max(nodes, 1), np.int64)
        ref.ref_generic_heap(arena.ctypes.data_as(T._i64p), T.C.c_int64(nodes))
        assert np.array_equal(got["hook_arena"][off[gi]:off[gi + 1]].reshape(-1), arena[:10 * nodes]), gi
        vb = int(b["g_voff"][gi])
        assert np.array_equal(got["hook_hroot"][vb:vb + g["n"]], w["hroot"]), gi
