"""Capacity edges, CPU tier: the crafted batches of tests/capacity_cases.py through the kernel bodies (1-lane host emulation).

Each batch puts contigs at, one below and one above a fixed-size structure of the kernels (the sweeps' 32-entry LDS ring, the
row-fill lane split, the heap wave's 16-key staging slot, the graph-build limits, the reversed-CSR fill forms, the sparse /
dense switch, the several-waves and chain classes).  The oracle says where each contig lands; the emulation must equal the
oracle in outputs and intermediates under every form that edge has, and the form must be the one the shape (or hook) names.
Several of these edges are in device-only code: the GPU tier runs the same batches on the card
(tests/test_gpu_capacity_edges.py)."""
import numpy as np
import pytest

import capacity_cases as CC

K_ = 4


@pytest.fixture(scope="module")
def BF(T):
    return CC.batch_facts(T)


def test_crafted_batches_reach_every_capacity_edge(T, BF):
    """Every value the capacity tests are for, counted from the oracle's own intermediates (CSR, SP tree, both sweeps' orders
    replayed in the kernels' push order): a crafted contig that misses its target fails here."""
    got, miss = CC.coverage(T, BF)
    assert miss == [], miss


def test_ring_replay_counts_the_spill_path():
    """The sweep replay itself on hand-made graphs: a fan of m released at once waits m entries; the window holds 31 waiting
    entries beside the one at hand, so the spill path starts at 32; from there on the window stops growing and every later
    entry is fetched from global memory (and more than 32 sources start the window full)."""
    def fan_graph(m):                                  # 0 -> 1..m -> m + 1
        rp = [0, m] + [m + j for j in range(1, m + 1)] + [2 * m]
        col = list(range(1, m + 1)) + [m + 1] * m
        return np.array(rp), np.array(col)
    for m, spill in ((30, False), (31, False), (32, True), (33, True), (64, True)):
        rp, col = fan_graph(m)
        for rev in (False, True):
            q, occ, sp = CC.kahn(rp, col, rev)
            assert occ == m and (sp > 0) == spill, (m, rev, occ, sp)
            assert sp == (m + 2 - CC.REVQ_N if spill else 0), (m, rev, sp)
    rp = np.array([0] * 33 + [0])                      # 33 isolated vertices: 33 sources at once
    assert CC.kahn(rp, np.zeros(0, np.int64), False)[1:] == (33, 1)


def _run(T, hb, K=K_, **hooks):
    want = T.oracle_solve(hb, K)
    got = T.emul_solve(hb, K, **hooks)
    assert T.diff_outputs(want, got) == [], hooks
    assert T.diff_intermediates(hb, T.emul_debug, K) == [], hooks
    return {name for name, _, _ in T.emul_launches()}


RING_FORMS = [("ring", {}, {"KN_CHAIN", "KN_FWD_SWEEP"}), ("ring", dict(chain="none"), {"KN_REV_SWEEP", "KN_FWD_SWEEP"}),
              ("grouped", {}, {"KN_REV_SWEEP_G", "KN_FWD_SWEEP_G"})]


@pytest.mark.parametrize("bn,hooks,kernels", RING_FORMS, ids=["chain_class", "one_wave", "grouped"])
def test_sweep_ring_edges(T, BF, bn, hooks, kernels):
    names, hb, _ = BF[bn]
    ks = _run(T, hb, **hooks)
    assert kernels <= ks, ks
    if bn == "grouped":
        assert not {"KN_CHAIN", "KN_CHAIN3", "KN_REV_SWEEP", "KN_FWD_SWEEP"} & ks


@pytest.mark.parametrize("bn,hooks", [("rows_sparse", {}), ("rows_sparse", dict(graph_launches=True)), ("rows_dense", {}),
                                      ("rows_dense", dict(graph_launches=True))], ids=["sparse", "sparse_launches", "dense", "dense_launches"])
def test_row_split_edges(T, BF, bn, hooks):
    names, hb, _ = BF[bn]
    ks = _run(T, hb, **hooks)
    assert "KN_TOPO_FILL" in ks
    if bn == "rows_sparse" and not hooks:
        assert "KN_GRAPH" in ks and "KN_ROW_FILL" not in ks
    else:
        assert "KN_ROW_FILL" in ks and not {"KN_GRAPH", "KN_GRAPH_L"} & ks


HEAP_FORMS = [(dict(chain="none", heap_waves="none"), "KN_HEAP"), (dict(chain="all"), "KN_CHAIN"),
              (dict(chain="all", chain_own_queue=True), "KN_CHAIN3"), (dict(heap_waves="all", heap_block_waves=4), "KN_HEAP_MW"),
              (dict(heap_waves="all", heap_block_waves=8), "KN_HEAP_MW8"), (dict(heap_waves="all", heap_block_waves=16), "KN_HEAP_MW16")]


@pytest.mark.parametrize("hooks,kernel", HEAP_FORMS, ids=["one_wave", "chain_order_wave", "chain_own_queue", "mw4", "mw8", "mw16"])
def test_heap_staging_slot_edges(T, BF, hooks, kernel):
    """15 ... 49 sidetracks on two vertices that follow each other in the heap wave's order, in every heap kernel; the arena
    (keys, children, ranks, roots) equals the oracle's node for node (diff_intermediates)."""
    names, hb, _ = BF["heap"]
    for K in (K_, 10000):
        ks = _run(T, hb, K, **hooks)
        assert kernel in ks, ks


GB_FLAG = {"gbV_1791": 1, "gbV_1792": 1, "gbV_1793": 2, "gbV_3584": 2, "gbV_3585": 0,
           "gbE_4095": 1, "gbE_4096": 1, "gbE_4097": 2, "gbE_8192": 2, "gbE_8193": 0}


def expected_gb(names, launches):
    want = np.array([0 if launches else GB_FLAG[n] for n in names])
    return want, [int((want == 1).sum()), int((want == 2).sum()), int((want == 0).sum())]


@pytest.mark.parametrize("launches", [False, True], ids=["default", "graph_launches"])
def test_graph_build_limits(T, BF, launches):
    names, hb, _ = BF["gb"]
    ks = _run(T, hb, graph_launches=launches)
    want, counts = expected_gb(names, launches)
    assert np.array_equal(T.emul_debug("gb_flag", np.int32)[:len(names)], want)
    assert [int(x) for x in T.emul_debug("counters", np.int64)[18:21]] == counts
    assert ("KN_GRAPH" in ks, "KN_GRAPH_L" in ks, "KN_ROW_FILL" in ks) == ((False, False, True) if launches else (True, True, True))


REV_FILL = {3072: "KN_REV_FILL_ORD_S", 3073: "KN_REV_FILL_ORD", 12288: "KN_REV_FILL_ORD", 12289: "KN_REV_FILL_W"}


@pytest.mark.parametrize("v", CC.REV_ORD_V)
def test_dense_rev_fill_form_by_largest_contig(T, BF, v):
    names, hb, _ = BF[f"rev_ord_{v}"]
    ks = _run(T, hb)
    fills = {k for k in ks if k.startswith("KN_REV_FILL")}
    assert fills == {REV_FILL[v]}, fills


@pytest.mark.parametrize("t", [0, 1])
def test_sparse_dense_switch(T, BF, t):
    """ET = 6 VT is still sparse (the sparse reversed fill, aasm_k46_graph and the chain class where a contig fits them);
    ET = 6 VT + 1 is dense (the dense reversed fill, neither of the others)."""
    names, hb, _ = BF[f"ratio_{t}"]
    ks = _run(T, hb)
    gb = T.emul_debug("gb_flag", np.int32)[:len(names)]
    fills = {k for k in ks if k.startswith("KN_REV_FILL")}
    if t == 0:
        assert fills == {"KN_REV_FILL"} and "KN_GRAPH" in ks and "KN_CHAIN" in ks and gb[names.index("ratio_0")] == 1
    else:
        assert fills == {"KN_REV_FILL_ORD"} and not {"KN_GRAPH", "KN_GRAPH_L", "KN_CHAIN", "KN_CHAIN3"} & ks and (gb == 0).all()


def test_several_waves_class_edge(T, BF):
    """mw_flag = I >= 6 V && V >= 128, by default (and every contig with heap_waves="all", none with "none")."""
    names, hb, _ = BF["mw"]
    want = np.array([int(v >= 128 and i >= 6 * v) for v, i in CC.MW_VI])
    assert list(want) == [0, 0, 0, 1]
    for hooks, w in (({}, want), (dict(heap_waves="all"), np.ones(4)), (dict(heap_waves="none"), np.zeros(4))):
        ks = _run(T, hb, **hooks)
        assert np.array_equal(T.emul_debug("mw_flag", np.int32)[:4], w), hooks
        assert bool({"KN_HEAP_MW", "KN_HEAP_MW8", "KN_HEAP_MW16"} & ks) == bool(w.any())


def test_chain_class_long_tail_edge(T, BF):
    """In a batch of more than 1 536 contigs the chain class is the contigs of >= max(2 048, 4 x mean) records: 2 048, not 2 047."""
    names, hb, _ = BF["tail"]
    ks = _run(T, hb)
    flag = T.emul_debug("chain_flag", np.int32)[:len(names)]
    assert [int(flag[names.index(f"tail_{n}")]) for n in CC.TAIL_N] == [0, 1]
    assert int(flag.sum()) == 1 and int(T.emul_debug("counters", np.int64)[17]) == 1
    assert "KN_CHAIN" in ks


def test_chain_class_takes_every_contig_of_the_small_batches(T, BF):
    for bn in ("ring", "heap", "rows_sparse"):
        names, hb, _ = BF[bn]
        _run(T, hb)
        assert (T.emul_debug("chain_flag", np.int32)[:len(names)] == 1).all(), bn
