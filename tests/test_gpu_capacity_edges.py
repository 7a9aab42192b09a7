"""Capacity edges, GPU tier: the crafted batches of tests/capacity_cases.py on the card, in every form of each edge.

Several of these edges live in device-only code that the 1-lane emulation of tests/test_capacity_edges.py never runs: the
16-lane / whole-wave row fills past AASM_LONG_ROW and AASM_MID_ROW, the multi-lane refill of the sweeps' LDS ring, the grouped
sweep's two rings per wave, the heap wave's prefetch of the next vertex's keys right after a refilled staging slot, and the
several-waves heap kernels.  Every solve must equal the oracle in outputs and in every intermediate (the heap arena node for
node), and the per-contig form flags must be the ones the shapes predict.  Forms that only a batch's shape can choose (the
dense reversed fill) are asserted in the emulation's launch log there; here the same batches run on the card."""
import numpy as np
import pytest

import capacity_cases as CC
from test_capacity_edges import GB_FLAG, HEAP_FORMS, RING_FORMS, expected_gb

pytestmark = pytest.mark.gpu

K_ = 4


@pytest.fixture(scope="module")
def BF(T):
    return CC.batch_facts(T)


def _solve(T, hb, K=K_, **hooks):
    """HIP solve with the debug arrays kept: outputs and intermediates against the oracle; -> {name: debug array} of the flags."""
    api = T.api()
    want = T.oracle_solve(hb, K)
    db = api.DeviceBatch(hb)
    res = db.solve(max_paths=K, keep_debug=True, **hooks)
    try:
        got = res.fetch()
        got["stats"] = res.stats()
        assert T.diff_outputs(want, got) == [], hooks
        bad = T.diff_intermediates(hb, res.debug, K)
        assert bad == [], (hooks, bad[:6])
        C = hb.n_contigs
        return {n: res.debug(n, np.int32)[:C].copy() for n in ("gb_flag", "mw_flag", "chain_flag")} | \
            {"counters": res.debug("counters", np.int64)[:21].copy()}
    finally:
        res.close()
        db.close()


@pytest.mark.parametrize("bn,hooks,kernels", RING_FORMS, ids=["chain_class", "one_wave", "grouped"])
def test_hip_sweep_ring_edges(T, BF, bn, hooks, kernels):
    """Ready queues of 30 ... 34, 63 ... 65 and 300 entries in both sweeps: the chain class's sweep, the one-wave sweep, and the
    grouped sweep (two contigs a wave, each with its own ring; the wide contigs share waves)."""
    names, hb, _ = BF[bn]
    f = _solve(T, hb, **hooks)
    assert (f["chain_flag"] == (1 if bn == "ring" and not hooks else 0)).all()


@pytest.mark.parametrize("bn,hooks", [("rows_sparse", {}), ("rows_sparse", dict(graph_launches=True)), ("rows_dense", {}),
                                      ("rows_dense", dict(graph_launches=True))], ids=["sparse", "sparse_launches", "dense", "dense_launches"])
def test_hip_row_split_edges(T, BF, bn, hooks):
    """Out-degrees 15, 16, 17 / 95, 96, 97 / 200 on an ordinary vertex and on src: row_fill_tile's one-lane, 16-lane and
    whole-wave rows (the separate launches: graph_launches, or a dense batch) and kb_topo_fill's split at 16."""
    names, hb, _ = BF[bn]
    f = _solve(T, hb, **hooks)
    gb = f["gb_flag"]
    assert (gb == (1 if bn == "rows_sparse" and not hooks else 0)).all(), gb


@pytest.mark.parametrize("hooks,kernel", HEAP_FORMS, ids=["one_wave", "chain_order_wave", "chain_own_queue", "mw4", "mw8", "mw16"])
def test_hip_heap_staging_slot_edges(T, BF, hooks, kernel):
    """15 ... 49 sidetracks on two vertices one after the other in the heap wave's order (refills of the 16-key slot, and the
    next vertex's keys prefetched right after them): the arena equals the oracle's node for node in every heap kernel."""
    names, hb, _ = BF["heap"]
    for K in (K_, 10000):
        f = _solve(T, hb, K, **hooks)
        assert (f["mw_flag"] == (1 if hooks.get("heap_waves") == "all" else 0)).all()
        assert (f["chain_flag"] == (1 if hooks.get("chain") == "all" else 0)).all()


@pytest.mark.parametrize("launches", [False, True], ids=["default", "graph_launches"])
def test_hip_graph_build_limits(T, BF, launches):
    """V = 1 791 / 1 792 / 1 793 / 3 584 / 3 585 and E = 4 095 / 4 096 / 4 097 / 8 192 / 8 193 in one sparse batch: each contig
    in the aasm_k46_graph form (or the separate launches) its counts name."""
    names, hb, _ = BF["gb"]
    f = _solve(T, hb, graph_launches=launches)
    want, counts = expected_gb(names, launches)
    assert np.array_equal(f["gb_flag"], want), (list(f["gb_flag"]), GB_FLAG)
    assert [int(x) for x in f["counters"][18:21]] == counts


@pytest.mark.parametrize("v", CC.REV_ORD_V)
def test_hip_dense_rev_fill_forms(T, BF, v):
    """A dense batch whose largest contig has 3 072 / 3 073 / 12 288 / 12 289 vertices: kb_rev_fill_ord's small and large LDS
    forms and the lane-per-edge fill (the choice: test_capacity_edges.py::test_dense_rev_fill_form_by_largest_contig)."""
    names, hb, _ = BF[f"rev_ord_{v}"]
    f = _solve(T, hb)
    assert (f["gb_flag"] == 0).all() and (f["chain_flag"] == 0).all()


@pytest.mark.parametrize("t", [0, 1])
def test_hip_sparse_dense_switch(T, BF, t):
    names, hb, _ = BF[f"ratio_{t}"]
    f = _solve(T, hb)
    c = names.index(f"ratio_{t}")
    assert f["gb_flag"][c] == f["chain_flag"][c] == (1 if t == 0 else 0)
    if t:
        assert (f["gb_flag"] == 0).all() and (f["chain_flag"] == 0).all()


def test_hip_several_waves_class_edge(T, BF):
    names, hb, _ = BF["mw"]
    f = _solve(T, hb)
    assert list(f["mw_flag"]) == [int(v >= 128 and i >= 6 * v) for v, i in CC.MW_VI] == [0, 0, 0, 1]


def test_hip_chain_class_long_tail_edge(T, BF):
    names, hb, _ = BF["tail"]
    f = _solve(T, hb)
    flag = f["chain_flag"]
    assert [int(flag[names.index(f"tail_{n}")]) for n in CC.TAIL_N] == [0, 1] and int(flag.sum()) == 1
    assert int(f["counters"][17]) == 1
