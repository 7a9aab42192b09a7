"""GPU tier of aasm_topology_sort and aasm_sssp_dag, under poisoned working memory as tests/test_gpu_poison.py: the 64-lane list walk
of kb_sssp_dag (alignasm_amd/csrc/aasm_sssp.h) - the atomic countdown with heads that repeat inside a chunk and across chunks, the
appends by a head's last lane, the parallel stores and the shared heads settled in lane order - exists only on the card; the
one-lane emulation of tests/test_dag_cpu.py never sees a chunk of more than one edge.  Every comparison is exact: against the real
reference's recorded runs (ref_dag.npz), the plain-Python checker, aasm_k_shortest_walks' tree and the pipeline's own sweeps."""
import numpy as np
import pytest

import bf_cases as BC
import dag_cases as DC
import ksw_cases as KC
from poison_testlib import BYTE_IDS, BYTES, cached, guarded, poisoned

pytestmark = pytest.mark.gpu

both_bytes = pytest.mark.parametrize("byte", BYTES, ids=BYTE_IDS)
MAX = [-1, -1, -1, -1, 0]


def _random():
    gs = cached("dag random", lambda: DC.random_graphs(4713, 160))
    return gs, cached("dag random checker", lambda: [DC.checker(g) for g in gs])


@both_bytes
def test_dag_on_the_whole_case_set(T, byte):
    """Every recorded graph and fresh random ones in one call: order, d, prev, status against the reference's runs and the checker;
    then every hub and fan-in graph alone, a batch of its own."""
    api = T.api()
    gold = DC.golden_graphs()
    rand, wants = _random()
    gs, ws = gold + rand, [g["want"] for g in gold] + wants
    with poisoned(api, byte):
        b = KC.make_batch(gs)
        assert DC.compare_dag(b, gs, ws, guarded(api, DC.gpu_dag, api, b)) == []
        hubs = [g for g in gold if g["name"].startswith(("hub_", "fan_in_", "parallel_straddle_"))]
        assert len(hubs) == 12
        for g in hubs:
            b = KC.make_batch([g])
            assert DC.compare_dag(b, [g], [g["want"]], guarded(api, DC.gpu_dag, api, b)) == [], g["name"]


@both_bytes
def test_topology_sort_alone(T, byte):
    """aasm_topology_sort equals the order of aasm_sssp_dag and the fixture; without order=True the distances are the same."""
    api = T.api()
    gold = DC.golden_graphs()
    rand, wants = _random()
    gs, ws = gold + rand, [g["want"] for g in gold] + wants
    with poisoned(api, byte):
        b = KC.make_batch(gs)
        topo = guarded(api, DC.gpu_topo, api, b)
        full = guarded(api, DC.gpu_dag, api, b)
        d, prev, status = guarded(api, api.sssp_dag, b["g_voff"], b["rowptr"], b["col"], b["w"], b["src"])
    assert DC.compare_dag(b, gs, ws, topo) == []
    assert np.array_equal(topo["order"], full["order"]) and np.array_equal(topo["status"], full["status"])
    assert np.array_equal(d, full["d"]) and np.array_equal(prev, full["prev"]) and np.array_equal(status, full["status"])


@both_bytes
def test_cycles_among_dags(T, byte):
    """Cyclic and acyclic graphs alternating in one batch: the statuses sit on the right graphs, the cyclic ones hold the reset
    values, the acyclic ones are word for word what they are when solved alone."""
    api = T.api()
    gold = DC.golden_graphs()
    bad = [g for g in gold if g["want"]["status"] == 1]
    good = [g for g in gold if g["want"]["status"] == 0 and g["name"].startswith(("hub_", "fan_in_", "random_"))][:len(bad) * 3]
    assert len(bad) == 6
    gs = [x for i, g in enumerate(good) for x in ((bad[i % len(bad)], g))]
    with poisoned(api, byte):
        b = KC.make_batch(gs)
        got = guarded(api, DC.gpu_dag, api, b)
        alone = guarded(api, DC.gpu_dag, api, KC.make_batch(gs[1::2]))
    assert list(got["status"]) == [1, 0] * (len(gs) // 2)
    assert DC.compare_dag(b, gs, [g["want"] for g in gs], got) == []
    for gi in range(0, len(gs), 2):
        vb, n, s = int(b["g_voff"][gi]), gs[gi]["n"], gs[gi]["src"]
        want_d = np.tile(np.array(MAX, np.int64), (n, 1)); want_d[s] = 0
        assert np.array_equal(got["d"][vb:vb + n], want_d) and (got["prev"][vb:vb + n] == -1).all() and (got["order"][vb:vb + n] == -1).all()
    vt = np.concatenate([np.arange(b["g_voff"][i], b["g_voff"][i + 1]) for i in range(1, len(gs), 2)])
    for key in ("d", "prev", "order"):
        assert np.array_equal(got[key][vt], alone[key]), key


@both_bytes
def test_reversed_graph_equals_k_walks_tree(T, byte):
    """Against code that is already pinned: on ksw_cases' DAG batches the run over the reversed graph from the sink gives
    api.k_shortest_walks(tree=True)'s d5 and best."""
    api = T.api()
    gs = cached("dag ksw graphs", lambda: KC.random_graphs(321, 200))
    b = KC.make_batch(gs)
    rb = KC.make_batch([DC.reversed_graph(g) for g in gs])
    with poisoned(api, byte):
        tree = guarded(api, api.k_shortest_walks, b["g_voff"], b["rowptr"], b["col"], b["w"], b["src"], b["sink"], 4, walks=False, tree=True)
        got = guarded(api, DC.gpu_dag, api, rb)
    assert not tree["status"].any() and not got["status"].any()
    assert np.array_equal(got["d"], tree["d"]) and np.array_equal(got["prev"], tree["best"])


def test_contig_graphs_equal_the_pipeline(T):
    """Contig graphs from a solve with keep_debug, a C1-size batch and overhang contigs with negative edges: the forward graph's
    order is the pipeline's fwd_order; the reversed graph from the sink gives its rev_order, sp_d and sp_best."""
    import overhang_cases as OC
    api = T.api()
    hbs = [T.synth(10, 100, 1)] + [OC.overhang(T.synth(nc, nr, seed), mode, seed) for nc, nr, seed, mode in BC.OVERHANG_BATCHES]
    seen_negative = False
    for hb in hbs:
        batch, want = DC.pipeline_dags(api, hb)
        seen_negative |= bool((batch["w"][:, 0] + batch["w"][:, 1] < 0).any())
        rb = DC.reversed_batch(batch)
        with poisoned(api, BYTES[0]):
            fwd = guarded(api, DC.gpu_dag, api, batch)
            rev = guarded(api, DC.gpu_dag, api, rb)
            topo = guarded(api, DC.gpu_topo, api, batch)
        assert not fwd["status"].any() and not rev["status"].any()
        assert np.array_equal(fwd["order"], want["fwd_order"]) and np.array_equal(topo["order"], want["fwd_order"])
        assert np.array_equal(rev["order"], want["rev_order"])
        assert np.array_equal(rev["d"], want["d5"]) and np.array_equal(rev["prev"].astype(np.int64), want["best"])
    assert seen_negative


def test_large_dags_with_permuted_ids(T):
    """One batch of 8 random DAGs of 5 000 vertices with permuted ids, against the checker."""
    api = T.api()
    gs = DC.random_graphs(99, 8, nmax=5000, nmin=5000, dense=True)
    wants = [DC.checker(g) for g in gs]
    assert all((w["prv"] >= 0).sum() > 500 for w in wants)
    b = KC.make_batch(gs)
    with poisoned(api, BYTES[1]):
        got = guarded(api, DC.gpu_dag, api, b)
    assert DC.compare_dag(b, gs, wants, got) == []
