"""GPU tier of aasm_sssp_bellman_ford and of aasm_k_shortest_walks with AASM_KSW_NEGATIVE, under poisoned working memory as
tests/test_gpu_poison.py: the 64-lane list walk of bf_spfa (alignasm_amd/csrc/aasm_sssp.h) - the ballot over a chunk, the commits in
lane order, the re-evaluation behind a self-loop - exists only on the card; the one-lane emulation of tests/test_bf_cpu.py walks edge
by edge.  Every comparison is exact: against the real reference's recorded runs (ref_bellman_ford.npz), the plain-Python checker,
and, on contigs whose records run past the query's end, the pipeline's own K6-K8."""
import numpy as np
import pytest

import bf_cases as BC
import ksw_cases as KC
import ksw_cyclic_cases as CC
from poison_testlib import BYTE_IDS, BYTES, cached, guarded, poisoned

pytestmark = pytest.mark.gpu

both_bytes = pytest.mark.parametrize("byte", BYTES, ids=BYTE_IDS)


def _random():
    gs = cached("bf random", lambda: BC.random_graphs(4712, 160))
    return gs, cached("bf random checker", lambda: [BC.checker_bf(g)[0] for g in gs])


@both_bytes
def test_bellman_ford_on_the_whole_case_set(T, byte):
    """Every recorded graph and fresh random ones in one call: d, prev, status, cycle against the reference's runs and the checker;
    then the hub graphs alone, each a batch of its own."""
    api = T.api()
    gold = BC.golden_graphs()
    rand, wants = _random()
    gs, ws = gold + rand, [g["bf"] for g in gold] + wants
    with poisoned(api, byte):
        b = KC.make_batch(gs)
        assert BC.compare_bf(b, gs, ws, guarded(api, BC.gpu_bf, api, b)) == []
        hubs = [g for g in gold if g["name"].startswith(("hub_", "fan_in_"))]
        assert len(hubs) == 16
        b = KC.make_batch(hubs)
        assert BC.compare_bf(b, hubs, [g["bf"] for g in hubs], guarded(api, BC.gpu_bf, api, b)) == []
        for g in hubs:
            b = KC.make_batch([g])
            assert BC.compare_bf(b, [g], [g["bf"]], guarded(api, BC.gpu_bf, api, b)) == [], g["name"]


@both_bytes
def test_k_walks_with_the_bellman_ford_tree(T, byte):
    """negative=True, cycles=True: all recorded graphs in one batch at k = 60, every tenth at k = 400, arena included."""
    api = T.api()
    gold = BC.golden_graphs()
    with poisoned(api, byte):
        b = KC.make_batch(gold)
        got = guarded(api, BC.gpu_ksw, api, b, 60, BC.NEG_CYC)
        assert KC.compare(b, gold, [BC.first_walks(g["want"], 60) for g in gold], got, 60) == []
        for gi, g in enumerate(gold):
            vb = int(b["g_voff"][gi])
            if g["want"] is None:
                assert (got["d"][vb:vb + g["n"]] == [-1, -1, -1, -1, 0]).all() and (got["best"][vb:vb + g["n"]] == -1).all(), g["name"]
            else:
                assert np.array_equal(CC.arena_words(got, gi), g["want"]["arena"]), g["name"]
        # every tenth random graph is recorded at k = 400; of the others, those whose recorded run is complete below 60 walks
        tenth = [g for g in gold if g["K"] == 400] + [g for g in gold[::10] if g["K"] != 400 and (g["want"] is None or g["want"]["nd"] < 60)]
        assert sum(g["K"] == 400 for g in tenth) == 4
        b = KC.make_batch(tenth)
        got = guarded(api, BC.gpu_ksw, api, b, 400, BC.NEG_CYC)
        assert KC.compare(b, tenth, [BC.first_walks(g["want"], 400) for g in tenth], got, 400) == []
        assert max(int(x) for x in got["n_found"]) == 400


@both_bytes
def test_negative_dags_in_the_dag_mode(T, byte):
    api = T.api()
    gs = [g for g in BC.golden_graphs() if g["want_dag"] is not None]
    assert len(gs) == 10
    with poisoned(api, byte):
        b = KC.make_batch(gs)
        got = guarded(api, BC.gpu_ksw, api, b, 60, BC.NEG)
        assert KC.compare(b, gs, [BC.first_walks(g["want_dag"], 60) for g in gs], got, 60) == []
        for gi, g in enumerate(gs):
            assert np.array_equal(CC.arena_words(got, gi), g["want_dag"]["arena"]), g["name"]


def test_overhang_contigs_equal_the_pipeline(T):
    """Contig DAGs with negative dest edges and walk sums: n_found, dist5, d5, best, heap_nodes equal the pipeline's K6-K8 of the same
    solve; without the flag the same batch is refused."""
    api = T.api()
    K = 16
    seen_negative = seen_negative_walk = False
    for batch, want in BC.overhang_batches(T, K):
        w = batch["w"]
        seen_negative |= bool((w[:, 0] + w[:, 1] < 0).any())
        args = (batch["g_voff"], batch["rowptr"], batch["col"], w, batch["src"], batch["sink"], K)
        with poisoned(api, BYTES[0]):
            got = guarded(api, api.k_shortest_walks, *args, walks=True, tree=True, negative=True)
        assert KC.compare_pipeline(batch, want, got, K) == []
        seen_negative_walk |= any((kd[:, 0] + kd[:, 1] < 0).any() for kd in want["kd"] if len(kd))
        if (w[:, 0] + w[:, 1] < 0).any():
            with pytest.raises(api.AlignasmError) as ei:
                api.k_shortest_walks(*args)
            assert ei.value.code == BC.E_OVERFLOW
    assert seen_negative and seen_negative_walk


@both_bytes
def test_negative_cycles_among_solvable_graphs(T, byte):
    """A batch that mixes graphs with a negative cycle and solvable ones, one after the other: the statuses sit on the right graphs
    and the others are solved as they are alone."""
    api = T.api()
    gold = BC.golden_graphs()
    bad = [g for g in gold if g["bf"]["status"] == 1]
    good = [g for g in gold if g["bf"]["status"] == 0]
    gs = [x for pair in zip(bad, good) for x in pair]
    assert len(gs) >= 30
    with poisoned(api, byte):
        b = KC.make_batch(gs)
        got = guarded(api, BC.gpu_bf, api, b)
        assert list(got["status"]) == [1, 0] * (len(gs) // 2)
        assert BC.compare_bf(b, gs, [g["bf"] for g in gs], got) == []
        kw = guarded(api, BC.gpu_ksw, api, b, 60, BC.NEG_CYC)
        assert KC.compare(b, gs, [BC.first_walks(g["want"], 60) for g in gs], kw, 60) == []
        assert all(kw["status"][i] == BC.E_INVAL for i in range(0, len(gs), 2))
        sub = KC.make_batch(gs[1::2])
        alone = guarded(api, BC.gpu_bf, api, sub)
        vt = np.concatenate([np.arange(b["g_voff"][i], b["g_voff"][i + 1]) for i in range(1, len(gs), 2)])
        assert np.array_equal(got["d"][vt], alone["d"]) and np.array_equal(got["prev"][vt], alone["prev"])
