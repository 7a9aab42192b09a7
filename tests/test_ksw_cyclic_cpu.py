"""CPU tier of aasm_k_shortest_walks with AASM_KSW_CYCLES (the solver's is_dag = false): the kernels of
alignasm_amd/csrc/aasm_ksw.h with their host driver (1-lane host emulation, tests/host_emul/graphs_emul.cpp) against the real reference's
runs recorded in ref_ksw_cyclic.npz, against the plain-Python checker (tests/ksw_cyclic_checker.py) on random cyclic graphs, and
against a brute force that shares nothing with the heaps; the checker itself against the reference; the guards and the surface."""
import ctypes as C
import heapq
import os
import re

import numpy as np
import pytest

import ksw_cases as KC
import ksw_cyclic_cases as CC
import ksw_cyclic_checker as CK

ROOT = KC.ROOT


@pytest.fixture(scope="module")
def emk():
    return KC.build_emul()


def _arena(want):
    return np.array(want["arena"], np.int64).reshape(-1, 10)


# ---- the product (emulated) against the recorded reference ---------------------------------------------------------------------
def test_emulation_equals_reference_fixture(emk):
    """Every recorded graph alone and all in one batch: distances, every walk as (u, v), best, d, heap roots, node counts."""
    gs = CC.golden_graphs()
    assert len(gs) >= 50
    for g in gs:
        b = KC.make_batch([g])
        rc, got = CC.emul_run(emk, b, g["K"])
        assert rc == 0
        assert KC.compare(b, [g], [g["want"]], got, g["K"]) == [], g["name"]
    b = KC.make_batch(gs)
    rc, got = CC.emul_run(emk, b, 60)
    assert rc == 0 and KC.compare(b, gs, [CC.first_walks(g["want"], 60) for g in gs], got, 60) == []
    # the walks do run through cycles and through the sink
    byname = {g["name"]: g for g in gs}
    assert [len(p) // 2 for p in byname["cycle"]["want"]["paths"][:4]] == [3, 5, 7, 9]
    p = byname["sink_back_to_source"]["want"]["paths"][-1].reshape(-1, 2)
    assert (p[:-1, 1] == byname["sink_back_to_source"]["sink"]).any()


def test_hook_arena_equals_the_checkers_and_the_references(emk):
    """Word for word, {rank, key[5], u, v, left, right} per node (the heaps do not depend on k)."""
    gs = CC.golden_graphs()
    z = np.load(CC.GOLDEN)
    b = KC.make_batch(gs)
    rc, got = CC.emul_run(emk, b, 400)
    assert rc == 0
    for gi, g in enumerate(gs):
        want = CC.checker_run(g, 400)
        assert np.array_equal(CC.arena_words(got, gi), _arena(want)), g["name"]
        assert np.array_equal(_arena(want), z[f"g{gi}_arena"].reshape(-1, 10)), g["name"]


def test_checker_equals_reference_fixture():
    for g in CC.golden_graphs():
        got, want = CC.checker_run(g, g["K"]), g["want"]
        assert got["nd"] == want["nd"], g["name"]
        for key in ("dist", "best", "d", "hcount"):
            assert np.array_equal(got[key], want[key]), (g["name"], key)
        if want["nd"]:
            assert np.array_equal(got["hroot"], want["hroot"]), g["name"]
        assert all(np.array_equal(a, b) for a, b in zip(got["paths"], want["paths"])), g["name"]


def test_dijkstra_tree_differs_from_dag_tree_on_a_tied_dag(emk):
    g = dict((name, g) for name, g in CC.hand_graphs())["dag_tied_trees"]
    b = KC.make_batch([g])
    (rc0, dag), (rc1, cyc) = KC.emul_run(emk, b, 10), CC.emul_run(emk, b, 10)
    assert rc0 == 0 and rc1 == 0
    assert dag["best"][0] == 1 and cyc["best"][0] == 2
    assert np.array_equal(dag["d"], cyc["d"]) and np.array_equal(dag["dist"], cyc["dist"])


# ---- the product (emulated) against independent checks ------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 40, 1000])
def test_emulation_equals_checker_random(emk, K):
    gs = CC.random_graphs(500 + K, 200)
    wants = [CC.checker_run(g, K) for g in gs]
    assert all(w is not None for w in wants)
    b = KC.make_batch(gs)
    rc, got = CC.emul_run(emk, b, K)
    assert rc == 0
    assert KC.compare(b, gs, wants, got, K) == []
    off = np.concatenate([[0], np.cumsum(got["heap_nodes"])])
    for gi, w in enumerate(wants):
        assert np.array_equal(got["hook_arena"][off[gi]:off[gi + 1]], _arena(w)), gi
    assert sum(w["nd"] == K for w in wants) > len(gs) // 3          # cycles: k walks whatever k


def test_emulation_chunks_graphs_by_budget(emk):
    gs = CC.random_graphs(7, 60)
    b = KC.make_batch(gs)
    rc0, a = CC.emul_run(emk, b, 25)
    rc1, c = CC.emul_run(emk, b, 25, budget=2000)
    assert rc0 == 0 and rc1 == 0
    for key in a:
        assert np.array_equal(a[key], c[key]), key


def _k_smallest_walk_weights(g, k):
    """Brute force: the weights of the k lightest walks source -> sink by the k-pop dijkstra (a vertex is expanded the first k
    times it is popped).  Needs weights >= 1, so that only finitely many walks are lighter than any bound."""
    rp, col, w = g["rowptr"], g["col"], g["w"][:, 0]
    pops = [0] * g["n"]
    pq, out = [(0, g["src"])], []
    while pq and len(out) < k:
        dv, v = heapq.heappop(pq)
        if pops[v] >= k:
            continue
        pops[v] += 1
        if v == g["sink"]:
            out.append(dv)
        for e in range(rp[v], rp[v + 1]):
            heapq.heappush(pq, (dv + int(w[e]), int(col[e])))
    return out


@pytest.mark.parametrize("K", [1, 7, 60])
def test_distances_equal_brute_force_on_scalar_graphs(emk, K):
    gs = CC.random_graphs(900 + K, 120, kinds=("scalar1",), nmax=14)
    b = KC.make_batch(gs)
    rc, got = CC.emul_run(emk, b, K)
    assert rc == 0 and not got["status"].any()
    for gi, g in enumerate(gs):
        want = _k_smallest_walk_weights(g, K)
        assert got["n_found"][gi] == len(want), gi
        assert list(got["dist"][gi, :len(want), 0]) == want, gi
        assert list(got["dist"][gi, :len(want), 4]) == [int(x) for x in np.diff(got["walk_off"][gi * K:gi * K + len(want) + 1])], gi


def test_flag_changes_no_distance_on_scalar_dags(emk):
    rng = np.random.default_rng(31)
    gs = []
    for _ in range(80):
        n = int(rng.integers(2, 40))
        rowptr, col, w, order = KC.random_dag(rng, n, int(rng.integers(0, 4 * n + 1)), "scalar")
        a, c = sorted(rng.choice(n, 2, replace=False))
        gs.append(KC.graph(n, rowptr, col, w, int(order[a]), int(order[c])))
    b = KC.make_batch(gs)
    (rc0, dag), (rc1, cyc) = KC.emul_run(emk, b, 50), CC.emul_run(emk, b, 50)
    assert rc0 == 0 and rc1 == 0 and not dag["status"].any() and not cyc["status"].any()
    assert np.array_equal(dag["n_found"], cyc["n_found"]) and dag["n_found"].max() > 10
    assert np.array_equal(dag["dist"][:, :, 0], cyc["dist"][:, :, 0])


# ---- the checker against the reference ---------------------------------------------------------------------------------------
def test_checker_with_the_dag_tree_reproduces_the_recorded_dags():
    gs = KC.golden_graphs()
    assert len(gs) == 11
    for g in gs:
        got, want = CC.checker_run(g, g["K"], tree="dag"), g["want"]
        assert got["nd"] == want["nd"]
        for key in ("dist", "best", "d", "hroot", "hcount"):
            assert np.array_equal(got[key], np.asarray(want[key]).reshape(-1)), key
        assert all(np.array_equal(a, b) for a, b in zip(got["paths"], want["paths"]))


@pytest.mark.ref
def test_checker_dijkstra_equals_the_real_header(T):
    ref = T.ref(False)
    if ref is None:
        pytest.skip("oracle/_ref not built (no reference sources on the build machine)")
    for g in CC.random_graphs(77, 120) + [g for _, g in CC.hand_graphs()]:
        n, rp, col, w = g["n"], g["rowptr"], g["col"], g["w"]
        tails = np.repeat(np.arange(n), np.diff(rp))
        order = np.argsort(col, kind="stable")                       # the reversed graph as :180-183 builds it
        rrp = np.zeros(n + 1, np.int64); rrp[1:] = np.cumsum(np.bincount(col, minlength=n))
        rcol, rw = np.ascontiguousarray(tails[order], np.int64), np.ascontiguousarray(w[order].reshape(-1), np.int64)
        d, prv = np.zeros(5 * n, np.int64), np.zeros(n, np.int64)
        ref.ref_generic_dijkstra(C.c_int64(n), T._P(rrp), T._P(rcol), T._P(rw), C.c_int64(g["sink"]), T._P(d), T._P(prv))
        g_rev = [[(int(rcol[e]), tuple(int(x) for x in rw[5 * e:5 * e + 5]), int(order[e])) for e in range(rrp[v], rrp[v + 1])] for v in range(n)]
        dc, pc, _, _ = CK.dijkstra(g_rev, g["sink"])
        assert [x for t in dc for x in t] == list(d) and pc == list(prv)


# ---- guards ----------------------------------------------------------------------------------------------------------------------
def test_ever_improving_cycle_overflows_and_neighbours_are_solved(emk):
    """dijkstra() of the reference does not return on it; the heap stays at a few entries, so only the bound on pushes ends it."""
    bad = CC.ever_improving()
    with pytest.raises(CK.Overflow):
        CK.solve(bad["n"], bad["rowptr"], bad["col"], bad["w"], bad["src"], bad["sink"], 5, push_limit=64 * (len(bad["col"]) + 2))
    gs = CC.random_graphs(11, 6)
    gs = gs[:3] + [bad] + gs[3:]
    wants = [CC.checker_run(g, 20) if i != 3 else None for i, g in enumerate(gs)]
    b = KC.make_batch(gs)
    rc, got = CC.emul_run(emk, b, 20)
    assert rc == 0
    assert got["status"][3] == CC.E_OVERFLOW and got["n_found"][3] == 0 and got["heap_nodes"][3] == 0
    assert got["walk_off"][3 * 20] == got["walk_off"][4 * 20]
    keep = [i for i in range(len(gs)) if i != 3]
    sub = KC.make_batch([gs[i] for i in keep])
    rc, alone = CC.emul_run(emk, sub, 20)
    assert rc == 0 and KC.compare(sub, [gs[i] for i in keep], [wants[i] for i in keep], alone, 20) == []
    assert np.array_equal(got["dist"][keep], alone["dist"]) and np.array_equal(got["n_found"][keep], alone["n_found"])


def test_best_cycle_is_invalid(emk):
    """A witness of the tree guard: the sink's own distance improves round a cycle (identity -> mapq ratio 2/2), so best[] is the
    cycle 0 -> 1 -> 0 and no tree.  The checker, like the reference, finds no end of the BFS over tree[]."""
    bad = CC.sink_improves()
    assert CC.checker_run(bad, 5) is None
    gs = CC.random_graphs(12, 4) + [bad]
    b = KC.make_batch(gs)
    rc, got = CC.emul_run(emk, b, 9)
    assert rc == 0
    assert KC.compare(b, gs, [CC.checker_run(g, 9) for g in gs], got, 9) == []          # None: AASM_E_INVAL and no walks
    vb = int(b["g_voff"][4])
    assert list(got["best"][vb:vb + 2]) == [1, 0]                   # as dijkstra left it


RING = 8192


def _ring(w):
    """0 -> 1 -> ... -> RING - 1 -> 0, source 0, sink RING - 1: walk i goes round i times."""
    return CC.from_edges(RING, [(i, (i + 1) % RING) for i in range(RING)], [w] * RING, 0, RING - 1)


def test_magnitude_guard(emk):
    wq = (1 << 39) - 1
    gs = [_ring([wq, 0, 0, 0, 1])] + CC.random_graphs(13, 2)
    b = KC.make_batch(gs)
    rc, got = CC.emul_run(emk, b, 1100, flags=KC.AASM_KSW_TREE | CC.AASM_KSW_CYCLES)
    assert rc == 0
    first_out = next(i for i in range(1100) if (RING - 1 + i * RING) * wq >= 1 << 62)
    assert got["status"][0] == CC.E_OVERFLOW and got["n_found"][0] == first_out
    assert list(got["dist"][0, first_out - 1]) == [(RING - 1 + (first_out - 1) * RING) * wq, 0, 0, 0, RING - 1 + (first_out - 1) * RING]
    assert not got["dist"][0, first_out:].any()
    assert list(got["status"][1:]) == [0, 0]


def test_walk_edge_cap(emk):
    gs = [_ring(1)] + CC.random_graphs(14, 2)
    K = 300
    total = sum(RING - 1 + i * RING for i in range(K))
    assert total > 1 << 28
    b = KC.make_batch(gs)
    rc, got = CC.emul_run(emk, b, K)
    assert rc == 0
    assert got["status"][0] == CC.E_OVERFLOW and got["n_found"][0] == K
    assert list(got["dist"][0, :, 0]) == [RING - 1 + i * RING for i in range(K)]
    assert (np.diff(got["walk_off"][:K + 1]) == 0).all()
    assert list(got["status"][1:]) == [0, 0]
    wants = [CC.checker_run(g, K) for g in gs[1:]]
    sub = KC.make_batch(gs[1:])
    rc, alone = CC.emul_run(emk, sub, K)
    assert rc == 0 and KC.compare(sub, gs[1:], wants, alone, K) == []
    assert np.array_equal(got["walk_edges"] - int(b["rowptr"][RING]), alone["walk_edges"])
    # under the cap the same ring gives its walks
    rc, few = CC.emul_run(emk, KC.make_batch([_ring(1)]), 5)
    assert rc == 0 and few["status"][0] == 0 and list(np.diff(few["walk_off"])) == [RING - 1 + i * RING for i in range(5)]


# ---- surface -----------------------------------------------------------------------------------------------------------------------
def test_header_and_abi_agree_on_the_flag(T):
    from alignasm_amd import _abi
    src = open(os.path.join(ROOT, "include", "alignasm_amd.h")).read()
    assert int(re.search(r"#define AASM_KSW_CYCLES\s+(0x[0-9A-Fa-f]+)", src).group(1), 16) == _abi.AASM_KSW_CYCLES == 0x4
    assert re.search(r"#define AASM_ABI_VERSION 3\b", src)
    assert C.sizeof(_abi.KswOut) == 2 * 8 + 10 * 8
    import inspect
    assert inspect.signature(T.api().k_shortest_walks).parameters["cycles"].default is False


def test_without_the_flag_a_cycle_is_still_invalid(emk):
    b = KC.make_batch([KC.cycle_graph()])
    rc, got = KC.emul_run(emk, b, 5)
    assert rc == 0 and got["status"][0] == CC.E_INVAL and got["n_found"][0] == 0
    rc, got = CC.emul_run(emk, b, 5)
    assert rc == 0 and got["status"][0] == 0 and list(np.diff(got["walk_off"])) == [3, 5, 7, 9, 11]


def test_no_device_gives_nodevice(T):
    api = T.api()
    if api.device_count() > 0:
        pytest.skip("a GPU is present; the no-device path is exercised on CPU-only boxes")
    with pytest.raises(api.AlignasmError) as ei:
        CC.gpu_run(api, KC.make_batch([KC.cycle_graph()]), 3)
    assert ei.value.code == -2          # AASM_E_NODEVICE
