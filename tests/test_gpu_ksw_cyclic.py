"""GPU tier of aasm_k_shortest_walks with AASM_KSW_CYCLES (the solver's is_dag = false) on the MI355X: the real reference's
recorded runs (ref_ksw_cyclic.npz), the plain-Python checker on hundreds of mixed cyclic graphs in one call, the host emulation
bit for bit, the real header's dijkstra() where oracle/_ref is built, the guards, and the default mode beside them."""
import ctypes as C

import numpy as np
import pytest

import ksw_cases as KC
import ksw_cyclic_cases as CC

pytestmark = pytest.mark.gpu


def _arena(want):
    return np.array(want["arena"], np.int64).reshape(-1, 10)


def test_gpu_equals_reference_fixture(T):
    api = T.api()
    gs = CC.golden_graphs()
    for g in gs:
        b = KC.make_batch([g])
        assert KC.compare(b, [g], [g["want"]], CC.gpu_run(api, b, g["K"]), g["K"]) == [], g["name"]
    b = KC.make_batch(gs)
    got = CC.gpu_run(api, b, 60)
    assert KC.compare(b, gs, [CC.first_walks(g["want"], 60) for g in gs], got, 60) == []
    z = np.load(CC.GOLDEN)
    for gi, g in enumerate(gs):
        if g["want"]["nd"]:
            assert np.array_equal(CC.arena_words(got, gi), z[f"g{gi}_arena"].reshape(-1, 10)), g["name"]


def test_api_walks_of_the_cycle_graph(T):
    """api.k_shortest_walks(..., cycles=True) on 0 -> 1 -> 2 -> 1, 2 -> 3: the walks 3, 5, 7, 9, ... edges long."""
    api = T.api()
    g = KC.cycle_graph()
    r = api.k_shortest_walks([0, g["n"]], g["rowptr"], g["col"], g["w"], [g["src"]], [g["sink"]], 8, cycles=True)
    assert r["status"][0] == 0 and r["n_found"][0] == 8
    assert list(np.diff(r["walk_off"])) == [3, 5, 7, 9, 11, 13, 15, 17]
    assert list(r["dist"][0, :, 0]) == [3, 5, 7, 9, 11, 13, 15, 17]


@pytest.mark.parametrize("K", [1, 5, 64, 2000])
def test_gpu_equals_checker_mixed_batch(T, K):
    """400 cyclic graphs of the four kinds in one call, each against its own checker run."""
    api = T.api()
    gs = CC.random_graphs(700 + K, 400)
    wants = [CC.checker_run(g, K) for g in gs]
    assert all(w is not None for w in wants)
    b = KC.make_batch(gs)
    got = CC.gpu_run(api, b, K)
    assert KC.compare(b, gs, wants, got, K) == []
    off = np.concatenate([[0], np.cumsum(got["heap_nodes"])])
    for gi, w in enumerate(wants):
        assert np.array_equal(got["hook_arena"][off[gi]:off[gi + 1]], _arena(w)), gi


def test_gpu_equals_emulation_bitwise(T):
    """All output arrays; the guards' graphs (tree guard, walk-edge cap) ride in the batch."""
    api = T.api()
    lib = KC.build_emul()
    gs = CC.random_graphs(78, 148) + [CC.sink_improves()]
    ring = 8192
    gs.append(CC.from_edges(ring, [(i, (i + 1) % ring) for i in range(ring)], [1] * ring, 0, ring - 1))
    b = KC.make_batch(gs)
    rc, want = CC.emul_run(lib, b, 300)
    assert rc == 0
    got = CC.gpu_run(api, b, 300)
    for key in want:
        assert np.array_equal(want[key], got[key]), key
    assert got["status"][148] == CC.E_INVAL and got["status"][149] == CC.E_OVERFLOW and got["n_found"][149] == 300
    assert not got["status"][:148].any()


def test_gpu_magnitude_guard(T):
    api = T.api()
    ring, wq = 8192, (1 << 39) - 1
    gs = [CC.from_edges(ring, [(i, (i + 1) % ring) for i in range(ring)], [[wq, 0, 0, 0, 1]] * ring, 0, ring - 1)] + CC.random_graphs(13, 2)
    b = KC.make_batch(gs)
    got = CC.gpu_run(api, b, 1100, flags=KC.AASM_KSW_TREE | CC.AASM_KSW_CYCLES)
    first_out = next(i for i in range(1100) if (ring - 1 + i * ring) * wq >= 1 << 62)
    assert got["status"][0] == CC.E_OVERFLOW and got["n_found"][0] == first_out
    assert list(got["status"][1:]) == [0, 0]


@pytest.mark.ref
def test_gpu_tree_equals_the_real_headers_dijkstra(T):
    """d5 and best of AASM_KSW_TREE against ref_generic_dijkstra on the reversed graph (:180-185)."""
    ref = T.ref(False)
    if ref is None:
        pytest.skip("oracle/_ref not built (no reference sources on the build machine)")
    api = T.api()
    gs = CC.random_graphs(79, 120) + [g for _, g in CC.hand_graphs()]
    b = KC.make_batch(gs)
    got = CC.gpu_run(api, b, 3, flags=KC.AASM_KSW_TREE | CC.AASM_KSW_CYCLES)
    for gi, g in enumerate(gs):
        n, rp, col, w = g["n"], g["rowptr"], g["col"], g["w"]
        tails = np.repeat(np.arange(n), np.diff(rp))
        order = np.argsort(col, kind="stable")
        rrp = np.zeros(n + 1, np.int64); rrp[1:] = np.cumsum(np.bincount(col, minlength=n))
        rcol, rw = np.ascontiguousarray(tails[order], np.int64), np.ascontiguousarray(w[order].reshape(-1), np.int64)
        d, prv = np.zeros(5 * n, np.int64), np.zeros(n, np.int64)
        ref.ref_generic_dijkstra(C.c_int64(n), T._P(rrp), T._P(rcol), T._P(rw), C.c_int64(g["sink"]), T._P(d), T._P(prv))
        vb = int(b["g_voff"][gi])
        assert np.array_equal(got["d"][vb:vb + n].reshape(-1), d) and np.array_equal(got["best"][vb:vb + n], prv), gi


def test_gpu_default_mode_equals_emulation(T):
    """The flag off: DAGs and a cycle among them, every output array equal to the emulation's."""
    api = T.api()
    lib = KC.build_emul()
    gs = KC.random_graphs(91, 100)
    gs.insert(40, KC.cycle_graph())
    b = KC.make_batch(gs)
    rc, want = KC.emul_run(lib, b, 45)
    assert rc == 0 and want["status"][40] == CC.E_INVAL
    got = KC.gpu_run(api, b, 45)
    for key in want:
        assert np.array_equal(want[key], got[key]), key


def test_gpu_ever_improving_cycle_overflows(T):
    """The bound on dijkstra's pushes ends it (shown first on the CPU tier); its batch neighbours are solved."""
    api = T.api()
    gs = CC.random_graphs(11, 6)
    gs = gs[:3] + [CC.ever_improving()] + gs[3:]
    b = KC.make_batch(gs)
    got = CC.gpu_run(api, b, 20)
    assert got["status"][3] == CC.E_OVERFLOW and got["n_found"][3] == 0
    keep = [i for i in range(len(gs)) if i != 3]
    sub = KC.make_batch([gs[i] for i in keep])
    assert KC.compare(sub, [gs[i] for i in keep], [CC.checker_run(gs[i], 20) for i in keep], CC.gpu_run(api, sub, 20), 20) == []
    assert np.array_equal(got["dist"][keep], CC.gpu_run(api, sub, 20)["dist"])
