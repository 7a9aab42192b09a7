"""CPU tier of aasm_sssp_bellman_ford and of aasm_k_shortest_walks with AASM_KSW_NEGATIVE: the kernels of alignasm_amd/csrc/aasm_sssp.h
and aasm_ksw.h with their host drivers (1-lane host emulation, tests/host_emul/graphs_emul.cpp) against the real reference's runs recorded
in ref_bellman_ford.npz, against the plain-Python checker (tests/bf_checker.py) on graphs the file does not hold, and against a
brute-force relaxation; the argument checks, the queue's room, the sanitizer program, and the refactored AASM_KSW_CYCLES tree kernel
against its own recorded runs."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import bf_cases as BC
import bf_checker as BK
import ksw_cases as KC
import ksw_cyclic_cases as CC

N_RECORDED = 66


@pytest.fixture(scope="module")
def built():
    return KC.build_emul(san=True)


@pytest.fixture(scope="module")
def emk(built):
    return built[0]


def _ksw_ok(b, gs, wants, got, k):
    """KC.compare, the arena word for word, and max / -1 in d / best of the graphs that come back AASM_E_INVAL."""
    bad = KC.compare(b, gs, wants, got, k)
    for gi, (g, w) in enumerate(zip(gs, wants)):
        vb = int(b["g_voff"][gi])
        if w is None:
            if not (got["d"][vb:vb + g["n"]] == np.array(BK.MAX)).all() or not (got["best"][vb:vb + g["n"]] == -1).all():
                bad.append((gi, "d / best of a graph without a distance vector"))
        elif not np.array_equal(CC.arena_words(got, gi), np.array(w["arena"], np.int64).reshape(-1, 10)):
            bad.append((gi, "arena"))
    return bad


# ---- the product (emulated) against the recorded reference ---------------------------------------------------------------------
def test_bellman_ford_equals_reference_fixture(emk):
    """Every recorded graph in one batch and one by one: d, prv, status, cycle."""
    gs = BC.golden_graphs()
    assert len(gs) == N_RECORDED == len(BC.cases())
    b = KC.make_batch(gs)
    rc, got = BC.emul_bf(emk, b)
    assert rc == 0 and BC.compare_bf(b, gs, [g["bf"] for g in gs], got) == []
    for g in gs:
        b = KC.make_batch([g])
        rc, got = BC.emul_bf(emk, b)
        assert rc == 0 and BC.compare_bf(b, [g], [g["bf"]], got) == [], g["name"]
    st = [g["bf"]["status"] for g in gs]
    assert st.count(1) >= 15 and st.count(0) >= 30
    byname = {g["name"]: g for g in gs}
    assert list(byname["negative_self_loop_n1"]["bf"]["cycle"]) == [0, 0]
    assert byname["diamond_tied_negative"]["bf"]["prv"][3] == 2      # the first of two equal offers stays
    assert byname["ever_improving_ratio"]["bf"]["status"] == 1       # no negative score sum, and still round n relaxes


def test_recorded_graphs_are_the_cases():
    for g, (name, c, K) in zip(BC.golden_graphs(), BC.cases()):
        assert g["name"] == name and g["K"] == K and g["src"] == c["src"] and g["sink"] == c["sink"]
        assert np.array_equal(g["rowptr"], c["rowptr"]) and np.array_equal(g["col"], c["col"]) and np.array_equal(g["w"], c["w"])


def test_k_walks_equal_reference_fixture(emk):
    """AASM_KSW_CYCLES | AASM_KSW_NEGATIVE: distances, walks as (u, v), best, d5, heap roots and the arena words; AASM_E_INVAL, no
    walks and max / -1 where bellman_ford from the sink reports a cycle."""
    gs = BC.golden_graphs()
    for g in gs:
        b = KC.make_batch([g])
        rc, got = KC.emul_run(emk, b, g["K"], BC.NEG_CYC)
        assert rc == 0 and _ksw_ok(b, [g], [g["want"]], got, g["K"]) == [], g["name"]
    b = KC.make_batch(gs)
    rc, got = KC.emul_run(emk, b, 60, BC.NEG_CYC)
    assert rc == 0
    wants = [BC.first_walks(g["want"], 60) for g in gs]
    assert KC.compare(b, gs, wants, got, 60) == []
    assert sum(w is None for w in wants) >= 15 and sum(w is not None and w["nd"] == 60 for w in wants) >= 10


def test_negative_dags_equal_reference_fixture(emk):
    """AASM_KSW_NEGATIVE alone: the DAG relaxation on negative sums, against the solver with is_dag = true."""
    gs = [g for g in BC.golden_graphs() if g["want_dag"] is not None]
    assert len(gs) == 10
    assert any((g["w"][:, 0] + g["w"][:, 1] < 0).any() for g in gs)
    for g in gs:
        b = KC.make_batch([g])
        rc, got = KC.emul_run(emk, b, g["K"], BC.NEG)
        assert rc == 0 and _ksw_ok(b, [g], [g["want_dag"]], got, g["K"]) == [], g["name"]
    b = KC.make_batch(gs)
    rc, got = KC.emul_run(emk, b, 60, BC.NEG)
    assert rc == 0 and KC.compare(b, gs, [BC.first_walks(g["want_dag"], 60) for g in gs], got, 60) == []


def test_checker_equals_reference_fixture():
    for g in BC.golden_graphs():
        got, _ = BC.checker_bf(g)
        for key in ("status", "d", "prv", "cycle"):
            assert np.array_equal(got[key], g["bf"][key]), (g["name"], key)
        got, want = BC.checker_ksw(g, g["K"]), g["want"]
        assert (got is None) == (want is None), g["name"]
        if want is not None:
            assert got["nd"] == want["nd"], g["name"]
            for key in ("dist", "best", "d", "hcount"):
                assert np.array_equal(got[key], want[key]), (g["name"], key)
            assert all(np.array_equal(a, b) for a, b in zip(got["paths"], want["paths"])), g["name"]


# ---- the product (emulated) against independent checks ------------------------------------------------------------------------
def test_bellman_ford_equals_checker_random(emk):
    gs = BC.random_graphs(4711, 240)
    wants = [BC.checker_bf(g)[0] for g in gs]
    b = KC.make_batch(gs)
    rc, got = BC.emul_bf(emk, b)
    assert rc == 0 and BC.compare_bf(b, gs, wants, got) == []
    assert sum(w["status"] == 1 for w in wants) > 40 and sum(w["status"] == 0 for w in wants) > 100


@pytest.mark.parametrize("K", [1, 7, 120])
def test_k_walks_equal_checker_random(emk, K):
    gs = BC.random_graphs(900 + K, 120)
    wants = [BC.checker_ksw(g, K) for g in gs]
    b = KC.make_batch(gs)
    rc, got = KC.emul_run(emk, b, K, BC.NEG_CYC)
    assert rc == 0 and _ksw_ok(b, gs, wants, got, K) == []
    assert sum(w is None for w in wants) > 10 and sum(w is not None and w["nd"] == K for w in wants) > 20


def _brute_force(g):
    """V - 1 rounds of relaxing every edge, on the score alone: the distance, or None for unreachable."""
    n, rp, col, w = g["n"], g["rowptr"], g["col"], g["w"][:, 0]
    d = [None] * n
    d[g["src"]] = 0
    for _ in range(n - 1):
        for u in range(n):
            if d[u] is not None:
                for e in range(rp[u], rp[u + 1]):
                    v = int(col[e])
                    if d[v] is None or d[u] + int(w[e]) < d[v]:
                        d[v] = d[u] + int(w[e])
    return d


def test_distances_equal_brute_force_on_scalar_graphs(emk):
    rng = np.random.default_rng(5)
    gs = []
    for _ in range(150):
        n = int(rng.integers(2, 25))
        rowptr, col, w = CC.random_cyclic(rng, n, int(rng.integers(n, 4 * n)), "scalar1")
        p = rng.integers(0, 40, n)
        w[:, 0] += p[np.repeat(np.arange(n), np.diff(rowptr))] - p[col]      # negative edges, every cycle's sum >= 1
        gs.append(KC.graph(n, rowptr, col, w, int(rng.integers(0, n)), 0))
    assert any((g["w"][:, 0] < 0).any() for g in gs)
    b = KC.make_batch(gs)
    rc, got = BC.emul_bf(emk, b)
    assert rc == 0 and not got["status"].any()
    for gi, g in enumerate(gs):
        vb = int(b["g_voff"][gi])
        for v, want in enumerate(_brute_force(g)):
            d = got["d"][vb + v]
            assert (list(d) == list(BK.MAX)) if want is None else (d[0] == want and d[1] == 0), (gi, v)


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def _one_edge(wq, wr=0):
    return KC.make_batch([KC.graph(2, [0, 1, 1], [1], [[wq, wr, 0, 0, 1]], 0, 1)])


def test_argument_checks(emk):
    neg = _one_edge(-3, 2)
    assert KC.emul_run(emk, neg, 3, KC.ALL)[0] == BC.E_OVERFLOW                       # without the flag a negative sum is refused as ever
    assert KC.emul_run(emk, neg, 3, KC.ALL | CC.AASM_KSW_CYCLES)[0] == BC.E_OVERFLOW
    rc, got = KC.emul_run(emk, neg, 3, BC.NEG)
    assert rc == 0 and list(got["dist"][0, 0]) == [-3, 2, 0, 0, 1]
    assert KC.emul_run(emk, neg, 3, BC.NEG_CYC)[0] == 0 and BC.emul_bf(emk, neg)[0] == 0
    for big in (_one_edge(1 << 39), _one_edge(-(1 << 39) - 1), _one_edge(0, 1 << 39)):
        assert KC.emul_run(emk, big, 3, BC.NEG)[0] == BC.E_OVERFLOW and KC.emul_run(emk, big, 3, BC.NEG_CYC)[0] == BC.E_OVERFLOW
        assert BC.emul_bf(emk, big)[0] == BC.E_OVERFLOW
    edge = _one_edge(-(1 << 39), (1 << 39) - 1)                                       # the domain's corner is inside
    assert BC.emul_bf(emk, edge)[0] == 0
    assert KC.emul_run(emk, neg, 3, BC.NEG | 0x10)[0] == BC.E_INVAL and KC.emul_run(emk, neg, 3, 0x40)[0] == BC.E_INVAL
    for name in ("status", "cycle_off", "cycle", "d5", "prev", "w5"):
        assert BC.emul_bf(emk, neg, raw={name: None})[0] == BC.E_INVAL, name
    bad = dict(neg, src=np.array([2], np.int32))
    assert BC.emul_bf(emk, bad)[0] == BC.E_INVAL


# ---- the queue's room ---------------------------------------------------------------------------------------------------------------
def test_queue_room_is_never_reached(emk):
    gs = BC.golden_graphs() + BC.random_graphs(4711, 240) + [g for _, g in CC.hand_graphs()] + CC.random_graphs(3, 80)
    b = KC.make_batch(gs)
    rc, got = BC.emul_bf(emk, b)
    assert rc == 0 and (got["status"] >= 0).all()
    for gi, g in enumerate(gs):
        E = len(g["col"])
        assert emk.emk_bf_queue_room(E) == 2 * (E + 2)
        assert 1 <= got["qhigh"][gi] <= 2 * E + 1 < 2 * (E + 2), (gi, int(got["qhigh"][gi]), E)
        want, high = BC.checker_bf(g)
        if want["status"] == 0:
            assert got["qhigh"][gi] == high, gi
    assert got["qhigh"].max() > 40


# ---- the sanitizer program ----------------------------------------------------------------------------------------------------------
def test_sanitizer_program_runs_clean_and_agrees(built, tmp_path):
    emk, prog = built
    gs = BC.golden_graphs() + BC.random_graphs(77, 40)
    b = KC.make_batch(gs)
    K = 25
    words = [len(gs), K, BC.NEG_CYC, int(b["g_voff"][-1]), len(b["col"])]
    raw = np.concatenate([np.array(words, np.int64), b["g_voff"], b["rowptr"], b["col"].astype(np.int64), b["w"].reshape(-1).astype(np.int64),
                          b["src"].astype(np.int64), b["sink"].astype(np.int64)])
    raw.tofile(tmp_path / "in.bin")
    r = subprocess.run([prog, "bf", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.fromfile(tmp_path / "out.bin", np.int64)
    rc, bf = BC.emul_bf(emk, b)
    rc2, kw = KC.emul_run(emk, b, K, BC.NEG_CYC)
    assert rc == 0 and rc2 == 0
    at = 0
    for gi, g in enumerate(gs):
        vb, n = int(b["g_voff"][gi]), g["n"]
        st, clen, nf, kst = (int(x) for x in out[at:at + 4]); at += 4
        assert st == bf["status"][gi] and clen == len(bf["cycles"][gi]), gi
        assert np.array_equal(out[at:at + 5 * n], bf["d"][vb:vb + n].reshape(-1)); at += 5 * n
        assert np.array_equal(out[at:at + n], bf["prev"][vb:vb + n]); at += n
        assert np.array_equal(out[at:at + clen], bf["cycles"][gi]); at += clen
        if st == 0:                                                  # (the program runs k-walks where the source's run found no cycle)
            assert nf == kw["n_found"][gi] and kst == kw["status"][gi], gi
            assert np.array_equal(out[at:at + 5 * nf], kw["dist"][gi, :nf].reshape(-1)), gi
        at += 5 * nf
    assert at == len(out)


# ---- the tail the two tree kernels share ----------------------------------------------------------------------------------------
def test_cycles_without_negative_is_still_word_for_word(emk):
    """AASM_KSW_CYCLES alone on its own recorded runs (ref_ksw_cyclic.npz): what the refactored kb_ksw_tree_cyc is held to."""
    gs = CC.golden_graphs()
    z = np.load(CC.GOLDEN)
    b = KC.make_batch(gs)
    rc, got = CC.emul_run(emk, b, 60)
    assert rc == 0 and KC.compare(b, gs, [CC.first_walks(g["want"], 60) for g in gs], got, 60) == []
    rc, got = CC.emul_run(emk, b, 400)
    assert rc == 0
    for gi, g in enumerate(gs):
        assert np.array_equal(CC.arena_words(got, gi), z[f"g{gi}_arena"].reshape(-1, 10)), g["name"]
    # on weights dijkstra() accepts the two trees give the same distances (the trees themselves may differ among ties)
    rc, neg = KC.emul_run(emk, b, 60, BC.NEG_CYC)
    assert rc == 0
    for gi, g in enumerate(gs):
        if neg["status"][gi] == 0 and got["status"][gi] == 0:
            nf = int(neg["n_found"][gi])
            assert nf == min(60, got["n_found"][gi]) and np.array_equal(neg["dist"][gi, :nf, :2].sum(1), got["dist"][gi, :nf, :2].sum(1)), g["name"]


# ---- surface -----------------------------------------------------------------------------------------------------------------------
def test_header_and_abi_agree(T):
    from alignasm_amd import _abi
    src = open(os.path.join(KC.ROOT, "include", "alignasm_amd.h")).read()
    assert int(re.search(r"#define AASM_KSW_NEGATIVE\s+(0x[0-9A-Fa-f]+)", src).group(1), 16) == _abi.AASM_KSW_NEGATIVE == 0x8
    assert re.search(r"#define AASM_ABI_VERSION 3\b", src)
    assert re.search(r"int\s+aasm_sssp_bellman_ford\(int64_t n_graphs, const int64_t \*g_voff, const int64_t \*rowptr, const int32_t \*col, "
                     r"const int64_t \*w5,\s+const int32_t \*src, int64_t \*d5, int32_t \*prev, int32_t \*status, int64_t \*cycle_off, "
                     r"int32_t \*cycle, int device\);", src)
    api = T.api()
    assert inspect.signature(api.k_shortest_walks).parameters["negative"].default is False
    assert list(inspect.signature(api.sssp_bellman_ford).parameters) == ["g_voff", "rowptr", "col", "w5", "src", "device"]
    assert hasattr(api.LIB, "aasm_sssp_bellman_ford")
