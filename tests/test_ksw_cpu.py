"""CPU tier of aasm_k_shortest_walks (row ★K): the C-ABI surface and its argument checks through the product library, and
the kernels of alignasm_amd/csrc/aasm_ksw.h with their host driver (1-lane host emulation, tests/host_emul/graphs_emul.cpp) against the
real reference's numbers in ref_algos.npz and against the oracle's restatement on random DAGs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ksw_cases as KC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emk():
    return KC.build_emul()


def test_header_declares_the_entry_and_abi_stays_3(T):
    src = open(os.path.join(ROOT, "include", "alignasm_amd.h")).read()
    assert re.search(r"int\s+aasm_k_shortest_walks\s*\(", src) and re.search(r"void\s+aasm_ksw_free\s*\(", src)
    assert re.search(r"#define AASM_ABI_VERSION 3\b", src)
    api = T.api()
    assert "aasm_k_shortest_walks" in api.EXPORTED and "aasm_ksw_free" in api.EXPORTED
    assert hasattr(api.LIB, "aasm_k_shortest_walks") and hasattr(api.LIB, "aasm_ksw_free")
    for name, val in (("AASM_KSW_WALKS", 0x1), ("AASM_KSW_TREE", 0x2), ("AASM_KSW_HOOK_ARENA", 0x100)):
        assert int(re.search(r"#define %s\s+(0x[0-9A-Fa-f]+)" % name, src).group(1), 16) == val


def test_abi_struct_size():
    from alignasm_amd import _abi
    assert C.sizeof(_abi.KswOut) == 2 * 8 + 10 * 8
    assert [f for f, _ in _abi.KswOut._fields_] == ["n_graphs", "k", "n_found", "dist5", "walk_off", "walk_edges", "d5", "best",
                                                    "heap_nodes", "status", "hook_arena", "hook_hroot"]


def _small():
    return KC.make_batch([KC.graph(3, [0, 2, 3, 3], [1, 2, 2], [1, 5, 1], 0, 2), KC.graph(2, [0, 1, 1], [1], [0], 0, 1)])


def test_no_device_gives_nodevice(T):
    api = T.api()
    if api.device_count() > 0:
        pytest.skip("a GPU is present; the no-device path is exercised on CPU-only boxes")
    b = _small()
    with pytest.raises(api.AlignasmError) as ei:
        KC.gpu_run(api, b, 3)
    assert ei.value.code == -2          # AASM_E_NODEVICE


@pytest.mark.parametrize("what", ["voff0", "voff_empty", "rowptr_down", "col_out", "anom", "qnz", "qtot", "score_sum", "score_big",
                                  "source", "sink", "k0", "k_big"])
def test_argument_checks(T, what):
    """Checked on the host before any device is touched, so they hold on every machine."""
    api = T.api()
    b = _small()
    k, code = 3, -1
    if what == "voff0":
        b["g_voff"] = b["g_voff"] + 1
    elif what == "voff_empty":
        b["g_voff"][1] = b["g_voff"][0]
    elif what == "rowptr_down":
        b["rowptr"][1], b["rowptr"][2] = b["rowptr"][2], b["rowptr"][1]
    elif what == "col_out":
        b["col"][3] = 2                 # graph 1 has vertices 0, 1
    elif what in ("anom", "qnz", "qtot"):
        b["w"][1, {"anom": 2, "qnz": 3, "qtot": 4}[what]] = 3; code = -5
    elif what == "score_sum":
        b["w"][1, 0] = -7; code = -5
    elif what == "score_big":
        b["w"][1, 0] = 1 << 39; code = -5
    elif what == "source":
        b["src"][1] = 2
    elif what == "sink":
        b["sink"][0] = -1
    elif what == "k0":
        k = 0
    elif what == "k_big":
        k = (1 << 24) + 1
    with pytest.raises(api.AlignasmError) as ei:
        KC.gpu_run(api, b, k)
    assert ei.value.code == code


def test_emulation_equals_reference_golden(emk):
    """The 11 DAGs recorded from the real header (monotonic allocator): distances, every walk mapped to (u, v), best, d, heap
    roots and node counts - graph by graph, and all in one batch."""
    gs = KC.golden_graphs()
    for g in gs:
        b = KC.make_batch([g])
        rc, got = KC.emul_run(emk, b, g["K"])
        assert rc == 0
        assert KC.compare(b, [g], [g["want"]], got, g["K"]) == []
    b = KC.make_batch(gs)
    rc, got = KC.emul_run(emk, b, 300)
    assert rc == 0 and KC.compare(b, gs, [g["want"] for g in gs], got, 300) == []


@pytest.mark.parametrize("K", [1, 3, 40, 1000])
def test_emulation_equals_oracle_random(T, emk, K):
    gs = KC.random_graphs(100 + K, 90)
    wants = [KC.checker_run(T, T.oracle(), "oracle_", g, K) for g in gs]
    b = KC.make_batch(gs)
    rc, got = KC.emul_run(emk, b, K)
    assert rc == 0
    assert KC.compare(b, gs, wants, got, K) == []
    if K == 1000:                       # more than every graph's walks: n_found is the number of walks
        assert all(w["nd"] < K for w in wants)


def test_emulation_chunks_graphs_by_budget(T, emk):
    """A small memory budget splits the batch into chunks of graphs; nothing changes."""
    gs = KC.random_graphs(7, 60)
    b = KC.make_batch(gs)
    rc0, a = KC.emul_run(emk, b, 25)
    rc1, c = KC.emul_run(emk, b, 25, budget=2000)
    assert rc0 == 0 and rc1 == 0
    for key in a:
        assert np.array_equal(a[key], c[key]), key


def test_cycle_is_reported_and_batch_neighbours_solved(T, emk):
    gs = KC.random_graphs(11, 6)
    gs = gs[:3] + [KC.cycle_graph()] + gs[3:]
    wants = [None if i == 3 else KC.checker_run(T, T.oracle(), "oracle_", g, 20) for i, g in enumerate(gs)]
    b = KC.make_batch(gs)
    rc, got = KC.emul_run(emk, b, 20)
    assert rc == 0
    assert got["status"][3] == -1 and got["n_found"][3] == 0
    assert KC.compare(b, gs, wants, got, 20) == []


def test_scalar_weights_order_as_scalars(emk):
    """w given as [E]: (w, 0, 0, 0, 1) per edge, whose CALC_SUM order is the scalar order; qtot counts a walk's edges."""
    rowptr, col, w = np.array([0, 3, 5, 6, 6]), np.array([1, 2, 3, 3, 3, 3]), np.array([4, 1, 1, 2, 2, 0])
    b = KC.make_batch([KC.graph(4, rowptr, col, w, 0, 3)])
    b["w"] = w                          # [E]: ksw_inputs widens it
    rc, got = KC.emul_run(emk, b, 10)
    assert rc == 0 and got["n_found"][0] == 4          # 0-3, 0-2-3, and 0-1-3 over either parallel edge
    assert list(got["dist"][0, :4, 0]) == [1, 1, 6, 6]
    wo, we = got["walk_off"], got["walk_edges"]
    for i in range(4):
        e = we[wo[i]:wo[i + 1]]
        assert w[e].sum() == got["dist"][0, i, 0] and len(e) == got["dist"][0, i, 4]
    assert sorted(tuple(we[wo[i]:wo[i + 1]]) for i in (2, 3)) == [(0, 3), (0, 4)]


def test_emulation_heap_arena_equals_reference_header(T, emk):
    """The heap arena word for word against ref_generic_heap of the real header (monotonic allocator), where oracle/_ref is built."""
    ref = T.ref(True)
    if ref is None:
        pytest.skip("oracle/_ref not built (no reference sources on the build machine)")
    gs = KC.golden_graphs()[:6] + KC.random_graphs(5, 12)
    b = KC.make_batch(gs)
    rc, got = KC.emul_run(emk, b, 50)
    assert rc == 0
    off = np.concatenate([[0], np.cumsum(got["heap_nodes"])])
    for gi, g in enumerate(gs):
        w = KC.checker_run(T, ref, "ref_", g, 50)
        if w["nd"] == 0:
            continue
        nodes = int(w["hcount"][0])
        assert got["heap_nodes"][gi] == nodes
        arena = np.zeros(10 * max(nodes, 1), np.int64)
        ref.ref_generic_heap(arena.ctypes.data_as(T._i64p), T.C.c_int64(nodes))
        assert np.array_equal(got["hook_arena"][off[gi]:off[gi + 1]].reshape(-1), arena[:10 * nodes]), gi
