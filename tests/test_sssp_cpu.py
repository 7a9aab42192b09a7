"""CPU tier of the generic SSSP entries, aasm_sssp_dijkstra (row ★J) and aasm_sssp_dial (row K5): the kernels of
alignasm_amd/csrc/aasm_sssp.h with their host drivers (1-lane host emulation, tests/host_emul/graphs_emul.cpp) against the recorded reference
vectors (ref_algos.npz, ref_dial.npz) and the oracle, and the argument checks of all three graph entries through the product
library, which run before any device is touched."""
import ctypes as C
import heapq
import os
from fractions import Fraction

import numpy as np
import pytest

import ksw_cases as KC
import test_dial as TD
import test_dijkstra as TJ

DIAL_WIN = 256


@pytest.fixture(scope="module")
def emk():
    """tests/host_emul/graphs_emul.cpp, built on demand"""
    return KC.build_emul()


def _P(a):
    return a.ctypes.data_as(C.c_void_p)


def batch(graphs):
    """[(n, rowptr, col, weights, src)] -> one batch: g_voff, rowptr, col, weights (rows concatenated), src."""
    voff, rps, cols, ws, srcs = [0], [np.zeros(1, np.int64)], [], [], []
    for n, rp, col, w, src in graphs:
        rps.append(np.asarray(rp[1:], np.int64) + rps[-1][-1]); cols.append(col); ws.append(w); srcs.append(src); voff.append(voff[-1] + n)
    return np.array(voff, np.int64), np.concatenate(rps), np.concatenate(cols), np.concatenate(ws), np.array(srcs)


def emul_dijkstra(lib, voff, rowptr, col, w5, src):
    from alignasm_amd._abi import graph_inputs
    voff, rowptr, col, src, _, w5, _ = graph_inputs(voff, rowptr, col, src, w5=w5)
    d, prev = np.zeros((int(voff[-1]), 5), np.int64), np.zeros(int(voff[-1]), np.int32)
    rc = lib.emk_sssp_dijkstra(C.c_int64(len(voff) - 1), _P(voff), _P(rowptr), _P(col), _P(w5), _P(src), _P(d), _P(prev))
    return rc, d, prev


def emul_dial(lib, voff, rowptr, col, cost, src, lim):
    from alignasm_amd._abi import graph_inputs
    voff, rowptr, col, src, _, _, cost = graph_inputs(voff, rowptr, col, src, cost=cost)
    dist, pre = np.zeros(int(voff[-1]), np.int64), np.zeros(int(voff[-1]), np.int64)
    rc = lib.emk_sssp_dial(C.c_int64(len(voff) - 1), _P(voff), _P(rowptr), _P(col), _P(cost), _P(src), int(lim), _P(dist), _P(pre))
    return rc, dist, pre


# ---- dijkstra ----------------------------------------------------------------------------------------------------------------
def dj_golden(T):
    z = np.load(os.path.join(T.GOLDEN, "ref_algos.npz"))
    return [(int(z[f"dj{i}_meta"][0]), z[f"dj{i}_rowptr"], z[f"dj{i}_col"], z[f"dj{i}_w"], int(z[f"dj{i}_meta"][1]), z[f"dj{i}_d"], z[f"dj{i}_prv"])
            for i in range(int(z["n_dj"][0]))]


def test_emulated_dijkstra_equals_recorded_reference_vectors(T, emk):
    gs = dj_golden(T)
    voff, rowptr, col, w, src = batch([g[:5] for g in gs])
    rc, d, prev = emul_dijkstra(emk, voff, rowptr, col, w, src)
    assert rc == 0
    for i, g in enumerate(gs):
        assert np.array_equal(d[voff[i]:voff[i + 1]], g[5]) and np.array_equal(prev[voff[i]:voff[i + 1]], g[6]), i
        rc, d1, p1 = emul_dijkstra(emk, [0, g[0]], g[1], g[2], g[3], [g[4]])
        assert rc == 0 and np.array_equal(d1, g[5]) and np.array_equal(p1, g[6]), ("alone", i)


def test_emulated_dijkstra_equals_oracle_on_cyclic_digraphs(T, emk):
    """test_dijkstra's random digraphs: cycles, parallel edges, lists in random order; one batch."""
    cs = TJ.cases()
    voff, rowptr, col, w, src = batch(cs)
    rc, d, prev = emul_dijkstra(emk, voff, rowptr, col, w, src)
    assert rc == 0
    for i, (n, rp, cl, ww, s) in enumerate(cs):
        do, po = TJ.run(T.oracle(), "oracle_", n, rp, cl, ww, s)
        assert np.array_equal(d[voff[i]:voff[i + 1]], do) and np.array_equal(prev[voff[i]:voff[i + 1]], po), i


def _heap_peak(n, rp, col, w, src):
    """The largest size the reference's priority queue reaches (pushes and pops as dijkstra() makes them; lazy deletion)."""
    def key(x):
        return (x[0] + x[1], x[2], -Fraction(x[3], x[4] or 1))
    d = [None] * n
    d[src] = (0, 0, 0, 0, 0)
    h, peak = [(key(d[src]), src, d[src])], 1
    while h:
        _, v, dv = heapq.heappop(h)
        if key(dv) != key(d[v]) or dv[:3] != d[v][:3]:
            continue
        for e in range(rp[v], rp[v + 1]):
            to, c = int(col[e]), tuple(int(a + b) for a, b in zip(dv, w[5 * e:5 * e + 5]))
            if d[to] is None or key(c) < key(d[to]):
                d[to] = c
                heapq.heappush(h, (key(c), to, c))
                peak = max(peak, len(h))
    return peak


def heap_retry_graph(m=10):
    """s = 0 reaches u = 1 with mapq ratio 0/0 and x = 2 with 0/1, equal keys, so u is expanded first and pushes its m leaves.  x then
    improves u to 1/2 (a better ratio at the same score sum): u is expanded again and every leaf improves and is pushed again.  The heap
    holds 2m leaf entries at once, more than E + 2 = m + 5: the driver's first run overflows and the 4x run finishes."""
    rows = [[(1, [0, 0, 0, 0, 0]), (2, [0, 0, 0, 0, 1])], [(3 + j, [1, 0, 0, 0, 0]) for j in range(m)], [(1, [0, 0, 0, 1, 1])]] + [[] for _ in range(m)]
    rp, col, w = [0], [], []
    for r in rows:
        for v, ww in r:
            col.append(v); w.extend(ww)
        rp.append(len(col))
    return 3 + m, np.array(rp, np.int64), np.array(col, np.int64), np.array(w, np.int64), 0


def test_emulated_dijkstra_takes_the_heap_retry(T, emk):
    n, rp, col, w, src = heap_retry_graph()
    E = len(col)
    assert E + 2 < _heap_peak(n, rp, col, w, src) <= 4 * (E + 2)
    do, po = TJ.run(T.oracle(), "oracle_", n, rp, col, w, src)
    rc, d, prev = emul_dijkstra(emk, [0, n], rp, col, w, [src])
    assert rc == 0 and np.array_equal(d, do) and np.array_equal(prev, po)
    assert d[3][3] == 1 and prev[3] == 1                   # the leaves carry the improved ratio
    small = TJ.cases()[:4]                                  # beside graphs that fit the first run
    voff, rowptr, cl, ww, s = batch(small + [(n, rp, col, w, src)])
    rc, d, prev = emul_dijkstra(emk, voff, rowptr, cl, ww, s)
    assert rc == 0 and np.array_equal(d[voff[-2]:], do) and np.array_equal(prev[voff[-2]:], po)
    for i, (n1, rp1, c1, w1, s1) in enumerate(small):
        do1, po1 = TJ.run(T.oracle(), "oracle_", n1, rp1, c1, w1, s1)
        assert np.array_equal(d[voff[i]:voff[i + 1]], do1) and np.array_equal(prev[voff[i]:voff[i + 1]], po1), i


# ---- Dial --------------------------------------------------------------------------------------------------------------------
def test_emulated_dial_equals_recorded_reference_vectors_and_oracle(T, emk):
    """test_dial's cases: cycles, parallel edges, zero-cost cycles (lim = 0), lim 0 .. 7, rows far longer than DIAL_WIN, so that one
    bucket's stack spills to global memory and refills; each graph alone, and the lim = 2 graphs in one batch."""
    z = np.load(TD.GOLD)
    cs = TD.cases()
    assert any(lim == 0 for *_, lim in cs) and max(int(np.diff(c[1]).max()) for c in cs) > 4 * DIAL_WIN
    for i, (n, rp, col, cost, src, lim) in enumerate(cs):
        rc, d1, p1 = emul_dial(emk, [0, n], rp, col, cost, [src], lim)
        assert rc == 0 and np.array_equal(d1, z[f"c{i}_dist"]) and np.array_equal(p1, z[f"c{i}_pre"]), ("alone", i)
        do, po = TD.run(T.oracle(), "oracle_", n, rp, col, cost, src, lim)
        assert np.array_equal(d1, do) and np.array_equal(p1, po), i
    two = [(i, c) for i, c in enumerate(cs) if c[5] == 2]
    voff, rowptr, col, cost, src = batch([(n, rp, cl, co, s) for _, (n, rp, cl, co, s, _) in two])
    rc, dist, pre = emul_dial(emk, voff, rowptr, col, cost, src, 2)
    assert rc == 0
    for k, (i, _) in enumerate(two):
        a, b = voff[k], voff[k + 1]
        assert np.array_equal(dist[a:b], z[f"c{i}_dist"]) and np.array_equal(pre[a:b], z[f"c{i}_pre"]), ("batch", i)


# ---- argument checks: the product library, no device needed ---------------------------------------------------------------
def _two_graphs():
    """graph 0: 3 vertices, edges 0->1, 0->2, 1->2; graph 1: 2 vertices, edge 0->1"""
    w = np.tile(np.array([1, 1, 0, 0, 1], np.int64), (4, 1))
    return np.array([0, 3, 5], np.int64), np.array([0, 2, 3, 3, 4, 4], np.int64), np.array([1, 2, 2, 1], np.int64), w, np.array([0, 0], np.int64)


LAYOUT_FAULTS = ["voff0", "voff_flat", "rowptr0", "rowptr_down", "col_out", "col_neg", "source"]


def _layout_fault(what, voff, rowptr, col, src):
    if what == "voff0":
        voff[0] = 1
    elif what == "voff_flat":
        voff[1] = voff[0]
    elif what == "rowptr0":
        rowptr[0] = 1
    elif what == "rowptr_down":
        rowptr[1], rowptr[2] = rowptr[2], rowptr[1]
    elif what == "col_out":
        col[3] = 2                                          # graph 1 has vertices 0, 1
    elif what == "col_neg":
        col[0] = -1
    elif what == "source":
        src[1] = 2


@pytest.mark.parametrize("what", LAYOUT_FAULTS + ["anom", "qnz", "qtot", "score_sum", "score_big", "score_small"])
def test_dijkstra_argument_checks(T, emk, what):
    api = T.api()
    voff, rowptr, col, w, src = _two_graphs()
    code = -1
    if what in LAYOUT_FAULTS:
        _layout_fault(what, voff, rowptr, col, src)
    else:
        code = -5
        if what in ("anom", "qnz", "qtot"):
            w[1, {"anom": 2, "qnz": 3, "qtot": 4}[what]] = 3
        elif what == "score_sum":
            w[1, 0] = -7
        elif what == "score_big":
            w[1, 0] = 1 << 39
        else:
            w[1, 1] = -(1 << 39) - 1
    with pytest.raises(api.AlignasmError) as ei:
        api.sssp_dijkstra(voff, rowptr, col, w, src)
    assert ei.value.code == code
    assert emul_dijkstra(emk, voff, rowptr, col, w, src)[0] == code


@pytest.mark.parametrize("what", LAYOUT_FAULTS + ["cost_big", "cost_neg", "lim_big", "lim_neg"])
def test_dial_argument_checks(T, emk, what):
    api = T.api()
    voff, rowptr, col, _, src = _two_graphs()
    cost, lim = np.array([0, 2, 1, 2], np.int64), 2
    if what in LAYOUT_FAULTS:
        _layout_fault(what, voff, rowptr, col, src)
    elif what == "cost_big":
        cost[3] = 3
    elif what == "cost_neg":
        cost[0] = -1
    elif what == "lim_big":
        lim = 8
    else:
        lim = -1
    with pytest.raises(api.AlignasmError) as ei:
        api.sssp_dial(voff, rowptr, col, cost, src, lim=lim)
    assert ei.value.code == -1
    assert emul_dial(emk, voff, rowptr, col, cost, src, lim)[0] == -1


def test_well_formed_batches_reach_the_device_step(T):
    """The same batches pass every check: without a device the entries then report AASM_E_NODEVICE, not a layout error."""
    api = T.api()
    if api.device_count() > 0:
        pytest.skip("a GPU is present; the no-device path is exercised on CPU-only boxes")
    voff, rowptr, col, w, src = _two_graphs()
    for call in (lambda: api.sssp_dijkstra(voff, rowptr, col, w, src), lambda: api.sssp_dial(voff, rowptr, col, np.array([0, 2, 1, 2]), src),
                 lambda: api.k_shortest_walks(voff, rowptr, col, w, src, np.array([2, 1]), 2)):
        with pytest.raises(api.AlignasmError) as ei:
            call()
        assert ei.value.code == -2


@pytest.mark.parametrize("what", ["rowptr", "col", "w", "src", "sink"])
def test_short_arrays_raise_value_error(T, what):
    """Arrays shorter than the offsets say are refused in Python, before the C side would read past them."""
    api = T.api()
    voff, rowptr, col, w, src = _two_graphs()
    sink, cost = np.array([2, 1]), np.array([0, 2, 1, 2])
    cut = {"rowptr": (rowptr[:-1], col, w, cost, src, sink), "col": (rowptr, col[:-1], w, cost, src, sink),
           "w": (rowptr, col, w[:-1], cost[:-1], src, sink), "src": (rowptr, col, w, cost, src[:1], sink),
           "sink": (rowptr, col, w, cost, src, sink[:1])}[what]
    rp, cl, ww, co, s, t = cut
    with pytest.raises(ValueError):
        api.k_shortest_walks(voff, rp, cl, ww, s, t, 2)
    if what != "sink":
        with pytest.raises(ValueError):
            api.sssp_dijkstra(voff, rp, cl, ww, s)
        with pytest.raises(ValueError):
            api.sssp_dial(voff, rp, cl, co, s)
