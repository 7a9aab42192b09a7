"""Shared pieces of the tests of aasm_topology_sort and aasm_sssp_dag (tests/test_dag_cpu.py, tests/test_gpu_dag.py,
tests/golden/make_ref_dag.py): the case list - the smallest shapes at which the kernel's 64-lane list walk can still go wrong -, the
recorded reference runs (tests/golden/ref_dag.npz), and the runs of the emulation, the product and the checker."""
import ctypes as C
import os

import numpy as np

import dag_checker as DK
import ksw_cases as KC
import ksw_cyclic_cases as CC
from alignasm_amd._abi import dag_outputs, graph_inputs

ROOT = KC.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_dag.npz")
E_INVAL, E_OVERFLOW = -1, -5
HUB_DEGREES = (64, 65, 129, 200)
LIM = 1 << 39


def G(n, edges, w, src):
    """A graph from (u, v) pairs in list order; w per pair, a scalar s standing for (s, 0, 0, 0, 1)."""
    return CC.from_edges(n, edges, [[x, 0, 0, 0, 1] if np.isscalar(x) else list(x) for x in w], src, 0)


# ---- hand-made graphs --------------------------------------------------------------------------------------------------
def _tie_weights(rng, m):
    """Small weights in every key, so that candidates tie in the order with different five numbers."""
    return [[int(rng.integers(0, 4)), int(rng.integers(0, 3)), int(rng.integers(0, 3)), int(rng.integers(0, 2)), int(rng.integers(0, 2))] for _ in range(m)]


def hub(deg, seed):
    """0 -> 1 (the hub) -> deg edges.  About half of them lead to eight vertices named again and again, inside a chunk of 64 and
    across chunks; the others each to a vertex of their own, whose ids are a random permutation, so several heads become ready in one
    chunk in an order other than ascending id.  Vertex 0 names a few of the heads itself, before the hub, and every head leads on to
    the last vertex, which the heads reach with tied distances.  From 129 edges on, head 2 is named in the first chunk and then only
    once more, in the third: its last in-edge from the hub lies there."""
    rng = np.random.default_rng(seed)
    rep = list(range(2, 10))
    pick = [bool(rng.random() < 0.5) for _ in range(deg)]
    n_single = deg - sum(pick)
    singles = [int(x) for x in 10 + rng.permutation(n_single)]
    n = 10 + n_single + 1
    heads = []
    for i in range(deg):
        heads.append(int(rng.choice(rep[1:] if deg >= 129 else rep)) if pick[i] else singles.pop())
    if deg >= 129:
        heads[5], heads[20], heads[128] = 2, 2, 2
    pre = [int(x) for x in rng.choice(sorted(set(heads)), 6, replace=False)]
    edges = [(0, v) for v in pre] + [(0, 1)] + [(1, v) for v in heads] + [(v, n - 1) for v in sorted(set(heads), key=lambda x: (x * 7) % 11)]
    return G(n, edges, _tie_weights(rng, len(edges)), 0)


def fan_in(tails, seed):
    """0 -> `tails` vertices in a permuted id order -> one head, with ties: the first tail in the queue among the best stays."""
    rng = np.random.default_rng(seed)
    ids = [int(x) for x in 2 + rng.permutation(tails)]
    edges = [(0, v) for v in ids] + [(v, 1) for v in sorted(ids)]
    w = [[int(rng.integers(0, 3)), 0, 0, 0, 1] for _ in ids] + [[int(rng.integers(0, 3)), int(rng.integers(0, 2)), 0, 0, 1] for _ in ids]
    return G(tails + 2, edges, w, 0)


def straddle(better):
    """A list of 70 edges whose positions 63 and 64 - the last lane of one chunk, the first of the next - are parallel edges: equal
    in the order with another qry / ref split (the first stays), or the second strictly better."""
    edges = [(0, 1)] + [(1, 2 + i) for i in range(63)] + [(1, 70), (1, 70)] + [(1, 2 + i) for i in range(5)]
    w = [[1, 0, 0, 0, 1]] + [[i % 5, 0, 0, 0, 1] for i in range(63)] + [[3, 1, 0, 0, 1], [1, 2 if better else 3, 0, 0, 1]] + [[0, 0, 0, 0, 1]] * 5
    return G(71, edges, w, 0)


def isolated_plus_path():
    path = [137, 2, 66, 131, 64, 9]
    return G(140, list(zip(path, path[1:])), [3, 1, 4, 1, 5], 137)


def long_cycle(n):
    return G(n, [(i, (i + 1) % n) for i in range(n)], [1] * n, 0)


def hand_graphs():
    one = [1, 0, 0, 0, 1]
    out = [
        ("one_vertex", G(1, [], [], 0)),
        ("isolated_70", G(70, [], [], 33)),
        ("isolated_130_plus_path", isolated_plus_path()),
        # 0's list names 2 before 1: the order is 0 2 1 ..., and 3 hears from 2 first; 2's and 1's offers tie
        ("diamond_push_order", G(5, [(0, 2), (0, 1), (2, 3), (1, 3), (1, 4), (2, 4)], [2, 1, [1, 1, 0, 0, 1], [2, 1, 0, 0, 1], 1, 0], 0)),
        ("permuted_ids", G(6, [(4, 2), (2, 0), (0, 3), (3, 1), (4, 0), (2, 3), (4, 5), (5, 1)], [1, 1, 1, 1, 2, 3, 1, 2], 4)),
        ("src_not_a_source", G(6, [(0, 1), (1, 2), (2, 3), (0, 3), (3, 4), (2, 5)], [1, 2, 3, 1, 1, 1], 2)),
        # 0 and 3 come before src = 1 in the order and stay at max(): their edges into 2 and 4 relax nothing
        ("unreachable_before_src", G(5, [(0, 2), (3, 2), (1, 2), (3, 4), (2, 4)], [-50, -60, 5, -70, 1], 1)),
        ("src_reaches_nothing", G(5, [(0, 1), (1, 2), (0, 3), (3, 4)], [1, 1, 1, 1], 4)),
        ("parallel_second_better", G(3, [(0, 1), (0, 1), (1, 2)], [5, 3, 1], 0)),
        ("parallel_equal_other_split", G(3, [(0, 1), (0, 1), (1, 2), (1, 2)], [[3, 1, 0, 0, 1], [1, 3, 0, 0, 1], [1, 3, 0, 0, 1], [3, 1, 0, 0, 1]], 0)),
        ("parallel_straddle_equal", straddle(False)),
        ("parallel_straddle_better", straddle(True)),
    ]
    out += [(f"hub_{deg}", hub(deg, deg)) for deg in HUB_DEGREES] + [(f"hub_{deg}_b", hub(deg, deg + 1000)) for deg in HUB_DEGREES]
    out += [("fan_in_100", fan_in(100, 5)), ("fan_in_64", fan_in(64, 6))]
    out += [
        ("anom_only", G(4, [(0, 1), (0, 2), (1, 3), (2, 3)], [[2, 2, 1, 0, 1], [3, 1, 0, 0, 1], [1, 1, 1, 0, 1], [1, 1, 1, 0, 1]], 0)),
        # the mapq ratio alone: 0 / (0 -> 1), 1 / 1, 0 / 1, 1 / 2; the greater ratio is the better distance
        ("ratio_only", G(6, [(0, 1), (0, 2), (0, 3), (0, 4), (1, 5), (2, 5), (3, 5), (4, 5)],
                         [[1, 0, 0, 0, 0], [1, 0, 0, 1, 1], [1, 0, 0, 0, 1], [1, 0, 0, 1, 1], [1, 0, 0, 0, 0], [1, 0, 0, 0, 0], [1, 0, 0, 0, 0], [1, 0, 0, 0, 1]], 0)),
        ("ratio_zero_total", G(3, [(0, 1), (0, 1), (1, 2), (1, 2)], [[1, 0, 0, 0, 0], [0, 1, 0, 0, 1], [2, 0, 0, 0, 0], [2, 0, 0, 1, 1]], 0)),
        ("negative_sums", G(6, [(0, 1), (0, 2), (1, 3), (2, 3), (3, 4), (1, 4), (4, 5), (2, 5)],
                            [[-5, 2, 0, 0, 1], [3, -9, 1, 0, 1], [-4, 0, 0, 1, 1], [2, 0, 0, 0, 1], [-7, -7, 2, 0, 0], [-20, 0, 0, 0, 1], one, [-30, 5, 0, 1, 1]], 0)),
        ("scores_near_limit", G(5, [(0, 1), (0, 2), (1, 3), (2, 3), (3, 4), (0, 4)],
                                [[LIM - 1, -LIM, 0, 0, 1], [-LIM, LIM - 1, 0, 0, 1], [LIM - 1, LIM - 1, 0, 0, 1], [LIM - 1, LIM - 2, 1, 0, 1],
                                 [-LIM, -LIM, 0, 1, 1], [LIM - 1, LIM - 1, 0, 0, 0]], 0)),
        ("self_loop", G(3, [(0, 1), (1, 1), (1, 2)], [1, 1, 1], 0)),
        ("self_loop_alone", G(1, [(0, 0)], [1], 0)),
        ("two_cycle", G(4, [(0, 1), (1, 2), (2, 1), (2, 3)], [1, 1, 1, 1], 0)),
        ("long_cycle_150", long_cycle(150)),
        ("cycle_src_cannot_reach", G(6, [(0, 1), (1, 2), (3, 4), (4, 5), (5, 3)], [1, 1, 1, 1, 1], 0)),
        ("cycle_behind_a_dag_part", G(7, [(0, 1), (0, 2), (1, 3), (2, 3), (3, 4), (4, 5), (5, 6), (6, 4)], [1, 2, 2, 1, 1, 1, 1, 1], 0)),
    ]
    return out


# ---- random DAGs -------------------------------------------------------------------------------------------------------
KINDS = ("mixed", "zero", "big", "scalar", "signed")


def random_graph(rng, kind, nmax, nmin=2, dense=False):
    """A DAG whose ids are a random permutation of a topological order, lists shuffled, parallel edges.  dense: six edges per vertex
    and src among the first of the order, so that src reaches a large part of a large graph."""
    n = int(rng.integers(nmin, nmax + 1))
    m = 6 * n if dense else int(rng.integers(n // 2, 4 * n + 1))
    rowptr, col, w, topo = KC.random_dag(rng, n, m, "scalar" if kind == "signed" else kind)
    if kind == "signed":
        E = len(col)
        w = np.stack([rng.integers(-200, 200, E), rng.integers(-100, 100, E), rng.integers(0, 3, E), rng.integers(0, 2, E), rng.integers(0, 2, E)], 1)
    # src: mostly among the first third of a topological order, so that it reaches much of the graph; else any vertex
    src = int(topo[rng.integers(0, max(1, n // (50 if dense else 3)))]) if dense or rng.random() < 0.7 else int(rng.integers(0, n))
    g = KC.graph(n, rowptr, col, w, src, 0)
    g["kind"] = kind
    return g


def random_graphs(seed, count, nmax=300, nmin=2, dense=False):
    rng = np.random.default_rng(seed)
    return [random_graph(rng, KINDS[i % len(KINDS)], nmax, nmin, dense) for i in range(count)]


def cases():
    """(name, graph) of the recorded file."""
    return hand_graphs() + [(f"random_{g['kind']}_{i}", g) for i, g in enumerate(random_graphs(20262, 40))]


def reversed_graph(g):
    """g_rev as k_shortest_walks() builds it (:180-183): v's list holds the tails of v's in-edges in ascending edge id; src = g's sink."""
    n, rp, col = g["n"], g["rowptr"], g["col"]
    tail = np.repeat(np.arange(n), np.diff(rp))
    by_head = np.argsort(col, kind="stable")
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(col, minlength=n))
    return KC.graph(n, rowptr, tail[by_head], g["w"][by_head], g["sink"], g["src"])


# ---- the recorded reference runs ---------------------------------------------------------------------------------------
_GOLD = []


def golden_graphs():
    """The recorded graphs, read once: g["want"] = {status, order, d, prv} of topology_sort(g) and shortest_path_dag(g, src); the
    reference's empty order of a graph with a cycle is recorded as status 1 and given here as -1 everywhere."""
    if not _GOLD:
        z = np.load(GOLDEN)
        for gi in range(int(z["n_graphs"])):
            n, s = (int(x) for x in z[f"g{gi}_meta"])
            g = KC.graph(n, z[f"g{gi}_rowptr"], z[f"g{gi}_col"], z[f"g{gi}_w"].reshape(-1, 5), s, 0)
            g["name"] = str(z["names"][gi])
            order = z[f"g{gi}_order"]
            assert len(order) in (0, n)
            g["want"] = {"status": 0 if len(order) == n else 1, "order": order if len(order) == n else np.full(n, -1, np.int64),
                         "d": z[f"g{gi}_d"], "prv": z[f"g{gi}_prv"]}
            _GOLD.append(g)
    return _GOLD


# ---- runs (lib: the graph family's emulation library, KC.build_emul) -----------------------------------------------------
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def emul_dag(lib, batch, raw=None):
    """emk_sssp_dag on a batch -> (rc, {d, prev, order, status}).  raw: replacements for the pointer arguments by name (None = NULL),
    for the argument checks."""
    g_voff, rowptr, col, src, _, w5, _ = graph_inputs(batch["g_voff"], batch["rowptr"], batch["col"], batch["src"], w5=batch["w"])
    d, prev, order, status = dag_outputs(g_voff)
    args = dict(g_voff=g_voff, rowptr=rowptr, col=col, w5=w5, src=src, d5=d, prev=prev, order=order, status=status)
    args.update(raw or {})
    rc = lib.emk_sssp_dag(C.c_int64(len(g_voff) - 1), *[_ptr(args[k]) for k in ("g_voff", "rowptr", "col", "w5", "src", "d5", "prev", "order", "status")])
    return rc, {"d": d, "prev": prev, "order": order, "status": status}


def emul_topo(lib, batch, raw=None):
    g_voff, rowptr, col, _, _, _, _ = graph_inputs(batch["g_voff"], batch["rowptr"], batch["col"], None)
    order, status = dag_outputs(g_voff, relax=False)
    args = dict(g_voff=g_voff, rowptr=rowptr, col=col, order=order, status=status)
    args.update(raw or {})
    rc = lib.emk_topology_sort(C.c_int64(len(g_voff) - 1), *[_ptr(args[k]) for k in ("g_voff", "rowptr", "col", "order", "status")])
    return rc, {"order": order, "status": status}


def gpu_dag(api, batch):
    d, prev, status, order = api.sssp_dag(batch["g_voff"], batch["rowptr"], batch["col"], batch["w"], batch["src"], order=True)
    return {"d": d, "prev": prev, "order": order, "status": status}


def gpu_topo(api, batch):
    order, status = api.topology_sort(batch["g_voff"], batch["rowptr"], batch["col"])
    return {"order": order, "status": status}


def checker(g):
    return DK.solve(g["n"], g["rowptr"], g["col"], g["w"], g["src"])


def compare_dag(batch, graphs, wants, got):
    """Mismatches of a batch result against per-graph {status, order, d, prv}; a result without d (the sort alone) is held to
    status and order."""
    bad = []
    for gi, (g, want) in enumerate(zip(graphs, wants)):
        vb, n = int(batch["g_voff"][gi]), g["n"]
        if got["status"][gi] != want["status"]:
            bad.append((gi, "status", int(got["status"][gi]), want["status"])); continue
        if not np.array_equal(got["order"][vb:vb + n], want["order"]):
            bad.append((gi, "order"))
        if "d" in got and not np.array_equal(got["d"][vb:vb + n].reshape(-1), want["d"]):
            bad.append((gi, "d"))
        if "prev" in got and not np.array_equal(got["prev"][vb:vb + n], want["prv"]):
            bad.append((gi, "prev"))
    return bad


# ---- contig graphs of the PAF pipeline (GPU tier) ----------------------------------------------------------------------
def pipeline_dags(api, hb, K=4):
    """The contig DAGs of a solve of `hb` with keep_debug, as KC.pipeline_batch gives them (src = V - 2, sink = V - 1), beside the
    pipeline's own sweeps on them: want["fwd_order"] / ["rev_order"] (local ids) and KC.pipeline_batch's d5 / best, which its reverse
    sweep computed from the sink."""
    db = api.DeviceBatch(hb)
    res = db.solve(max_paths=K, keep_debug=True)
    try:
        batch, contigs, want = KC.pipeline_batch(res, hb, K)
        ctgV, voff = res.debug("ctgV", np.int32), res.debug("voff", np.int64)
        vsel = np.concatenate([np.arange(voff[c], voff[c] + ctgV[c]) for c in contigs])
        want = dict(want, fwd_order=res.debug("fwd_order", np.int32)[vsel].copy(), rev_order=res.debug("rev_order", np.int32)[vsel].copy())
    finally:
        res.close(); db.close()
    return batch, want


def reversed_batch(batch):
    """Every graph of a batch reversed as reversed_graph does, from its sink."""
    out = []
    for gi in range(len(batch["src"])):
        vb, ve = int(batch["g_voff"][gi]), int(batch["g_voff"][gi + 1])
        rp = batch["rowptr"][vb:ve + 1]
        g = KC.graph(ve - vb, rp - rp[0], batch["col"][rp[0]:rp[-1]], batch["w"][rp[0]:rp[-1]], batch["src"][gi], batch["sink"][gi])
        out.append(reversed_graph(g))
    return KC.make_batch(out)
