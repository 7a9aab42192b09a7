"""Shared pieces of the tests of k shortest walks on graphs with cycles (AASM_KSW_CYCLES; tests/test_ksw_cyclic_cpu.py,
tests/test_gpu_ksw_cyclic.py, tests/golden/make_ref_ksw_cyclic.py): the hand-made and random graphs, the recorded reference runs
(tests/golden/ref_ksw_cyclic.npz), and the runs of the emulation, the product and the checker with the flag."""
import os

import numpy as np

import ksw_cases as KC
import ksw_cyclic_checker as CK
from alignasm_amd._abi import AASM_KSW_CYCLES

ROOT = KC.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_ksw_cyclic.npz")
ALL = KC.ALL | AASM_KSW_CYCLES
LIM = KC.LIM
E_INVAL, E_OVERFLOW = -1, -5


def from_edges(n, edges, w, src, sink):
    """A graph from (u, v) pairs in list order (a vertex's list keeps the order of the pairs); w per pair, scalars or 5-tuples."""
    order = sorted(range(len(edges)), key=lambda i: edges[i][0])
    rowptr = np.zeros(n + 1, np.int64)
    for u, _ in edges:
        rowptr[u + 1] += 1
    return KC.graph(n, np.cumsum(rowptr), [edges[i][1] for i in order], np.array([w[i] for i in order], np.int64), src, sink)


def hand_graphs():
    """(name, graph): the shapes the DAG mode cannot have, and two DAGs with tied distances."""
    one = [1, 0, 0, 0, 1]
    out = [
        ("cycle", KC.cycle_graph()),
        ("sink_back_to_source", from_edges(4, [(0, 1), (1, 2), (2, 1), (2, 3), (3, 0)], [1, 1, 1, 1, 2], 0, 3)),
        ("source_is_sink_on_cycle", from_edges(3, [(0, 1), (1, 2), (2, 0), (1, 0)], [1, 2, 1, 5], 0, 0)),
        ("self_loop", from_edges(3, [(0, 1), (1, 1), (1, 2)], [2, 1, 3], 0, 2)),
        ("self_loop_on_sink", from_edges(2, [(0, 1), (1, 1)], [1, 2], 0, 1)),
        ("parallel_in_cycle", from_edges(4, [(0, 1), (1, 2), (1, 2), (2, 1), (2, 1), (2, 3), (2, 3)], [1, 1, 1, 2, 1, 1, 3], 0, 3)),
        ("zero_cycle", from_edges(4, [(0, 1), (1, 2), (2, 1), (2, 3)], [[0] * 5] * 4, 0, 3)),
        ("zero_scalar_cycle", from_edges(4, [(0, 1), (1, 2), (2, 1), (2, 3)], [0, 0, 0, 0], 0, 3)),
        ("source_cannot_reach_sink", from_edges(4, [(1, 0), (1, 2), (2, 1), (2, 3)], [1, 1, 1, 1], 0, 3)),
        ("cycle_cannot_reach_sink", from_edges(5, [(0, 1), (1, 2), (2, 1), (0, 3), (3, 4), (0, 4)], [1, 1, 1, 1, 1, 5], 0, 4)),
        ("two_cycles_on_the_way", from_edges(6, [(0, 1), (1, 2), (2, 1), (2, 3), (3, 4), (4, 3), (4, 5)], [1, 2, 1, 1, 1, 3, 1], 0, 5)),
        # 0 -> 1 -> 3 (1 + 3) and 0 -> 2 -> 3 (3 + 1) tie: the DAG relaxation takes the reversed graph's Kahn order (1 before 2,
        # best[0] = 1), dijkstra pops the nearer vertex first (2 before 1, best[0] = 2)
        ("dag_tied_trees", from_edges(5, [(0, 2), (0, 1), (2, 3), (1, 3), (0, 3), (4, 0)], [3, 1, 1, 3, 9, 1], 4, 3)),
        ("dag_tied_mapq", from_edges(4, [(0, 1), (0, 2), (1, 3), (2, 3)], [one, [1, 0, 0, 1, 1], [1, 0, 0, 1, 1], one], 0, 3)),
    ]
    return out


def random_cyclic(rng, n, m, kind, par=0.15, loops=0.05):
    """A digraph of n vertices and about m edges with cycles, self-loops (rate loops) and parallel edges (rate par), lists shuffled.
    In every kind the first key (the score sum) rises strictly along an edge or the mapq ratio is the same on every walk, so
    dijkstra() pushes a vertex at most once per in-edge: the reference returns."""
    edges = []
    for _ in range(m):
        a, b = (int(x) for x in rng.integers(0, n, 2))
        if a == b and rng.random() >= loops * 4:
            continue
        edges.append((a, b))
        if rng.random() < par:
            edges.append((a, b))
    rng.shuffle(edges)
    rows = [[] for _ in range(n)]
    for u, v in edges:
        rows[u].append(v)
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.array([v for r in rows for v in r], np.int64)
    E = len(col)
    w = np.zeros((E, 5), np.int64)
    if kind == "scalar":
        w[:, 0] = rng.integers(0, 4, E); w[:, 4] = 1
    elif kind == "scalar1":
        w[:, 0] = rng.integers(1, 5, E); w[:, 4] = 1
    elif kind == "mixed":
        w[:, 0] = rng.integers(-50, 200, E)
        w[:, 1] = rng.integers(0, 100, E)
        w[:, 1] = np.maximum(w[:, 1], 1 - w[:, 0])
        w[:, 2] = rng.integers(0, 3, E)
        w[:, 3] = rng.integers(0, 2, E)
        w[:, 4] = rng.integers(0, 2, E)
    elif kind == "big":
        q = rng.integers(LIM - 64, LIM, E)
        sign = rng.random(E) < 0.5
        w[:, 0] = np.where(sign, q, -q)
        w[:, 1] = np.minimum(np.where(sign, -q, q) + rng.integers(1, 64, E), LIM - 1)
        w[:, 0] = np.maximum(w[:, 0], 1 - w[:, 1])
        w[:, 2] = rng.integers(0, 3, E)
        w[:, 3] = rng.integers(0, 2, E)
        w[:, 4] = rng.integers(0, 2, E)
    else:
        assert kind == "zero"
    return rowptr, col, w


KINDS = ("scalar", "zero", "mixed", "big")


def random_graphs(seed, count, kinds=KINDS, nmax=40):
    """Random cyclic graphs of the four kinds in turn.  The sink is a vertex the source reaches (the source itself now and then),
    or, one time in eleven, any vertex: then there may be no walk."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        kind = kinds[i % len(kinds)]
        n = int(rng.integers(2, nmax + 1))
        m = int(rng.integers(n // 2 + 1, 3 * n + 1))
        rowptr, col, w = random_cyclic(rng, n, m, kind)
        s = int(rng.integers(0, n))
        seen, todo = {s}, [s]
        while todo:
            u = todo.pop()
            for v in col[rowptr[u]:rowptr[u + 1]]:
                if int(v) not in seen:
                    seen.add(int(v)); todo.append(int(v))
        if i % 11 == 7:
            t = int(rng.integers(0, n))
        elif i % 13 == 3 or len(seen) == 1:
            t = s
        else:
            t = int(rng.choice(sorted(seen - {s})))
        g = KC.graph(n, rowptr, col, w, s, t)
        g["kind"] = kind
        out.append(g)
    return out


def ever_improving():
    """a -> t with mapq counts (0, 1); a <-> b with (1, 1), all scores zero: seen from t, d[a] goes 0/1, 2/3, 4/5, ... for ever."""
    return from_edges(3, [(0, 2), (0, 1), (1, 0)], [[0, 0, 0, 0, 1], [0, 0, 0, 1, 1], [0, 0, 0, 1, 1]], 0, 2)


def sink_improves():
    """0 <-> 1 with mapq counts (1, 1), all scores zero, sink 1: round the cycle the sink's own distance improves once, from the
    identity (ratio 0) to 2/2, and best[] becomes the cycle 0 -> 1 -> 0.  The reference's BFS over tree[] never ends on it."""
    return from_edges(2, [(0, 1), (1, 0)], [[0, 0, 0, 1, 1]] * 2, 0, 1)


# ---- the recorded reference runs ---------------------------------------------------------------------------------------
def golden_graphs():
    z = np.load(GOLDEN)
    out = []
    for g in range(int(z["n_graphs"])):
        n, s, t, K = (int(x) for x in z[f"g{g}_meta"])
        gr = KC.graph(n, z[f"g{g}_rowptr"], z[f"g{g}_col"], z[f"g{g}_w"].reshape(-1, 5), s, t)
        paths, off = [], 0
        for m in z[f"g{g}_path_len"]:
            paths.append(z[f"g{g}_paths"][off:off + int(m)]); off += int(m)
        gr["want"] = {"nd": len(z[f"g{g}_dist"]) // 5, "dist": z[f"g{g}_dist"], "best": z[f"g{g}_best"], "d": z[f"g{g}_d"],
                      "hroot": z[f"g{g}_hroot"], "hcount": z[f"g{g}_hcount"], "paths": paths}
        gr["K"] = K
        gr["name"] = str(z["names"][g])
        out.append(gr)
    return out


def first_walks(want, k):
    """A recorded run cut down to its first k walks (the enumeration does not depend on k but for where it stops)."""
    nd = min(want["nd"], k)
    return dict(want, nd=nd, dist=want["dist"][:5 * nd], paths=want["paths"][:nd])


# ---- runs --------------------------------------------------------------------------------------------------------------
def emul_run(lib, batch, k, flags=ALL, budget=0):
    return KC.emul_run(lib, batch, k, flags, budget)


def gpu_run(api, batch, k, flags=ALL):
    return api.k_shortest_walks(batch["g_voff"], batch["rowptr"], batch["col"], batch["w"], batch["src"], batch["sink"], k,
                                walks=bool(flags & KC.AASM_KSW_WALKS), tree=bool(flags & KC.AASM_KSW_TREE),
                                cycles=bool(flags & AASM_KSW_CYCLES), _hooks=flags & KC.AASM_KSW_HOOK_ARENA)


def checker_run(g, K, tree="dijkstra"):
    return CK.solve(g["n"], g["rowptr"], g["col"], g["w"], g["src"], g["sink"], K, tree=tree)


def arena_words(got, gi):
    off = np.concatenate([[0], np.cumsum(got["heap_nodes"])])
    return got["hook_arena"][off[gi]:off[gi + 1]]
