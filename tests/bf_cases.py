"""Shared pieces of the tests of aasm_sssp_bellman_ford and of k shortest walks with AASM_KSW_NEGATIVE (tests/test_bf_cpu.py,
tests/test_gpu_bf.py, tests/golden/make_ref_bellman_ford.py): small graphs with negative weights, the recorded reference runs
(tests/golden/ref_bellman_ford.npz), and the runs of the emulation, the product and the checker."""
import ctypes as C
import os

import numpy as np

import bf_checker as BK
import ksw_cases as KC
import ksw_cyclic_cases as CC
from alignasm_amd._abi import AASM_KSW_CYCLES, AASM_KSW_NEGATIVE, bellman_ford_outputs, graph_inputs, unpack_cycles

ROOT = KC.ROOT
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_bellman_ford.npz")
NEG = KC.ALL | AASM_KSW_NEGATIVE                 # the DAG mode with negative weights
NEG_CYC = NEG | AASM_KSW_CYCLES                  # the tree of bellman_ford()
E_INVAL, E_OVERFLOW = -1, -5
HUB_DEGREES = (63, 64, 65, 130)


# ---- hand-made graphs --------------------------------------------------------------------------------------------------
def hub(deg, loops, seed):
    """0 -> 1 (the hub) -> deg edges into eight vertices, so heads repeat inside a chunk of 64 with falling and rising weights; at the
    list positions `loops` the hub has a self-loop with mapq counts (1, 1).  Every other edge has counts (0, 0), so the loop improves
    the hub once (ratio 0 -> 1/1) and never again (2/2 is no better): the edges behind it are relaxed from the improved distance.
    The sink, 10, hangs on the source alone: seen from a sink behind the hub the loop would make best[hub] = hub, on which the
    reference's own BFS over tree[] does not end, and nothing could be recorded."""
    rng = np.random.default_rng(seed)
    edges, w = [(0, 1), (0, 10)], [[5, 0, 0, 0, 0], [-3, 0, 0, 0, 0]]
    for i in range(deg):
        if i in loops:
            edges.append((1, 1)); w.append([0, 0, 0, 1, 1])
        else:
            edges.append((1, int(rng.integers(2, 10)))); w.append([int(rng.integers(-20, 20)), int(rng.integers(0, 5)), int(rng.integers(0, 3)), 0, 0])
    return CC.from_edges(11, edges, w, 0, 10)


def fan_in(deg, seed):
    """The hub the other way round, for the tree of k shortest walks, which relaxes the REVERSED lists: 0 -> 2 .. 9 -> deg parallel
    edges into the hub, 1 -> the sink, 10.  g_rev[hub] names every tail many times inside a chunk of 64."""
    rng = np.random.default_rng(seed)
    edges = [(0, v) for v in range(2, 10)] + [(int(rng.integers(2, 10)), 1) for _ in range(deg)] + [(1, 10)]
    rng.shuffle(edges)
    return CC.from_edges(11, [tuple(int(x) for x in e) for e in edges], [int(x) for x in rng.integers(-20, 20, len(edges))], 0, 10)


def hub_graphs():
    out = []
    for deg in HUB_DEGREES:
        out.append((f"fan_in_{deg}", fan_in(deg, deg + 7)))
        out.append((f"hub_{deg}_loop_mid", hub(deg, {30}, deg)))
        out.append((f"hub_{deg}_loop_last_of_chunk", hub(deg, {min(63, deg - 1)}, deg + 1)))
        if deg > 64:
            out.append((f"hub_{deg}_loop_behind_boundary", hub(deg, {64}, deg + 2)))
            out.append((f"hub_{deg}_two_loops", hub(deg, {17, 64}, deg + 3)))
    return out


def late_path():
    """0 -> 1 -> ... -> 11 with weight -1, and before each such edge in the source's list a dear shortcut 0 -> v: vertex i gets its
    final distance in round i, so round n - 1 = 11 still relaxes and round n does not."""
    edges = [(0, v) for v in range(11, 1, -1)] + [(i, i + 1) for i in range(11)]
    return CC.from_edges(12, edges, [100] * 10 + [-1] * 11, 0, 11)


def hand_graphs():
    g = CC.from_edges
    return [
        ("single_vertex", g(1, [], [], 0, 0)),
        ("negative_self_loop_n1", g(1, [(0, 0)], [-1], 0, 0)),
        ("zero_self_loop_n1", g(1, [(0, 0)], [0], 0, 0)),
        ("negative_2cycle_unreachable", g(4, [(0, 1), (2, 3), (3, 2), (2, 1)], [1, -2, 1, 1], 0, 1)),
        ("negative_2cycle_reachable", g(4, [(0, 1), (1, 2), (2, 1), (1, 3)], [1, 1, -2, 1], 0, 3)),
        ("negative_2cycle_through_source", g(3, [(0, 1), (1, 0), (1, 2)], [1, -2, 1], 0, 2)),
        # 0 -> 2 -> 3 (5 - 2) and 0 -> 1 -> 3 (2 + 1) tie: 2 is queued first, so prv[3] = 2 and 1's equal offer is refused
        ("diamond_tied_negative", g(5, [(0, 2), (0, 1), (2, 3), (1, 3), (3, 4)], [5, 2, -2, 1, -1], 0, 4)),
        ("parallel_edges", g(3, [(0, 1), (0, 1), (0, 1), (0, 1), (1, 2), (1, 2)], [5, 3, -1, 3, -4, -4], 0, 2)),
        ("late_path_12", late_path()),
        ("ever_improving_ratio", CC.ever_improving()),
    ] + hub_graphs()


# ---- random graphs -----------------------------------------------------------------------------------------------------
def _signed_weights(rng, E):
    w = np.zeros((E, 5), np.int64)
    w[:, 0] = rng.integers(-200, 200, E); w[:, 1] = rng.integers(-100, 100, E)
    w[:, 2] = rng.integers(0, 3, E); w[:, 3] = rng.integers(0, 2, E); w[:, 4] = rng.integers(0, 2, E)
    return w


def _reachable_sink(rng, n, rowptr, col, s):
    seen, todo = {s}, [s]
    while todo:
        u = todo.pop()
        for v in col[rowptr[u]:rowptr[u + 1]]:
            if int(v) not in seen:
                seen.add(int(v)); todo.append(int(v))
    return int(rng.choice(sorted(seen - {s}))) if len(seen) > 1 else s


KINDS = ("neg_dag", "potentials", "planted_cycle", "mixed")


def random_graph(rng, kind, nmax=40):
    n = int(rng.integers(2, nmax + 1))
    m = int(rng.integers(n, min(150, 4 * n) + 1))
    if kind == "neg_dag":
        rowptr, col, _, order = KC.random_dag(rng, n, m, "scalar")
        w = _signed_weights(rng, len(col))
        s = int(order[0])
    else:
        rowptr, col, w = CC.random_cyclic(rng, n, m, "mixed")
        s = int(rng.integers(0, n))
        tails = np.repeat(np.arange(n), np.diff(rowptr))
        if kind in ("potentials", "planted_cycle"):                  # every cycle's score sum stays >= 1: the potentials cancel round it
            p = rng.integers(0, 300, n)
            w[:, 0] += p[tails] - p[col]
        else:                                                        # mixed: signs at random, negative cycles now and then
            w[:, 0] -= rng.integers(0, 120, len(col))
        if kind == "planted_cycle":                                  # a cycle of 2 .. 5 vertices whose last edge makes its sum negative
            cyc = [int(x) for x in rng.choice(n, int(rng.integers(2, min(5, n) + 1)), replace=False)]
            rows = [[(int(col[e]), w[e]) for e in range(rowptr[u], rowptr[u + 1])] for u in range(n)]
            for a, b in zip(cyc, cyc[1:] + cyc[:1]):
                wt = np.array([int(rng.integers(0, 20)), 0, 0, 0, 1], np.int64)
                if b == cyc[0]:
                    wt[0] = -200
                rows[a].insert(int(rng.integers(0, len(rows[a]) + 1)), (b, wt))
            rowptr = np.zeros(n + 1, np.int64); rowptr[1:] = np.cumsum([len(r) for r in rows])
            col = np.array([v for r in rows for v, _ in r], np.int64)
            w = np.array([x for r in rows for _, x in r], np.int64).reshape(-1, 5)
    g = KC.graph(n, rowptr, col, w, s, _reachable_sink(rng, n, rowptr, col, s))
    g["kind"] = kind
    return g


def random_graphs(seed, count, kinds=KINDS, nmax=40):
    rng = np.random.default_rng(seed)
    return [random_graph(rng, kinds[i % len(kinds)], nmax) for i in range(count)]


def cases():
    """(name, graph, K) of the recorded file: K = 60 everywhere, 400 for every tenth random graph (the cyclic ones without a
    negative cycle among them, which have that many walks)."""
    out = [(name, g, 60) for name, g in hand_graphs()]
    for i, g in enumerate(random_graphs(20261, 40)):
        out.append((f"random_{g['kind']}_{i}", g, 400 if i % 10 == 1 else 60))
    return out


# ---- the recorded reference runs ---------------------------------------------------------------------------------------
def _ksw_want(z, pre):
    paths, off = [], 0
    for m in z[pre + "path_len"]:
        paths.append(z[pre + "paths"][off:off + int(m)]); off += int(m)
    return {"nd": len(z[pre + "dist"]) // 5, "dist": z[pre + "dist"], "best": z[pre + "best"], "d": z[pre + "d"], "hroot": z[pre + "hroot"],
            "hcount": z[pre + "hcount"], "paths": paths, "arena": z[pre + "arena"].reshape(-1, 10)}


_GOLD = []


def golden_graphs():
    """The recorded graphs, read once: g["bf"] = {status, d, prv, cycle} of bellman_ford(g, src); g["want"] the solver's run with
    is_dag = false, negative_edge = true, or None where bellman_ford(g_rev, sink) reports a cycle; g["want_dag"] with is_dag = true
    (the negative DAGs only)."""
    if not _GOLD:
        z = np.load(GOLDEN)
        for gi in range(int(z["n_graphs"])):
            n, s, t, K = (int(x) for x in z[f"g{gi}_meta"])
            g = KC.graph(n, z[f"g{gi}_rowptr"], z[f"g{gi}_col"], z[f"g{gi}_w"].reshape(-1, 5), s, t)
            g["name"], g["K"] = str(z["names"][gi]), K
            g["bf"] = {"status": int(z[f"g{gi}_bf_status"][0]), "d": z[f"g{gi}_bf_d"], "prv": z[f"g{gi}_bf_prv"], "cycle": z[f"g{gi}_bf_cycle"]}
            g["want"] = _ksw_want(z, f"g{gi}_") if int(z[f"g{gi}_rev_status"][0]) == 0 else None
            g["want_dag"] = _ksw_want(z, f"g{gi}_dag_") if f"g{gi}_dag_dist" in z else None
            _GOLD.append(g)
    return _GOLD


def first_walks(want, k):
    return None if want is None else CC.first_walks(want, k)


# ---- runs (lib: the graph family's emulation library, KC.build_emul) -----------------------------------------------------
def emul_bf(lib, batch, raw=None):
    """emk_sssp_bellman_ford on a batch -> (rc, {d, prev, status, cycles, qhigh}).  raw: replacements for the pointer arguments by
    name (None = NULL), for the argument checks."""
    g_voff, rowptr, col, src, _, w5, _ = graph_inputs(batch["g_voff"], batch["rowptr"], batch["col"], batch["src"], w5=batch["w"])
    d, prev, status, cycle_off, cycle = bellman_ford_outputs(g_voff)
    qhigh = np.zeros(len(g_voff) - 1, np.int64)
    args = dict(g_voff=g_voff, rowptr=rowptr, col=col, w5=w5, src=src, d5=d, prev=prev, status=status, cycle_off=cycle_off, cycle=cycle, qhigh=qhigh)
    args.update(raw or {})
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rc = lib.emk_sssp_bellman_ford(C.c_int64(len(g_voff) - 1), *[P(args[k]) for k in ("g_voff", "rowptr", "col", "w5", "src", "d5", "prev", "status",
                                                                                      "cycle_off", "cycle", "qhigh")])
    return rc, {"d": d, "prev": prev, "status": status, "cycles": unpack_cycles(cycle_off, cycle), "qhigh": qhigh}


def gpu_bf(api, batch):
    d, prev, status, cycles = api.sssp_bellman_ford(batch["g_voff"], batch["rowptr"], batch["col"], batch["w"], batch["src"])
    return {"d": d, "prev": prev, "status": status, "cycles": cycles}


def gpu_ksw(api, batch, k, flags):
    return api.k_shortest_walks(batch["g_voff"], batch["rowptr"], batch["col"], batch["w"], batch["src"], batch["sink"], k,
                                walks=bool(flags & KC.AASM_KSW_WALKS), tree=bool(flags & KC.AASM_KSW_TREE), cycles=bool(flags & AASM_KSW_CYCLES),
                                negative=bool(flags & AASM_KSW_NEGATIVE), _hooks=flags & KC.AASM_KSW_HOOK_ARENA)


def checker_bf(g):
    """bellman_ford(g, src) by the checker, in the recorded shape -> ({status, d, prv, cycle}, the queue's high-water mark)."""
    r, high = BK.sssp(g["n"], g["rowptr"], g["col"], g["w"], g["src"])
    n = g["n"]
    if r[0] == "ok":
        return {"status": 0, "d": np.array([x for t in r[1] for x in t], np.int64), "prv": np.array(r[2], np.int64), "cycle": np.zeros(0, np.int64)}, high
    none = {"d": np.tile(np.array(BK.MAX, np.int64), n), "prv": np.full(n, -1, np.int64)}
    if r[0] == "cycle":
        return dict(none, status=1, cycle=np.array(r[1], np.int64)), high
    return dict(none, status=E_INVAL, cycle=np.zeros(0, np.int64)), high


def checker_ksw(g, K):
    """The checker's k-walk run in KC.compare's shape: None for a graph that must come back AASM_E_INVAL."""
    r = BK.solve(g["n"], g["rowptr"], g["col"], g["w"], g["src"], g["sink"], K)
    return None if r is None or isinstance(r, str) else r


def compare_bf(batch, graphs, wants, got):
    """Mismatches of a bellman_ford batch result against per-graph {status, d, prv, cycle}."""
    bad = []
    for gi, (g, want) in enumerate(zip(graphs, wants)):
        vb, n = int(batch["g_voff"][gi]), g["n"]
        if got["status"][gi] != want["status"]:
            bad.append((gi, "status", int(got["status"][gi]), want["status"])); continue
        if not np.array_equal(got["d"][vb:vb + n].reshape(-1), want["d"]):
            bad.append((gi, "d"))
        if not np.array_equal(got["prev"][vb:vb + n], want["prv"]):
            bad.append((gi, "prev"))
        if not np.array_equal(got["cycles"][gi], want["cycle"]):
            bad.append((gi, "cycle", list(got["cycles"][gi]), list(want["cycle"])))
    return bad


# ---- overhang contigs of the PAF pipeline (GPU tier) -------------------------------------------------------------------
OVERHANG_BATCHES = ((10, 60, 31, "longest"), (8, 80, 32, "mixed"))     # contigs, records, seed, tests/overhang_cases.py's mode


def overhang_batches(T, K):
    """Per batch (graph batch, what the pipeline's K6-K8 computed on it) as KC.pipeline_batch gives them: contig DAGs whose dest edges
    and walk sums are negative, because their records run to or past the query's end."""
    import overhang_cases as OC
    api = T.api()
    out = []
    for nc, nr, seed, mode in OVERHANG_BATCHES:
        hb = OC.overhang(T.synth(nc, nr, seed), mode, seed)
        db = api.DeviceBatch(hb)
        res = db.solve(max_paths=K, keep_debug=True)
        batch, contigs, want = KC.pipeline_batch(res, hb, K)
        res.close(); db.close()
        out.append((batch, want))
    return out
