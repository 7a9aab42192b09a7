"""Shared pieces of the k-shortest-walks tests (tests/test_ksw_cpu.py, tests/test_gpu_ksw.py): graph batches, the host
emulation of aasm_ksw.h (tests/host_emul/graphs_emul.cpp), the per-graph oracle / reference, and one comparison for all of them."""
import ctypes as C
import os

import numpy as np

import aasm_testlib
from alignasm_amd._abi import AASM_KSW_HOOK_ARENA, AASM_KSW_TREE, AASM_KSW_WALKS, KswOut, ksw_inputs, unpack_ksw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_algos.npz")
ALL = AASM_KSW_WALKS | AASM_KSW_TREE | AASM_KSW_HOOK_ARENA
LIM = 1 << 39


def _declare(lib):
    """The graph family's entries (tests/host_emul/graphs_emul.cpp): the host drivers emk_*, resident batches emr_*, k shortest walks on
    them emw_*."""
    for fn, n in ((lib.emk_k_shortest_walks, None), (lib.emk_sssp_dijkstra, None), (lib.emk_sssp_dial, None), (lib.emk_sssp_bellman_ford, None),
                  (lib.emk_topology_sort, None), (lib.emk_sssp_dag, None), (lib.emr_host_check, 1), (lib.emr_dijkstra, 4), (lib.emr_bellman_ford, 7),
                  (lib.emr_topology_sort, 3), (lib.emr_dag, 6), (lib.emr_dial, 5), (lib.emw_export, 3)):
        fn.restype = C.c_int
        if n:
            fn.argtypes = [C.c_void_p] * n
    lib.emk_bf_queue_room.restype, lib.emk_bf_queue_room.argtypes = C.c_int64, [C.c_int64]
    lib.emr_last_error.restype = C.c_char_p
    lib.emr_first_negative.restype = lib.emr_work_bytes.restype = C.c_int64
    lib.emr_first_negative.argtypes = lib.emr_work_bytes.argtypes = lib.emr_graphs_free.argtypes = [C.c_void_p]
    lib.emr_graphs_free.restype = None
    lib.emr_graphs_make.restype, lib.emr_graphs_make.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_void_p]
    lib.emw_solve.restype, lib.emw_solve.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    lib.emw_read_bytes.restype = C.c_int64
    lib.emw_alloc_limit.restype, lib.emw_alloc_limit.argtypes = None, [C.c_int64]


def build_emul(san=False):
    """The host emulation of the graph family -> its library, or with san (library, path of graphs_emul_san)."""
    return aasm_testlib.build_emul("graphs", san, _declare)


def emul_run(lib, batch, k, flags=ALL, budget=0):
    """The emulated entry on a batch (dict from make_batch); returns (rc, result dict or None)."""
    g_voff, rowptr, col, w5, src, sink = ksw_inputs(batch["g_voff"], batch["rowptr"], batch["col"], batch["w"], batch["src"], batch["sink"])
    out = KswOut()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.emk_k_shortest_walks(C.c_int64(len(g_voff) - 1), P(g_voff), P(rowptr), P(col), P(w5), P(src), P(sink), C.c_int64(k),
                                  int(flags), C.byref(out), C.c_int64(budget))
    if rc != 0:
        return rc, None
    try:
        return rc, unpack_ksw(out, int(g_voff[-1]), flags)
    finally:
        lib.emk_free(C.byref(out))


def gpu_run(api, batch, k, flags=ALL):
    return api.k_shortest_walks(batch["g_voff"], batch["rowptr"], batch["col"], batch["w"], batch["src"], batch["sink"], k,
                                walks=bool(flags & AASM_KSW_WALKS), tree=bool(flags & AASM_KSW_TREE), _hooks=flags & AASM_KSW_HOOK_ARENA)


# ---- graphs ------------------------------------------------------------------------------------------------------------
def graph(n, rowptr, col, w, src, sink):
    w = np.asarray(w, np.int64)
    if w.ndim == 1 and len(w) == 5 * len(col) and len(col) and len(w) != len(col):
        w = w.reshape(-1, 5)
    if w.ndim == 1:
        w5 = np.zeros((len(w), 5), np.int64); w5[:, 0] = w; w5[:, 4] = 1
        w = w5
    return {"n": int(n), "rowptr": np.asarray(rowptr, np.int64), "col": np.asarray(col, np.int64), "w": w.reshape(-1, 5).astype(np.int64),
            "src": int(src), "sink": int(sink)}


def golden_graphs():
    z = np.load(GOLDEN)
    out = []
    for g in range(int(z["n_graphs"][0]) if z["n_graphs"].ndim else int(z["n_graphs"])):
        n, s, t, K = (int(x) for x in z[f"g{g}_meta"])
        gr = graph(n, z[f"g{g}_rowptr"], z[f"g{g}_col"], z[f"g{g}_w"].reshape(-1, 5), s, t)
        paths, off = [], 0
        for m in z[f"g{g}_path_len"]:
            paths.append(z[f"g{g}_paths"][off:off + int(m)]); off += int(m)
        gr["want"] = {"nd": len(z[f"g{g}_dist"]) // 5, "dist": z[f"g{g}_dist"], "best": z[f"g{g}_best"], "d": z[f"g{g}_d"],
                      "hroot": z[f"g{g}_hroot"], "hcount": z[f"g{g}_hcount"], "paths": paths}
        gr["K"] = K
        out.append(gr)
    return out


def random_dag(rng, n, m, kind="mixed", par=0.2):
    """A DAG of n vertices and about m edges in a random topological order (lists shuffled, parallel edges at rate par)."""
    rank = rng.permutation(n)
    edges = []
    for _ in range(m if n > 1 else 0):
        a, b = rng.integers(0, n, 2)
        if rank[a] == rank[b]:
            continue
        u, v = (a, b) if rank[a] < rank[b] else (b, a)
        edges.append((int(u), int(v)))
        if rng.random() < par:
            edges.append((int(u), int(v)))
    rng.shuffle(edges)
    rows = [[] for _ in range(n)]
    for u, v in edges:
        rows[u].append(v)
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.array([v for r in rows for v in r], np.int64)
    E = len(col)
    w = np.zeros((E, 5), np.int64)
    if kind == "zero":
        pass
    elif kind == "big":
        q = rng.integers(LIM - 64, LIM, E)
        sign = rng.random(E) < 0.5
        w[:, 0] = np.where(sign, q, -q + rng.integers(0, 3, E) * 0)
        w[:, 1] = np.where(sign, -q + rng.integers(0, 64, E), q + rng.integers(0, 64, E))
        w[:, 1] = np.minimum(w[:, 1], LIM - 1)
        w[:, 0] = np.maximum(w[:, 0], -w[:, 1])
    elif kind == "scalar":
        w[:, 0] = rng.integers(0, 4, E); w[:, 4] = 1
    else:
        w[:, 0] = rng.integers(-50, 200, E)
        w[:, 1] = rng.integers(0, 100, E)
        w[:, 1] = np.maximum(w[:, 1], -w[:, 0])
        w[:, 2] = rng.integers(0, 3, E)
        w[:, 3] = rng.integers(0, 2, E)
        w[:, 4] = rng.integers(0, 2, E)
    order = np.argsort(rank)
    return rowptr, col, w, order


def random_graphs(seed, count):
    """Mixed random DAGs covering: parallel edges, shuffled lists, vertices that cannot reach the sink or are unreachable
    from the source, source == sink, a single vertex, all-zero weights, weights near +-2^39."""
    rng = np.random.default_rng(seed)
    kinds = ("mixed", "zero", "big", "scalar")
    out = []
    for i in range(count):
        kind = kinds[i % len(kinds)]
        n = 1 if i % 17 == 5 else int(rng.integers(2, 40))
        m = int(rng.integers(0, 4 * n + 1))
        rowptr, col, w, order = random_dag(rng, n, m, kind)
        if n == 1 or i % 13 == 3:
            s = t = int(rng.integers(0, n))
        else:
            a, b = sorted(rng.choice(n, 2, replace=False))
            s, t = int(order[min(a, n - 1)]), int(order[b])
            if i % 11 == 7:                                          # source after the sink: no walk
                s, t = t, s
        out.append(graph(n, rowptr, col, w, s, t))
    return out


def cycle_graph():
    # 0 -> 1 -> 2 -> 1, 2 -> 3
    return graph(4, [0, 1, 2, 4, 4], [1, 2, 1, 3], [1, 1, 1, 1], 0, 3)


def make_batch(graphs):
    n = [g["n"] for g in graphs]
    g_voff = np.zeros(len(graphs) + 1, np.int64); g_voff[1:] = np.cumsum(n)
    rps, base = [np.zeros(1, np.int64)], 0
    for g in graphs:
        rps.append(g["rowptr"][1:] + base); base += int(g["rowptr"][-1])
    return {"g_voff": g_voff, "rowptr": np.concatenate(rps), "col": np.concatenate([g["col"] for g in graphs]).astype(np.int32),
            "w": np.concatenate([g["w"] for g in graphs]).reshape(-1, 5), "src": np.array([g["src"] for g in graphs], np.int32),
            "sink": np.array([g["sink"] for g in graphs], np.int32)}


# ---- what the checkers say ---------------------------------------------------------------------------------------------
def checker_run(T, lib, prefix, g, K):
    return T.generic_run(lib, prefix, g["n"], np.ascontiguousarray(g["rowptr"], np.int64), np.ascontiguousarray(g["col"], np.int64),
                         np.ascontiguousarray(g["w"].reshape(-1), np.int64), g["src"], g["sink"], K)


def compare(batch, graphs, wants, got, k, check_hroot=True):
    """Mismatches of a batch result against per-graph checker outputs (None: a graph that must come back AASM_E_INVAL)."""
    bad = []
    g_voff, rowptr = batch["g_voff"], batch["rowptr"]
    VT = int(g_voff[-1])
    tail = np.repeat(np.arange(VT, dtype=np.int64), np.diff(rowptr))
    w_all = batch["w"].reshape(-1, 5)
    for gi, (g, want) in enumerate(zip(graphs, wants)):
        vb = int(g_voff[gi]); n = g["n"]
        if want is None:
            if got["status"][gi] != -1 or got["n_found"][gi] != 0:
                bad.append((gi, "cycle", int(got["status"][gi]), int(got["n_found"][gi])))
            continue
        if got["status"][gi] != 0:
            bad.append((gi, "status", int(got["status"][gi]))); continue
        nd = want["nd"]
        if got["n_found"][gi] != min(nd, k):
            bad.append((gi, "n_found", int(got["n_found"][gi]), nd)); continue
        if not np.array_equal(got["dist"][gi, :nd].reshape(-1), np.asarray(want["dist"][:nd * 5])):
            bad.append((gi, "dist"))
        if np.any(got["dist"][gi, nd:]):
            bad.append((gi, "dist beyond n_found"))
        if "best" in got and not np.array_equal(got["best"][vb:vb + n], want["best"]):
            bad.append((gi, "best"))
        if "d" in got and not np.array_equal(got["d"][vb:vb + n].reshape(-1), want["d"]):
            bad.append((gi, "d"))
        if got["heap_nodes"][gi] != int(np.asarray(want["hcount"]).reshape(-1)[0]):
            bad.append((gi, "heap_nodes", int(got["heap_nodes"][gi]), int(np.asarray(want["hcount"]).reshape(-1)[0])))
        if check_hroot and nd and "hook_hroot" in got and not np.array_equal(got["hook_hroot"][vb:vb + n], want["hroot"]):
            bad.append((gi, "hroot"))
        if "walk_off" in got:
            wo, we = got["walk_off"], got["walk_edges"]
            for i in range(k):
                a, b = int(wo[gi * k + i]), int(wo[gi * k + i + 1])
                if i >= nd:
                    if a != b:
                        bad.append((gi, i, "walk beyond n_found"))
                    continue
                e = we[a:b]
                uv = np.stack([tail[e] - vb, batch["col"][e].astype(np.int64)], 1).reshape(-1) if len(e) else np.zeros(0, np.int64)
                if not np.array_equal(uv, want["paths"][i]):
                    bad.append((gi, i, "walk")); break
                if not np.array_equal(w_all[e].sum(0) if len(e) else np.zeros(5, np.int64), got["dist"][gi, i]):
                    bad.append((gi, i, "walk weight sum")); break
        if len(bad) > 20:
            break
    return bad


# ---- contig graphs of the PAF pipeline (a solve with keep_debug) -------------------------------------------------------
def pipeline_batch(res, hb, K):
    """The alignment DAGs the pipeline built for the contigs of `hb` (those with a graph), as one batch with source V - 2 and
    sink V - 1, beside what the pipeline's K6-K8 computed on them: (batch, contigs, want) with want[name][i] for contig i."""
    from aasm_testlib import DIST_DT
    rec_off = hb.arrays["ctg_rec_off"]
    nC = len(rec_off) - 1
    ctgV, voff = res.debug("ctgV", np.int32)[:nC], res.debug("voff", np.int64)[:nC + 1]
    rowptr, col = res.debug("csr_rowptr", np.int64), res.debug("csr_col", np.int32)
    wq, wr, fl = res.debug("csr_w_qry", np.int64), res.debug("csr_w_ref", np.int32), res.debug("csr_w_flags", np.uint8)
    sp_d, sp_best = res.debug("sp_d", DIST_DT), res.debug("sp_best", np.int32)
    kfound, h_cnt, kd = res.debug("kfound", np.int32), res.debug("h_cnt", np.int32), res.debug("kd", DIST_DT)
    contigs = [c for c in range(nC) if rec_off[c + 1] - rec_off[c] > 1 and ctgV[c] > 0]
    vsel = np.concatenate([np.arange(voff[c], voff[c] + ctgV[c]) for c in contigs])
    esel = np.concatenate([np.arange(rowptr[voff[c]], rowptr[voff[c] + ctgV[c]]) for c in contigs])
    n = ctgV[contigs].astype(np.int64)
    g_voff = np.zeros(len(contigs) + 1, np.int64); g_voff[1:] = np.cumsum(n)
    deg = rowptr[vsel + 1] - rowptr[vsel]
    rp = np.zeros(len(vsel) + 1, np.int64); rp[1:] = np.cumsum(deg)
    f = fl[esel].astype(np.int64)
    w = np.stack([wq[esel], wr[esel].astype(np.int64), f & 3, (f >> 2) & 1, (f >> 3) & 1], 1)
    batch = {"g_voff": g_voff, "rowptr": rp, "col": col[esel].astype(np.int32), "w": w, "src": (n - 2).astype(np.int32), "sink": (n - 1).astype(np.int32)}
    d5 = np.stack([sp_d[vsel][f_] .astype(np.int64) for f_ in ("qry", "ref", "anom", "qnz", "qtot")], 1)
    kdc = [np.stack([kd[c * K:c * K + int(kfound[c])][f_].astype(np.int64) for f_ in ("qry", "ref", "anom", "qnz", "qtot")], 1) for c in contigs]
    want = {"kfound": kfound[contigs].astype(np.int64), "h_cnt": h_cnt[contigs].astype(np.int64), "d5": d5, "best": sp_best[vsel].astype(np.int64), "kd": kdc}
    return batch, contigs, want


def compare_pipeline(batch, want, got, K):
    bad = []
    if not np.array_equal(got["n_found"], want["kfound"]):
        bad.append("n_found")
    if not np.array_equal(got["heap_nodes"], want["h_cnt"]):
        bad.append("heap_nodes")
    if "d" in got and not np.array_equal(got["d"], want["d5"]):
        bad.append("d5")
    if "best" in got and not np.array_equal(got["best"].astype(np.int64), want["best"]):
        bad.append("best")
    for i, kd in enumerate(want["kd"]):
        if not np.array_equal(got["dist"][i, :len(kd)], kd):
            bad.append(("dist", i)); break
    if np.any(got["status"] != 0):
        bad.append("status")
    return bad
