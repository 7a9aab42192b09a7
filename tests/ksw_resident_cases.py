"""Shared pieces of the tests of k shortest walks on a resident graph batch (tests/test_ksw_resident_cpu.py,
tests/test_gpu_ksw_resident.py): the emulation's runs (the emw_* entries of tests/host_emul/graphs_emul.cpp, in KC.build_emul's
library), the packed result unpacked into the host entry's layout, the small batches, the sanitizer program's file format."""
import ctypes as C
import subprocess

import numpy as np

import graphs_resident_cases as GR
import ksw_cases as KC
import test_sssp_cpu as TS
from alignasm_amd._abi import (AASM_KSW_CYCLES, AASM_KSW_NEGATIVE, AASM_KSW_TREE, AASM_KSW_WALKS, KswDevOut, KswSizes)

E_INVAL, E_NOMEM, E_OVERFLOW = -1, -4, -5
WT = AASM_KSW_WALKS | AASM_KSW_TREE
MODES = {"dag": 0, "cycles": AASM_KSW_CYCLES, "negative": AASM_KSW_CYCLES | AASM_KSW_NEGATIVE}
GUARD = 0x5EA15EA15EA15EA1                                           # sentinel words round every output array
OUT_TYPES = {"n_found": np.int64, "found_off": np.int64, "dist5": np.int64, "walk_off": np.int64, "walk_edges": np.int64, "d5": np.int64,
             "best": np.int32, "heap_nodes": np.int64, "status": np.int32}


def out_lengths(sz, flags):
    """The stated length of every array of aasm_ksw_dev_out for a solve's sizes (0: not asked for)."""
    G, V, NW, NE = int(sz.n_graphs), int(sz.n_vertices), int(sz.n_walks), int(sz.n_walk_edges)
    ww, wt = bool(flags & AASM_KSW_WALKS), bool(flags & AASM_KSW_TREE)
    return {"n_found": G, "found_off": G + 1, "dist5": 5 * NW, "walk_off": (NW + 1) * ww, "walk_edges": NE * ww, "d5": 5 * V * wt, "best": V * wt,
            "heap_nodes": G, "status": G}


class EmwBatch(GR.EmrBatch):
    """A resident batch of the emulation (batch dict from KC.make_batch: `src` doubles as the sources) with the k-walk entries."""

    def __init__(self, lib, b, wrap):
        super().__init__(lib, dict(b, w=None if b.get("w") is None else np.asarray(b["w"], np.int64).reshape(-1)), wrap)
        self.src = np.ascontiguousarray(b["src"], np.int32)
        self.sink = np.ascontiguousarray(b["sink"], np.int32)

    def solve(self, k, flags, src=None, sink=None, raw=None):
        """-> (rc, KswSizes); raw: replacements for the pointers by name (None = NULL)"""
        P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
        sz = KswSizes()
        args = {"source": P(self.src if src is None else np.ascontiguousarray(src, np.int32)), "sink": P(self.sink if sink is None else np.ascontiguousarray(sink, np.int32)),
                "sz": C.cast(C.byref(sz), C.c_void_p)}
        args.update(raw or {})
        rc = self.lib.emw_solve(self.h, args["source"], args["sink"], C.c_int64(k), int(flags), args["sz"])
        return rc, sz

    def export(self, sz, null=(), odd=()):
        """-> (rc, dict of numpy arrays at their stated lengths).  Every array sits between GUARD words, which must survive.
        null / odd: names of arrays passed as NULL / half an element off their alignment."""
        n = out_lengths(sz, sz.flags)
        bufs = {name: np.full((n[name] * np.dtype(t).itemsize + 7) // 8 + 4, GUARD, np.uint64) for name, t in OUT_TYPES.items()}
        view = {name: bufs[name][2:].view(t)[:n[name]] for name, t in OUT_TYPES.items()}
        dst = KswDevOut(**{name: (None if name in null or not n[name] else view[name].ctypes.data + (np.dtype(t).itemsize // 2 if name in odd else 0))
                           for name, t in OUT_TYPES.items()})
        rc = self.lib.emw_export(self.h, C.byref(sz), C.byref(dst))
        for name, t in OUT_TYPES.items():
            whole, fresh = bufs[name].view(np.uint8), np.full(len(bufs[name]), GUARD, np.uint64).view(np.uint8)
            end = 16 + n[name] * np.dtype(t).itemsize
            assert np.array_equal(whole[:16], fresh[:16]) and np.array_equal(whole[end:], fresh[end:]), name
            if rc != 0:
                assert np.array_equal(whole, fresh), name            # a refused export has written nothing
        return rc, {name: view[name].copy() for name in OUT_TYPES}

    def run(self, k, flags):
        """solve + export -> (sizes, packed dict)"""
        rc, sz = self.solve(k, flags)
        assert rc == 0, (rc, self.lib.emr_last_error())
        rc, o = self.export(sz)
        assert rc == 0 and self.lib.emw_read_bytes() == 0, (rc, self.lib.emr_last_error())
        return sz, o


def unpack(o, G, k, flags):
    """A packed result (numpy arrays by aasm_ksw_dev_out's names) in the layout of _abi.unpack_ksw, the host entry's: dist [G, k, 5]
    (0 beyond n_found), walk_off [G * k + 1] (empty beyond n_found, at the graph's end), walk_edges, d, best."""
    nf, fo = o["n_found"], o["found_off"]
    assert fo[0] == 0 and np.array_equal(np.diff(fo), nf) and (nf >= 0).all() and (nf <= k).all()
    r = {"n_found": nf, "heap_nodes": o["heap_nodes"], "status": o["status"], "dist": np.zeros((G, k, 5), np.int64)}
    d5 = np.asarray(o["dist5"]).reshape(-1, 5)
    assert len(d5) == fo[-1]
    for g in range(G):
        r["dist"][g, :nf[g]] = d5[fo[g]:fo[g + 1]]
    if flags & AASM_KSW_WALKS:
        wo = o["walk_off"]
        assert len(wo) == fo[-1] + 1 and wo[0] == 0 and (np.diff(wo) >= 0).all() and len(o["walk_edges"]) == wo[-1]
        r["walk_off"] = np.zeros(G * k + 1, np.int64)
        for g in range(G):
            r["walk_off"][g * k:g * k + nf[g]] = wo[fo[g]:fo[g + 1]]
            r["walk_off"][g * k + nf[g]:(g + 1) * k] = wo[fo[g + 1]]
        r["walk_off"][G * k] = wo[-1]
        r["walk_edges"] = o["walk_edges"]
    if flags & AASM_KSW_TREE:
        r["d"], r["best"] = np.asarray(o["d5"]).reshape(-1, 5), o["best"]
    return r


def differ(got, want):
    """Keys on which an unpacked result differs from the host entry's (every key of the host entry's but its test hooks)."""
    keys = [key for key in want if not key.startswith("hook_")]
    return [key for key in keys if key not in got or got[key].shape != want[key].shape or not np.array_equal(got[key], want[key])]


def sub_batch(b, gi):
    sub = dict(GR.sub_batch(b, gi), sink=b["sink"][gi:gi + 1])
    return dict(sub, w=np.asarray(sub["w"], np.int64).reshape(-1, 5))   # ([E] would be scalar weights to ksw_inputs)


# ---- batches -------------------------------------------------------------------------------------------------------------
def tiny_graphs(count, seed, loops):
    """Graphs of 1 - 3 vertices and 0 - 5 edges: single vertices, unreachable sinks, source == sink, parallel edges, and with `loops`
    self-loops and two-cycles (AASM_KSW_CYCLES only).  Scalar weights 0 .. 3."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        n = int(rng.integers(1, 4))
        m = int(rng.integers(0, 6)) if n > 1 or loops else 0
        edges = []
        for _ in range(m):
            u, v = (int(x) for x in rng.integers(0, n, 2))
            if not loops:
                if u == v:
                    continue
                u, v = min(u, v), max(u, v)
            edges.append((u, v))
        rows = [[v for u, v in edges if u == x] for x in range(n)]
        rowptr = np.zeros(n + 1, np.int64)
        rowptr[1:] = np.cumsum([len(r) for r in rows])
        col = np.array([v for r in rows for v in r], np.int64)
        s, t = (int(x) for x in rng.integers(0, n, 2))
        if i % 5 == 0:
            t = s
        out.append(KC.graph(n, rowptr, col, rng.integers(0, 4, len(col)), s, t))
    return out


def reversed_heap_retry_graph(m=10):
    """TS.heap_retry_graph with every edge turned round, as a k-walk graph whose SINK is its source: the dijkstra from the sink over
    the reversed graph is the original's, list order included (the reversed lists are in ascending edge id, and the edges are sorted
    by their new tail = the old head), so the tree stage's first round runs out of heap room and the 4x round finishes.  The
    source is the first leaf."""
    n, rp, col, w, src = TS.heap_retry_graph(m)
    w = np.asarray(w).reshape(-1, 5)
    edges = sorted((int(col[e]), u, e) for u in range(n) for e in range(int(rp[u]), int(rp[u + 1])))
    rowptr = np.zeros(n + 1, np.int64)
    for t, _, _ in edges:
        rowptr[t + 1] += 1
    return KC.graph(n, np.cumsum(rowptr), np.array([u for _, u, _ in edges], np.int64), np.stack([w[e] for _, _, e in edges]), 3, src)


# ---- the sanitizer program -------------------------------------------------------------------------------------------------
def san_run(prog, tmp_path, b, k, flags, mode=0):
    """-> (OUT words, stdout) of graphs_emul_san ksw_resident on a batch (b["w"] None: a batch without w5)."""
    t = GR.typed(dict(b, w=None if b.get("w") is None else np.asarray(b["w"], np.int64).reshape(-1)))
    G = len(t["g_voff"]) - 1
    parts = [np.array([G, t["n_vertices"], t["n_edges"], t["w"] is not None, k, flags, mode], np.int64), t["g_voff"], t["rowptr"], t["col"].astype(np.int64)]
    parts += [] if t["w"] is None else [t["w"]]
    parts += [np.asarray(b["src"], np.int64), np.asarray(b["sink"], np.int64)]
    np.concatenate(parts).tofile(tmp_path / "in.bin")
    r = subprocess.run([prog, "ksw_resident", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return np.fromfile(tmp_path / "out.bin", np.int64), r.stdout


def san_expected(sz, o, flags):
    names = ["n_found", "found_off", "dist5", "heap_nodes", "status"] + (["walk_off", "walk_edges"] if flags & AASM_KSW_WALKS else []) + \
            (["d5", "best"] if flags & AASM_KSW_TREE else [])
    return np.concatenate([np.array([0, sz.n_walks, sz.n_walk_edges], np.int64)] + [np.asarray(o[n], np.int64).reshape(-1) for n in names])
