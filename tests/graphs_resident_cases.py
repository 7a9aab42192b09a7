"""Shared pieces of the tests of resident graph batches (tests/test_graphs_resident_cpu.py, tests/test_gpu_graphs_resident.py): the
emulation's runs (the emr_* entries of tests/host_emul/graphs_emul.cpp, in KC.build_emul's library), the single-defect batches, the
seeded mutations, the sanitizer program's file format, and the host entries' answers in the resident entries' shape."""
import ctypes as C

import numpy as np

import ksw_cases as KC
from alignasm_amd._abi import GraphsIn

ROOT = KC.ROOT
E_INVAL, E_OVERFLOW, E_INTERNAL = -1, -5, -6
LIM = 1 << 39
TYPES = {"g_voff": np.int64, "rowptr": np.int64, "col": np.int32, "w": np.int64, "cost": np.int32, "src": np.int32}


# ---- batches -----------------------------------------------------------------------------------------------------------
def typed(b):
    """A batch dict {g_voff, rowptr, col, src, w?, cost?, lim?, n_vertices?, n_edges?} with every array contiguous in its C type; the
    stated lengths default to the arrays' own."""
    out = {k: (None if b.get(k) is None else np.ascontiguousarray(b[k], t).reshape(-1)) for k, t in TYPES.items()}
    out["lim"] = int(b.get("lim", 2))
    out["n_vertices"] = int(b.get("n_vertices", len(out["rowptr"]) - 1))
    out["n_edges"] = int(b.get("n_edges", len(out["col"])))
    return out


def graphs_in(b, ptr=lambda a: a.ctypes.data):
    b = typed(b)
    col = b["col"] if len(b["col"]) else np.zeros(1, np.int32)      # (col must not be NULL)
    P = lambda a: None if a is None else ptr(a)   # noqa: E731
    gi = GraphsIn(len(b["g_voff"]) - 1, b["n_vertices"], b["n_edges"], P(b["g_voff"]), P(b["rowptr"]), P(col), P(b["w"]), P(b["cost"]), b["lim"], 0)
    return gi, (b, col)


def with_cost(batch, seed=1, lim=2):
    """KC.make_batch's dict with random costs 0 .. lim beside its weights."""
    return dict(batch, cost=np.random.default_rng(seed).integers(0, lim + 1, len(batch["col"])).astype(np.int32), lim=lim)


def sub_batch(b, gi):
    """Graph gi of a batch as a batch of its own."""
    v0, v1 = int(b["g_voff"][gi]), int(b["g_voff"][gi + 1])
    rp = np.asarray(b["rowptr"][v0:v1 + 1], np.int64)
    e0, e1 = int(rp[0]), int(rp[-1])
    out = {"g_voff": np.array([0, v1 - v0], np.int64), "rowptr": rp - e0, "col": b["col"][e0:e1], "src": b["src"][gi:gi + 1], "lim": b.get("lim", 2)}
    for k, width in (("w", 5), ("cost", 1)):
        if b.get(k) is not None:
            out[k] = np.asarray(b[k]).reshape(-1)[width * e0:width * e1]
    return out


# ---- the emulation -------------------------------------------------------------------------------------------------------
def emr_verdict(lib, b, wrap):
    """(rc, message) of a creation path; a batch that is accepted is freed again."""
    gi, keep = graphs_in(b)
    h = C.c_void_p()
    rc = lib.emr_graphs_make(C.byref(gi), int(wrap), C.byref(h))
    msg = lib.emr_last_error().decode()
    if rc == 0:
        lib.emr_graphs_free(h)
    return rc, msg


def host_verdict(lib, b):
    gi, keep = graphs_in(b)
    return lib.emr_host_check(C.byref(gi)), lib.emr_last_error().decode()


class EmrBatch:
    """A resident batch of the emulation; wrap: the arrays are borrowed (kept here) and checked by the kernels."""

    def __init__(self, lib, b, wrap):
        self.lib, self.b = lib, typed(b)
        gi, self._keep = graphs_in(self.b)
        self.h = C.c_void_p()
        rc = lib.emr_graphs_make(C.byref(gi), int(wrap), C.byref(self.h))
        assert rc == 0, (rc, lib.emr_last_error())
        self.G, self.V = len(self.b["g_voff"]) - 1, self.b["n_vertices"]

    def close(self):
        self.lib.emr_graphs_free(self.h)

    def run(self, entry, src=None, order=True):
        """-> (rc, dict in GraphBatch's shape)"""
        G, V = self.G, self.V
        P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
        src = None if src is None else np.ascontiguousarray(src, np.int32)
        o = {"d": np.full((V, 5), 77, np.int64), "prev": np.full(V, 77, np.int32), "status": np.full(G, 77, np.int32)}
        if entry == "dijkstra":
            o.pop("status")
            rc = self.lib.emr_dijkstra(self.h, P(src), P(o["d"]), P(o["prev"]))
        elif entry == "bellman_ford":
            o.update(cycle_off=np.full(G + 1, 77, np.int64), cycle=np.full(V + G, 77, np.int32))
            rc = self.lib.emr_bellman_ford(self.h, P(src), P(o["d"]), P(o["prev"]), P(o["status"]), P(o["cycle_off"]), P(o["cycle"]))
        elif entry == "topology_sort":
            o = {"order": np.full(V, 77, np.int32), "status": o["status"]}
            rc = self.lib.emr_topology_sort(self.h, P(o["order"]), P(o["status"]))
        elif entry == "dag":
            if order:
                o["order"] = np.full(V, 77, np.int32)
            rc = self.lib.emr_dag(self.h, P(src), P(o["d"]), P(o["prev"]), P(o.get("order")), P(o["status"]))
        else:
            o = {"dist": np.full(V, 77, np.int64), "pre": np.full(V, 77, np.int64), "status": o["status"]}
            rc = self.lib.emr_dial(self.h, P(src), P(o["dist"]), P(o["pre"]), P(o["status"]))
        return rc, o


def same(got, want):
    """Keys of two result dicts that differ; `cycle` is compared up to cycle_off's end (beyond it nothing is written)."""
    bad = [k for k in want if k != "cycle" and not np.array_equal(got[k], want[k])]
    if "cycle" in want:
        n = int(want["cycle_off"][-1])
        if "cycle_off" not in bad and not np.array_equal(got["cycle"][:n], want["cycle"][:n]):
            bad.append("cycle")
    return bad


# ---- the host entries, in the resident entries' shape --------------------------------------------------------------------
def host_results(call, b, entry):
    """call(name, *arrays) -> the host entry's tuple (api.sssp_* or an emulation's); -> the resident entry's dict."""
    v = (b["g_voff"], b["rowptr"], b["col"])
    if entry == "dijkstra":
        d, prev = call("dijkstra", *v, b["w"], b["src"])
        return {"d": d, "prev": prev}
    if entry == "bellman_ford":
        d, prev, status, cycles = call("bellman_ford", *v, b["w"], b["src"])
        off = np.zeros(len(cycles) + 1, np.int64)
        off[1:] = np.cumsum([len(c) for c in cycles])
        return {"d": d, "prev": prev, "status": status, "cycle_off": off, "cycle": np.concatenate(list(cycles) + [np.zeros(0, np.int32)]).astype(np.int32)}
    if entry == "topology_sort":
        order, status = call("topology_sort", *v)
        return {"order": order, "status": status}
    if entry == "dag":
        d, prev, status, order = call("dag", *v, b["w"], b["src"])
        return {"d": d, "prev": prev, "status": status, "order": order}
    dist, pre = call("dial", *v, b["cost"], b["src"], b.get("lim", 2))
    return {"dist": dist, "pre": pre, "status": np.zeros(len(b["src"]), np.int32)}


def api_call(api):
    fns = {"dijkstra": api.sssp_dijkstra, "bellman_ford": api.sssp_bellman_ford, "topology_sort": api.topology_sort,
           "dag": lambda *a: api.sssp_dag(*a, order=True), "dial": api.sssp_dial}
    return lambda name, *a: fns[name](*a)


# ---- single-defect batches -----------------------------------------------------------------------------------------------
def valid_batch():
    """Five graphs of 3, 5, 2, 5 and 4 vertices with weights and costs (lim 2); every row holds one to three edges but each graph's
    second, which is empty, and the batch's last, which holds two.  The first and the last graph have a bigger neighbour."""
    rng = np.random.default_rng(12)
    gs = []
    for n in (3, 5, 2, 5, 4):
        rows = [[int(x) for x in rng.integers(0, n, 0 if v == 1 else 2 if v == n - 1 else int(rng.integers(1, 4)))] for v in range(n)]
        rp = np.zeros(n + 1, np.int64)
        rp[1:] = np.cumsum([len(r) for r in rows])
        col = np.array([v for r in rows for v in r], np.int64)
        w = np.stack([rng.integers(-9, 9, len(col)), rng.integers(0, 9, len(col)), rng.integers(0, 3, len(col)), rng.integers(0, 2, len(col)),
                      rng.integers(0, 2, len(col))], 1)
        gs.append(KC.graph(n, rp, col, w, int(rng.integers(0, n)), 0))
    return typed(with_cost(KC.make_batch(gs)))


def _set(b, key, index, value, **more):
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in b.items()}
    out[key][index] = value
    out.update(more)
    return out


def defects():
    """[(name, batch)]: a valid batch with ONE defect, each first at index 0 of its array and then at its last index."""
    b = valid_batch()
    G, VT, ET = len(b["g_voff"]) - 1, b["n_vertices"], b["n_edges"]
    out = [("voff_start_1", _set(b, "g_voff", 0, 1)),
           ("voff_equal_first", _set(b, "g_voff", 1, 0)), ("voff_equal_last", _set(b, "g_voff", G, b["g_voff"][G - 1])),
           ("voff_huge_first", _set(b, "g_voff", 1, 1 << 62)), ("voff_huge_last", _set(b, "g_voff", G - 1, 1 << 62)),
           ("voff_end_one_more", _set(b, "g_voff", G, VT + 1)),
           ("rowptr_start_1", _set(b, "rowptr", 0, 1)),
           ("rowptr_decreases_at_0", _set(b, "rowptr", 1, -1)), ("rowptr_decreases_at_last", _set(b, "rowptr", VT, b["rowptr"][VT - 1] - 1)),
           ("rowptr_huge_first", _set(b, "rowptr", 1, 1 << 62)), ("rowptr_huge_last", _set(b, "rowptr", VT - 1, 1 << 62)),
           ("rowptr_negative_first", _set(b, "rowptr", 1, -(1 << 40))), ("rowptr_negative_last", _set(b, "rowptr", VT, -5)),
           ("rowptr_end_one_less", _set(b, "rowptr", VT, ET - 1)),
           ("lim_8", dict(b, lim=8)), ("lim_minus_1", dict(b, lim=-1)), ("lim_int32_max", dict(b, lim=(1 << 31) - 1))]
    sizes = np.diff(b["g_voff"])
    for at, e, g in (("first", 0, 0), ("last", ET - 1, G - 1)):
        out += [(f"head_minus_1_{at}", _set(b, "col", e, -1)), (f"head_is_own_count_{at}", _set(b, "col", e, int(sizes[g]))),
                (f"cost_minus_1_{at}", _set(b, "cost", e, -1)), (f"cost_lim_plus_1_{at}", _set(b, "cost", e, b["lim"] + 1))]
        for word, values in ((0, (LIM, -LIM - 1)), (1, (LIM, -LIM - 1)), (2, (-1, 3)), (3, (-1, 2)), (4, (-1, 2))):
            out += [(f"w5_{word}_is_{v}_{at}", _set(b, "w", 5 * e + word, v)) for v in values]
    assert sizes[0] < sizes[1] and sizes[G - 1] < sizes[G - 2]
    return out


def corners():
    """The w5 domain's corners, just inside: accepted."""
    b = valid_batch()
    ET = b["n_edges"]
    out = []
    for e in (0, ET - 1):
        for w in ((-LIM, LIM - 1, 2, 1, 1), (LIM - 1, -LIM, 0, 0, 0)):
            c = _set(b, "w", 5 * e, w[0])
            c["w"][5 * e:5 * e + 5] = w
            out.append(c)
    return out


def mutate(rng, b):
    """One random mutation of one cell of a valid batch (or of lim): mostly a value near the cell's own, its bounds or the array
    ends, sometimes a huge or a negative one."""
    key = ("g_voff", "rowptr", "col", "w", "cost", "lim")[int(rng.integers(0, 6))]
    near = [-1, 0, 1, 2, 3, 4, 5, 6, 8, b["n_vertices"], b["n_vertices"] + 1, b["n_edges"] - 1, b["n_edges"], b["n_edges"] + 1, LIM, LIM - 1, -LIM, -LIM - 1,
            1 << 62, -(1 << 62)]
    if key == "lim":
        return dict(b, lim=int(rng.integers(-2, 10)))
    a = b[key]
    i = int(rng.choice([0, len(a) - 1, int(rng.integers(0, len(a)))]))
    v = int(a[i]) + int(rng.integers(-2, 3)) if rng.random() < 0.4 else int(near[int(rng.integers(0, len(near)))])
    if a.dtype == np.int32:
        v = max(-(1 << 31), min((1 << 31) - 1, v))
    return _set(b, key, i, v)


def san_input(b, path):
    """The sanitizer program's IN file of a batch: every array at its STATED length."""
    b = typed(b)
    G, NV, NE = len(b["g_voff"]) - 1, b["n_vertices"], b["n_edges"]
    assert len(b["rowptr"]) == NV + 1 and len(b["col"]) == NE
    parts = [np.array([G, NV, NE, b["w"] is not None, b["cost"] is not None, b["lim"]], np.int64), b["g_voff"], b["rowptr"], b["col"].astype(np.int64)]
    parts += [b[k].astype(np.int64) for k in ("w", "cost") if b[k] is not None]
    np.concatenate(parts + [b["src"].astype(np.int64)]).tofile(path)


def san_expected(lib, b):
    """What the sanitizer program writes for an accepted batch, from the emulation library."""
    out = [0]
    for wrap, entries in ((True, ("dijkstra", "bellman_ford")), (False, ("topology_sort",)), (True, ("dag", "dial"))):
        eb = EmrBatch(lib, b, wrap)
        for entry in entries:
            rc, o = eb.run(entry, b["src"])
            out.append(rc)
            if rc == 0:
                if "cycle" in o:
                    o["cycle"] = o["cycle"][:int(o["cycle_off"][-1])]
                out += [x for a in o.values() for x in a.reshape(-1).tolist()]
        eb.close()
    return np.array(out, np.int64)
