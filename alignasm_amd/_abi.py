"""ctypes mirror of include/alignasm_amd.h (ABI version 3).

Plumbing only: no computation lives in Python.  The structs are shared by the product
binding (alignasm_amd.api) and by the test-side loaders of the oracle libraries.
"""
import ctypes as C

import numpy as np

AASM_N_PHASES = 16
PHASE_NAMES = ["sort", "pairs", "edges", "revcsr", "sptree", "fwd", "heap", "enum", "select", "gather", "heap_prep", "topo", "misc", "cs", "final", "chain"]

AASM_OK = 0
AASM_E_INVAL, AASM_E_NODEVICE, AASM_E_HIP, AASM_E_NOMEM = -1, -2, -3, -4
AASM_E_OVERFLOW, AASM_E_INTERNAL, AASM_E_PARSE, AASM_E_IO = -5, -6, -7, -8

# reader flags (aasm_paf_read_opts, aasm_paf_parse_device); AASM_READ_H_*: test hooks of the device reader, 0 in production
AASM_READ_DEVICE_RANGES, AASM_READ_H_WEAK_HASH, AASM_READ_H_FEW_BLOCKS = 1, 0x100, 0x200
# aasm_paf_parse_device_rows: the row columns stay resident (implied by the entry); text is device memory
AASM_READ_ROW_COLS, AASM_READ_TEXT_ON_DEVICE = 2, 4

# int aasm_debug_poison(int byte): (restype, argtypes); 0 = off, 1..255 = the allocators' fill byte, -1 for anything else
DEBUG_POISON_SIG = (C.c_int, [C.c_int])

_IN_ARRAYS = [
    ("ctg_rec_off", np.int64), ("qry_str", np.int64), ("qry_end", np.int64), ("ref_str", np.int64),
    ("ref_end", np.int64), ("qry_total", np.int64), ("ref_chr", np.int32), ("aln_fwd", np.uint8),
    ("map_qul", np.uint8), ("rec_rng_off", np.int64), ("rng_qry_l", np.int64), ("rng_qry_r", np.int64),
    ("rng_ref_l", np.int64),
]


class BatchIn(C.Structure):
    _fields_ = [("n_contigs", C.c_int64), ("n_records", C.c_int64), ("n_ranges", C.c_int64)] + [
        (name, C.c_void_p) for name, _ in _IN_ARRAYS
    ] + [("cs_text", C.c_void_p), ("rec_cs_off", C.c_void_p)]


class Opts(C.Structure):
    _fields_ = [
        ("max_paths", C.c_int32), ("non_skip_linkable", C.c_int32), ("device", C.c_int32),
        ("collect_timing", C.c_int32), ("keep_debug", C.c_int32), ("reserved", C.c_int32 * 3),
    ]


# test hooks in Opts.reserved: the names and values of include/alignasm_amd.h (tests/test_abi.py compares them)
AASM_H0_SEQ_SELECT, AASM_H0_HEAP_MW_ALL, AASM_H0_HEAP_MW_NONE, AASM_H0_ENUM_HEAP, AASM_H0_ENUM_SMALL = 0x1, 0x2, 0x4, 0x8, 0x10
AASM_H0_GRID_ORDER, AASM_H0_CHAIN_MASK, AASM_H0_CHAIN_ALL, AASM_H0_CHAIN_NONE, AASM_H0_CHAIN_HALF = 0x20, 0xC0, 0x40, 0x80, 0xC0
AASM_H0_MW_MASK, AASM_H0_MW_INPUT_ORDER, AASM_H0_MW_SHIFT, AASM_H0_GRAPH_LAUNCHES = 0xFF00, 1, 8, 0x10000
AASM_H2_LAUNCH_FAILURE, AASM_H2_WRAP_DEVICES, AASM_H2_DIRTY_SCAN, AASM_H2_CHAIN_HDR_LOST, AASM_H2_CHAIN_DONE_LOST = 0x1, 0x2, 0x4, 0x8, 0x10
AASM_H2_CHAIN_OWN_QUEUE, AASM_H2_SMALL_ROOT_RING, AASM_H2_SORT_DEPTH_MASK, AASM_H2_SORT_DEPTH_SHIFT = 0x20, 0x40, 0xFF00, 8
HOOK_CONSTANTS = {k: v for k, v in globals().items() if k.startswith(("AASM_H0_", "AASM_H2_"))}
_flag = lambda bits: {False: 0, True: bits}   # noqa: E731
# keyword -> (word of Opts.reserved, {value: its bits}, or None: the value itself); every default is 0
HOOKS = {
    "sequential_select": (0, _flag(AASM_H0_SEQ_SELECT)), "heap_waves": (0, {"auto": 0, "all": AASM_H0_HEAP_MW_ALL, "none": AASM_H0_HEAP_MW_NONE}),
    "enum_heap": (0, _flag(AASM_H0_ENUM_HEAP)), "enum_small": (0, _flag(AASM_H0_ENUM_SMALL)), "grid_order": (0, _flag(AASM_H0_GRID_ORDER)),
    "chain": (0, {"auto": 0, "all": AASM_H0_CHAIN_ALL, "none": AASM_H0_CHAIN_NONE, "half": AASM_H0_CHAIN_HALF}),
    "heap_input_order": (0, _flag(AASM_H0_MW_INPUT_ORDER << AASM_H0_MW_SHIFT)), "heap_block_waves": (0, {n: n << AASM_H0_MW_SHIFT for n in (0, 4, 8, 16)}),
    "graph_launches": (0, _flag(AASM_H0_GRAPH_LAUNCHES)), "test_max_contigs": (1, None),
    "test_inject_launch_failure": (2, _flag(AASM_H2_LAUNCH_FAILURE)), "wrap_devices": (2, _flag(AASM_H2_WRAP_DEVICES)), "test_dirty_scan": (2, _flag(AASM_H2_DIRTY_SCAN)),
    "test_chain_lost": (2, {0: 0, 1: AASM_H2_CHAIN_HDR_LOST, 2: AASM_H2_CHAIN_DONE_LOST}), "chain_own_queue": (2, _flag(AASM_H2_CHAIN_OWN_QUEUE)),
    "test_small_root_ring": (2, _flag(AASM_H2_SMALL_ROOT_RING)), "sort_depth_test": (2, {d: d << AASM_H2_SORT_DEPTH_SHIFT for d in range(256)}),
}


def make_opts(max_paths=10000, non_skip_linkable=False, device=0, timing=False, keep_debug=False, **hooks):
    """Opts of a solve; hooks by the keywords of HOOKS (unknown name: TypeError, unknown value: ValueError)."""
    o = Opts(int(max_paths), 1 if non_skip_linkable else 0, int(device), 1 if timing else 0, 1 if keep_debug else 0)
    for name, value in hooks.items():
        if name not in HOOKS:
            raise TypeError(f"unknown test hook {name!r}")
        word, table = HOOKS[name]
        if table is not None and value not in table:
            raise ValueError(f"test hook {name}={value!r}: not one of {sorted(table, key=str)}")
        o.reserved[word] |= int(value) if table is None else table[value]
    if hooks.get("heap_input_order") and hooks.get("heap_block_waves"):
        raise ValueError("heap_input_order and heap_block_waves set the same field")
    return o


class OutElem(C.Structure):
    _fields_ = [
        ("edited_qry_str", C.c_int64), ("edited_qry_end", C.c_int64), ("edited_ref_str", C.c_int64),
        ("edited_ref_end", C.c_int64), ("ctg_index", C.c_int32), ("is_alt_path", C.c_int32),
    ]


OUT_ELEM_DTYPE = np.dtype(
    [("qs", np.int64), ("qe", np.int64), ("rs", np.int64), ("re", np.int64), ("ctg_index", np.int32), ("is_alt", np.int32)]
)

_STAT_I64 = [
    "n_vertices", "n_pairs", "n_edges", "n_heap_nodes", "n_paths_found", "n_paths_converted",
    "n_unconnectable", "n_internal_errors", "n_single", "range_steps", "device_bytes",
    "ispr_edges", "ispr_vertices", "path_edges", "out_elems", "pq_pushes",
]


class Stats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in _STAT_I64] + [
        ("phase_ms", C.c_float * AASM_N_PHASES), ("total_ms", C.c_float), ("reserved_f", C.c_float * 3),
    ]

    def as_dict(self):
        d = {n: int(getattr(self, n)) for n in _STAT_I64}
        d["phase_ms"] = {PHASE_NAMES[i]: float(self.phase_ms[i]) for i in range(len(PHASE_NAMES))}
        d["total_ms"] = float(self.total_ms)
        return d


class BatchOut(C.Structure):
    _fields_ = [
        ("n_contigs", C.c_int64), ("main_off", C.c_void_p), ("alt_off", C.c_void_p), ("all_path_off", C.c_void_p),
        ("all_elem_off", C.c_void_p), ("main_elems", C.c_void_p), ("alt_elems", C.c_void_p), ("all_elems", C.c_void_p),
        ("n_all_paths", C.c_int64), ("ctg_status", C.c_void_p), ("stats", Stats),
    ]


class OutSizes(C.Structure):
    """aasm_out_sizes: the sizes of a result's arrays (aasm_result_sizes)."""
    _fields_ = [(n, C.c_int64) for n in ("n_contigs", "n_main", "n_alt", "n_all_paths", "n_all_elems")]


class DevOut(C.Structure):
    """aasm_dev_out: caller-owned DEVICE arrays a result is exported into (aasm_result_export)."""
    _fields_ = [(n, C.c_void_p) for n in ("main_off", "alt_off", "all_path_off", "all_elem_off", "main_elems", "alt_elems",
                                          "all_elems", "ctg_status")]


# ---- cut plans (aasm_cut_plans_device / aasm_writer_append_cuts) ----------------------------------------------------------------
AASM_CUT_IS_CUT, AASM_CUT_IRREGULAR = 0x1, 0x2
AASM_CUT_E_TAG, AASM_CUT_E_INS_CLIP, AASM_CUT_E_EDIT, AASM_CUT_E_RECORD = 0x10, 0x20, 0x40, 0x80
AASM_CUT_ERRORS = AASM_CUT_E_TAG | AASM_CUT_E_INS_CLIP | AASM_CUT_E_EDIT | AASM_CUT_E_RECORD


class CutPlan(C.Structure):
    """aasm_cut_plan: what a PAF row needs beyond its element's coordinates (48 bytes)."""
    _fields_ = [("keep_lo", C.c_int64), ("keep_hi", C.c_int64), ("head_keep", C.c_int64), ("tail_keep", C.c_int64),
                ("mat_num", C.c_int32), ("aln_len", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


CUT_DT = np.dtype([("keep_lo", np.int64), ("keep_hi", np.int64), ("head_keep", np.int64), ("tail_keep", np.int64),
                   ("mat_num", np.int32), ("aln_len", np.int32), ("flags", np.int32), ("reserved", np.int32)])


class DevCuts(C.Structure):
    """aasm_dev_cuts: caller-owned DEVICE plan arrays, parallel to DevOut's element lists."""
    _fields_ = [(n, C.c_void_p) for n in ("main", "alt", "all")]


class Cuts(C.Structure):
    """aasm_cuts: HOST plan arrays, parallel to BatchOut's element lists."""
    _fields_ = [("n_main", C.c_int64), ("n_alt", C.c_int64), ("n_all", C.c_int64), ("main", C.c_void_p), ("alt", C.c_void_p), ("all", C.c_void_p)]


# ---- output rows on the device (aasm_rows_sizes_device / aasm_rows_format_device / aasm_writer_append_device) -------------------------
AASM_ROWS_E_PLAN, AASM_ROWS_E_STRETCH, AASM_ROWS_H_FEW_BLOCKS = 0x100, 0x200, 0x200


class RowCols(C.Structure):
    """aasm_row_cols: DEVICE arrays of what an output row prints beyond BatchIn (aasm_paf_upload_rows)."""
    _fields_ = [("n_chr", C.c_int64)] + [(n, C.c_void_p) for n in ("ref_total", "mat_num", "aln_len", "row_index", "cord_type", "names", "ctg_name_off", "chr_name_off")]


class DevRows(C.Structure):
    """aasm_dev_rows: caller-owned DEVICE row offsets, one more entry than DevOut's element lists."""
    _fields_ = [(n, C.c_void_p) for n in ("main_off", "alt_off", "all_off")]


class RowsInfo(C.Structure):
    """aasm_rows_info: what aasm_rows_sizes_device returns."""
    _fields_ = [("bytes", C.c_int64 * 3), ("n_flagged", C.c_int64), ("bad_elem", C.c_int64), ("bad_list", C.c_int32), ("bad_flags", C.c_int32)]


def render_cut(plan, tag):
    """The cs tag of a row from its plan and the record's own tag (both str or both bytes); plans without AASM_CUT_IRREGULAR."""
    if not int(plan["flags"]) & AASM_CUT_IS_CUT:
        return tag
    colon, empty = (":", "") if isinstance(tag, str) else (b":", b"")
    num = (lambda v: str(int(v))) if isinstance(tag, str) else (lambda v: str(int(v)).encode())
    return (tag[:5] + (colon + num(plan["head_keep"]) if plan["head_keep"] else empty) + tag[int(plan["keep_lo"]):int(plan["keep_hi"])]
            + (colon + num(plan["tail_keep"]) if plan["tail_keep"] else empty))


class SynthCfg(C.Structure):
    _fields_ = [
        ("n_contigs", C.c_int64), ("recs_per_contig", C.c_int64), ("seed", C.c_uint64), ("dense", C.c_int32),
        ("heavy_tail", C.c_int32), ("dup_every", C.c_int32), ("reserved", C.c_int32),
    ]


def _np_from(ptr, n, dtype):
    if n <= 0 or not ptr:
        return np.zeros(0, dtype)
    buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype, count=n).copy()


def unpack_out(out: BatchOut):
    """BatchOut -> dict of numpy arrays (copies; the C side can be freed afterwards)."""
    c = int(out.n_contigs)
    main_off = _np_from(out.main_off, c + 1, np.int64)
    alt_off = _np_from(out.alt_off, c + 1, np.int64)
    all_path_off = _np_from(out.all_path_off, c + 1, np.int64)
    npaths = int(out.n_all_paths)
    all_elem_off = _np_from(out.all_elem_off, npaths + 1, np.int64)
    return {
        "n_contigs": c,
        "main_off": main_off,
        "alt_off": alt_off,
        "all_path_off": all_path_off,
        "all_elem_off": all_elem_off,
        "main": _np_from(out.main_elems, int(main_off[-1]) if c else 0, OUT_ELEM_DTYPE),
        "alt": _np_from(out.alt_elems, int(alt_off[-1]) if c else 0, OUT_ELEM_DTYPE),
        "all": _np_from(out.all_elems, int(all_elem_off[-1]) if npaths else 0, OUT_ELEM_DTYPE),
        "status": _np_from(out.ctg_status, c, np.int32),
        "stats": out.stats.as_dict(),
    }


class HostBatch:
    """A batch held in numpy arrays + the BatchIn view pointing at them."""

    def __init__(self, arrays: dict):
        self.arrays = {}
        for name, dt in _IN_ARRAYS:
            self.arrays[name] = np.ascontiguousarray(arrays[name], dtype=dt)
        self.view = BatchIn()
        self.view.n_contigs = len(self.arrays["ctg_rec_off"]) - 1
        self.view.n_records = len(self.arrays["qry_str"])
        self.view.n_ranges = len(self.arrays["rng_qry_l"])
        for name, _ in _IN_ARRAYS:
            setattr(self.view, name, self.arrays[name].ctypes.data)

    @property
    def n_contigs(self):
        return int(self.view.n_contigs)

    @staticmethod
    def from_view(view: BatchIn):
        """Copy a borrowed BatchIn (e.g. from aasm_paf_batch) into numpy arrays."""
        c, r, g = int(view.n_contigs), int(view.n_records), int(view.n_ranges)
        sizes = {
            "ctg_rec_off": c + 1, "qry_str": r, "qry_end": r, "ref_str": r, "ref_end": r, "qry_total": r,
            "ref_chr": r, "aln_fwd": r, "map_qul": r, "rec_rng_off": r + 1, "rng_qry_l": g, "rng_qry_r": g, "rng_ref_l": g,
        }
        return HostBatch({name: _np_from(getattr(view, name), sizes[name], dt) for name, dt in _IN_ARRAYS})

    @staticmethod
    def from_view_range(view: BatchIn, c0, c1):
        """Copy only contigs [c0, c1) of a borrowed BatchIn (offsets rebased to 0)."""
        off = _np_from(view.ctg_rec_off, int(view.n_contigs) + 1, np.int64)
        r0, r1 = int(off[c0]), int(off[c1])
        isz = {n: np.dtype(dt).itemsize for n, dt in _IN_ARRAYS}
        ro = _np_from(view.rec_rng_off + r0 * 8, r1 - r0 + 1, np.int64)
        g0, g1 = int(ro[0]), int(ro[-1])
        out = {"ctg_rec_off": off[c0:c1 + 1] - r0, "rec_rng_off": ro - g0}
        for name, dt in _IN_ARRAYS:
            if name in out:
                continue
            base = getattr(view, name)
            if name.startswith("rng_"):
                out[name] = _np_from(base + g0 * isz[name], g1 - g0, dt)
            else:
                out[name] = _np_from(base + r0 * isz[name], r1 - r0, dt)
        return HostBatch(out)

    def subset(self, contigs):
        """New HostBatch holding only the given contigs (used for sharding and tests)."""
        a = self.arrays
        off = a["ctg_rec_off"]
        rec_idx = np.concatenate([np.arange(off[c], off[c + 1]) for c in contigs]) if len(contigs) else np.zeros(0, np.int64)
        new_off = np.zeros(len(contigs) + 1, np.int64)
        new_off[1:] = np.cumsum([off[c + 1] - off[c] for c in contigs])
        ro = a["rec_rng_off"]
        lens = ro[rec_idx + 1] - ro[rec_idx] if len(rec_idx) else np.zeros(0, np.int64)
        new_ro = np.zeros(len(rec_idx) + 1, np.int64)
        new_ro[1:] = np.cumsum(lens)
        if len(rec_idx):
            rng_idx = np.concatenate([np.arange(ro[r], ro[r + 1]) for r in rec_idx])
        else:
            rng_idx = np.zeros(0, np.int64)
        out = {"ctg_rec_off": new_off, "rec_rng_off": new_ro}
        for name in ("qry_str", "qry_end", "ref_str", "ref_end", "qry_total", "ref_chr", "aln_fwd", "map_qul"):
            out[name] = a[name][rec_idx]
        for name in ("rng_qry_l", "rng_qry_r", "rng_ref_l"):
            out[name] = a[name][rng_idx]
        return HostBatch(out)


# ---- k shortest walks on caller graphs (aasm_k_shortest_walks) ----------------------------------------------------------------
AASM_KSW_WALKS, AASM_KSW_TREE, AASM_KSW_CYCLES, AASM_KSW_NEGATIVE, AASM_KSW_HOOK_ARENA = 0x1, 0x2, 0x4, 0x8, 0x100


class KswOut(C.Structure):
    _fields_ = [("n_graphs", C.c_int64), ("k", C.c_int64)] + [
        (name, C.c_void_p) for name in ("n_found", "dist5", "walk_off", "walk_edges", "d5", "best", "heap_nodes", "status",
                                        "hook_arena", "hook_hroot")
    ]


def graph_inputs(g_voff, rowptr, col, source, sink=None, w5=None, cost=None, scalar_w=False):
    """A graph batch (sssp_dijkstra's layout) as contiguous arrays in the C-ABI's types: (g_voff, rowptr, col, source, sink, w5, cost),
    None for what was not given.  w5 is [E, 5] or flat; with scalar_w a 1-D w is [E] scalar weights, taken as (w, 0, 0, 0, 1),
    which order as w does.  Raises ValueError when an array is shorter than the offsets say; the C side checks the rest."""
    def flat(a, t):
        return None if a is None else np.ascontiguousarray(a, t).reshape(-1)
    g_voff, rowptr, col, source, sink, cost = (flat(g_voff, np.int64), flat(rowptr, np.int64), flat(col, np.int32), flat(source, np.int32),
                                               flat(sink, np.int32), flat(cost, np.int32))
    if w5 is not None:
        w5 = np.asarray(w5, np.int64)
        if scalar_w and w5.ndim == 1:
            z = np.zeros_like(w5)
            w5 = np.stack([w5, z, z, z, z + 1], 1)
        w5 = flat(w5.reshape(-1, 5), np.int64)
    # what the offsets ask for; offsets the C side refuses (not from 0, or decreasing) are left to it: it reads nothing through them
    n_graphs = len(g_voff) - 1
    need = {"source": (source, 1, n_graphs), "sink": (sink, 1, n_graphs)}
    if n_graphs > 0 and g_voff[0] == 0 and (np.diff(g_voff) > 0).all():
        n_vertices = int(g_voff[-1])
        need["rowptr"] = (rowptr, 1, n_vertices + 1)
        if len(rowptr) > n_vertices and rowptr[0] == 0 and (np.diff(rowptr[:n_vertices + 1]) >= 0).all():
            n_edges = int(rowptr[n_vertices])
            need.update(col=(col, 1, n_edges), w5=(w5, 5, n_edges), cost=(cost, 1, n_edges))
    for name, (a, width, n) in need.items():
        if a is not None and len(a) // width < n:
            raise ValueError(f"{name}: {len(a) // width} rows, {n} needed")
    return g_voff, rowptr, col, source, sink, w5, cost


def bellman_ford_outputs(g_voff):
    """The caller's arrays of aasm_sssp_bellman_ford for a batch: d5 [VT, 5], prev [VT], status [G], cycle_off [G + 1], cycle [VT + G]."""
    G, VT = len(g_voff) - 1, int(g_voff[-1])
    return (np.zeros((VT, 5), np.int64), np.zeros(VT, np.int32), np.zeros(G, np.int32), np.zeros(G + 1, np.int64), np.zeros(VT + G, np.int32))


def unpack_cycles(cycle_off, cycle):
    """Per graph its cycle as an int32 array (empty where none was reported)."""
    return [cycle[int(cycle_off[g]):int(cycle_off[g + 1])].copy() for g in range(len(cycle_off) - 1)]


# aasm_topology_sort / aasm_sssp_dag (include/alignasm_amd.h): the entries' argument types in the header's order; every array is
# passed as a pointer.  api.py sets them on the library.
DAG_ARGTYPES = {
    "aasm_topology_sort": [C.c_int64] + [C.c_void_p] * 5 + [C.c_int],      # n_graphs; g_voff, rowptr, col, order, status; device
    "aasm_sssp_dag": [C.c_int64] + [C.c_void_p] * 9 + [C.c_int],           # n_graphs; g_voff, rowptr, col, w5, src, d5, prev, order, status; device
}


class GraphsIn(C.Structure):
    """aasm_graphs_in: a graph batch's arrays (host arrays for aasm_graphs_upload, DEVICE arrays for aasm_graphs_wrap_device and
    in aasm_graphs_view's answer) with their lengths as the caller states them."""
    _fields_ = [("n_graphs", C.c_int64), ("n_vertices", C.c_int64), ("n_edges", C.c_int64)] + [
        (n, C.c_void_p) for n in ("g_voff", "rowptr", "col", "w5", "cost")] + [("lim", C.c_int32), ("reserved", C.c_int32)]


# resident graph batches (include/alignasm_amd.h): (restype, argtypes) in the header's order; handles, structures, arrays and
# streams are all passed as pointers.  api.py sets them on the library.
GRAPHS_SIGS = {
    "aasm_graphs_upload": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),                     # host, device, gb
    "aasm_graphs_wrap_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),    # dev, device, stream, gb
    "aasm_graphs_view": (C.c_int, [C.c_void_p, C.c_void_p]),                                # gb, dev_view
    "aasm_graphs_free": (None, [C.c_void_p]),                                               # gb
    "aasm_sssp_dijkstra_device": (C.c_int, [C.c_void_p] * 5),                               # gb, src, d5, prev, stream
    "aasm_sssp_bellman_ford_device": (C.c_int, [C.c_void_p] * 8),                           # gb, src, d5, prev, status, cycle_off, cycle, stream
    "aasm_topology_sort_device": (C.c_int, [C.c_void_p] * 4),                               # gb, order, status, stream
    "aasm_sssp_dag_device": (C.c_int, [C.c_void_p] * 7),                                    # gb, src, d5, prev, order, status, stream
    "aasm_sssp_dial_device": (C.c_int, [C.c_void_p] * 6),                                   # gb, src, dist, pre, status, stream
}


class KswSizes(C.Structure):
    """aasm_ksw_sizes: what aasm_k_shortest_walks_device returns and aasm_ksw_export_device takes back unchanged."""
    _fields_ = [(n, C.c_int64) for n in ("n_graphs", "n_vertices", "k", "n_walks", "n_walk_edges")] + [("flags", C.c_int32), ("reserved", C.c_int32),
                                                                                                     ("serial", C.c_int64)]


class KswDevOut(C.Structure):
    """aasm_ksw_dev_out: the caller's DEVICE arrays of aasm_ksw_export_device."""
    _fields_ = [(n, C.c_void_p) for n in ("n_found", "found_off", "dist5", "walk_off", "walk_edges", "d5", "best", "heap_nodes", "status")]


# k shortest walks on a resident graph batch (include/alignasm_amd.h): (restype, argtypes) in the header's order.  A table of its
# own: unlike GRAPHS_SIGS' entries these take scalars (k, flags) beside their pointers.  api.py sets them on the library.
KSW_DEVICE_SIGS = {
    "aasm_k_shortest_walks_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),   # gb, source, sink, k, flags, stream, sz
    "aasm_ksw_export_device": (C.c_int, [C.c_void_p] * 4),                                                                       # gb, sz, dst, stream
}


def dag_outputs(g_voff, relax=True):
    """The caller's arrays of aasm_sssp_dag for a batch: d5 [VT, 5], prev [VT], order [VT], status [G]; of aasm_topology_sort
    (relax=False) the last two."""
    G, VT = len(g_voff) - 1, int(g_voff[-1])
    out = (np.zeros(VT, np.int32), np.zeros(G, np.int32))
    return ((np.zeros((VT, 5), np.int64), np.zeros(VT, np.int32)) + out) if relax else out


def ksw_inputs(g_voff, rowptr, col, w, source, sink):
    """k_shortest_walks' arrays (graph_inputs with scalar weights allowed): g_voff, rowptr, col, w5, source, sink."""
    g_voff, rowptr, col, source, sink, w5, _ = graph_inputs(g_voff, rowptr, col, source, sink, w5=w, scalar_w=True)
    return g_voff, rowptr, col, w5, source, sink


def unpack_ksw(out: KswOut, vt, flags):
    """KswOut -> dict of numpy arrays (copies; the C side can be freed afterwards)."""
    g, k = int(out.n_graphs), int(out.k)
    r = {
        "n_found": _np_from(out.n_found, g, np.int64),
        "dist": _np_from(out.dist5, g * k * 5, np.int64).reshape(g, k, 5),
        "heap_nodes": _np_from(out.heap_nodes, g, np.int64),
        "status": _np_from(out.status, g, np.int32),
    }
    if flags & AASM_KSW_WALKS:
        r["walk_off"] = _np_from(out.walk_off, g * k + 1, np.int64)
        r["walk_edges"] = _np_from(out.walk_edges, int(r["walk_off"][-1]), np.int64)
    if flags & AASM_KSW_TREE:
        r["d"] = _np_from(out.d5, vt * 5, np.int64).reshape(vt, 5)
        r["best"] = _np_from(out.best, vt, np.int32)
    if flags & AASM_KSW_HOOK_ARENA:
        r["hook_arena"] = _np_from(out.hook_arena, int(r["heap_nodes"].sum()) * 10, np.int64).reshape(-1, 10)
        r["hook_hroot"] = _np_from(out.hook_hroot, vt, np.int32)
    return r
