"""ctypes binding of libalignasm_amd.so (the C-ABI of include/alignasm_amd.h).

Host-side mirror of the reference's operator boundary for the per-contig path inference
(`solve_ctg_read`, /root/reference/src/paf_data.hpp:193): `solve_batch()` takes the records
of many contigs and returns, per contig, the three lists the reference writes to
`.aln.paf`, `.aln.alt.paf` and `.aln.all.paf`.

There is no CPU fallback: if the shared library is missing the import raises, and every
solve entry point raises `AlignasmError(AASM_E_NODEVICE)` when no MI355X/HIP device is
usable.  The CPU oracle under oracle/ is test infrastructure and is never loaded here.
"""
import ctypes as C
import os

import numpy as np

from ._abi import (DAG_ARGTYPES, GRAPHS_SIGS, KSW_DEVICE_SIGS, GraphsIn, KswDevOut, KswSizes, dag_outputs, AASM_CUT_ERRORS, AASM_CUT_E_RECORD, AASM_E_INVAL, AASM_E_PARSE, AASM_KSW_CYCLES, AASM_KSW_HOOK_ARENA, AASM_KSW_NEGATIVE, AASM_KSW_TREE, AASM_KSW_WALKS, AASM_OK, AASM_READ_TEXT_ON_DEVICE, CUT_DT, DEBUG_POISON_SIG, OUT_ELEM_DTYPE, BatchIn, BatchOut, Cuts, DevCuts, DevOut,
                   DevRows, HostBatch, RowCols, RowsInfo, KswOut, Opts, OutSizes, Stats, SynthCfg, bellman_ford_outputs, graph_inputs, ksw_inputs, unpack_cycles, make_opts, unpack_ksw, unpack_out)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AASM_LIB_OVERRIDE") or os.path.join(_HERE, "libalignasm_amd.so")   # override: diagnostic builds (tools/)


class AlignasmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"alignasm_amd error {code}: {msg}")
        self.code = code


def _torch_hip_runtime():
    """Path of the HIP runtime torch bundles (torch/lib/libamdhip64.so), or None; torch itself is not imported."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return None
    for d in (spec.submodule_search_locations or []) if spec else []:
        p = os.path.join(d, "lib", "libamdhip64.so")
        if os.path.exists(p):
            return p
    return None


def _load():
    # ONE HIP runtime per process, by decision: where torch is installed, the library runs on the HIP runtime torch bundles, not
    # on the ROCm install's it was linked against (both are soname libamdhip64.so.7; the bundled one may be an older minor
    # version - torch 2.10.0+rocm7.0 ships HIP 7.0 beside ROCm 7.2 - which runs the gfx950 code objects unchanged).  The library
    # needs libamdhip64.so.7; torch's libraries need "libamdhip64.so" from their own directory, a name the loader does not match
    # against the soname of a runtime already loaded from the ROCm install, so loading this library first would give a process
    # that later imports torch a second runtime, whose pointers and streams the first does not know.  Loading torch's copy
    # first (by path, global symbols, torch itself not imported) makes it serve both: its soname satisfies the library, and
    # torch's later load of the same file finds it mapped.  torch imported first: the runtime it loaded already serves the
    # library.  No torch installed: the ROCm install's runtime.  INTEGRATION.md, "results on the device".
    rt = _torch_hip_runtime()
    if rt:
        C.CDLL(rt, mode=C.RTLD_GLOBAL)
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP library first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C alignasm_amd/csrc).  alignasm_amd has no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    lib.aasm_last_error.restype = C.c_char_p
    lib.aasm_debug_fetch.restype = C.c_int64
    lib.aasm_debug_counter.restype = C.c_int64
    lib.aasm_debug_poison.restype, lib.aasm_debug_poison.argtypes = DEBUG_POISON_SIG
    lib.aasm_paf_n_contigs.restype = C.c_int64
    lib.aasm_cs_match_ranges.restype = C.c_int64
    lib.aasm_cs_edit.restype = C.c_int64
    # the device reader: (text, len, flags, device, aasm_paf **, aasm_upload **, aasm_batch_in *) / (path, flags, device, ...)
    lib.aasm_paf_parse_device.argtypes = [C.c_char_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.aasm_paf_parse_device.restype = C.c_int
    lib.aasm_paf_read_device.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.aasm_paf_read_device.restype = C.c_int
    # ... with the row columns: one more pointer, aasm_row_cols *; text may be a device address (c_void_p takes bytes and ints)
    lib.aasm_paf_parse_device_rows.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.aasm_paf_parse_device_rows.restype = C.c_int
    lib.aasm_paf_read_device_rows.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.aasm_paf_read_device_rows.restype = C.c_int
    # the --alt merge on a resident batch: (aasm_batch_in *, aasm_row_cols *, text, len, baseline, flags, device, aasm_upload **, aasm_batch_in *, aasm_row_cols *)
    lib.aasm_paf_merge_alt_device.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int64, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.aasm_paf_merge_alt_device.restype = C.c_int
    for name, argtypes in DAG_ARGTYPES.items():                       # aasm_topology_sort, aasm_sssp_dag
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, C.c_int
    for name, (restype, argtypes) in list(GRAPHS_SIGS.items()) + list(KSW_DEVICE_SIGS.items()):   # resident graph batches
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


LIB = _load()

# every symbol include/alignasm_amd.h declares (checked by tests/test_abi.py)
EXPORTED = [
    "aasm_abi_version", "aasm_device_count", "aasm_init", "aasm_last_error", "aasm_solve_batch", "aasm_solve_batch_multi", "aasm_solve_device",
    "aasm_result_stats", "aasm_result_fetch", "aasm_result_free", "aasm_free_out", "aasm_upload_batch", "aasm_upload_free",
    "aasm_contig_costs", "aasm_partition_contigs", "aasm_partition_costs", "aasm_solve_batch_range", "aasm_writer_open", "aasm_writer_append", "aasm_writer_close", "aasm_reserve_workspace", "aasm_sssp_dijkstra", "aasm_sssp_dial", "aasm_sssp_bellman_ford", "aasm_topology_sort", "aasm_sssp_dag", "aasm_debug_fetch", "aasm_debug_counter", "aasm_debug_poison", "aasm_debug_predicates", "aasm_debug_sort_replay", "aasm_paf_read", "aasm_paf_read_opts", "aasm_paf_parse_mem", "aasm_paf_parse_mem_opts", "aasm_paf_merge_alt", "aasm_paf_merge_alt_mem", "aasm_paf_free", "aasm_paf_batch", "aasm_paf_n_contigs",
    "aasm_paf_write_outputs", "aasm_set_host_threads", "aasm_cs_match_ranges", "aasm_cs_edit", "aasm_synth_paf", "aasm_synth_paf_range", "aasm_paf_to_text", "aasm_paf_save",
    "aasm_result_sizes", "aasm_result_export", "aasm_k_shortest_walks", "aasm_ksw_free", "aasm_cut_plans_device", "aasm_writer_append_cuts",
    "aasm_paf_parse_device", "aasm_paf_read_device", "aasm_paf_parse_device_rows", "aasm_paf_read_device_rows",
    "aasm_paf_upload_rows", "aasm_rows_sizes_device", "aasm_rows_format_device", "aasm_writer_append_device", "aasm_paf_merge_alt_device",
    "aasm_graphs_upload", "aasm_graphs_wrap_device", "aasm_graphs_view", "aasm_graphs_free", "aasm_sssp_dijkstra_device",
    "aasm_sssp_bellman_ford_device", "aasm_topology_sort_device", "aasm_sssp_dag_device", "aasm_sssp_dial_device",
    "aasm_k_shortest_walks_device", "aasm_ksw_export_device",
]


def _check(rc):
    if rc != AASM_OK:
        raise AlignasmError(rc, (LIB.aasm_last_error() or b"").decode(errors="replace"))


def set_host_threads(n):
    """Threads of the PAF reader / writers (0 = all); returns the previous setting."""
    return int(LIB.aasm_set_host_threads(int(n)))


def device_count():
    return int(LIB.aasm_device_count())


def sssp_dijkstra(g_voff, rowptr, col, w5, src, device=0):
    """dijkstra() of the reference's solver (k_shortest_walks.hpp:69-87) on the GPU over a batch of graphs.
    Returns (d: [V, 5] int64, prev: [V] int32)."""
    g_voff, rowptr, col, src, _, w5, _ = graph_inputs(g_voff, rowptr, col, src, w5=w5)
    VT = int(g_voff[-1])
    d = np.zeros((VT, 5), np.int64)
    prev = np.zeros(VT, np.int32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(LIB.aasm_sssp_dijkstra(C.c_int64(len(g_voff) - 1), P(g_voff), P(rowptr), P(col), P(w5), P(src), P(d), P(prev), int(device)))
    return d, prev


def sssp_bellman_ford(g_voff, rowptr, col, w5, src, device=0):
    """bellman_ford() of the reference's solver (k_shortest_walks.hpp:91-129) on the GPU over a batch of graphs whose edges may
    have negative score sums.  Returns (d: [V, 5] int64, prev: [V] int32, status: [G] int32, cycles: a list of int32 arrays).
    status 0: d / prev are the reference's vectors; 1: a negative cycle, d is max and prev -1 for that graph and cycles[g] holds
    the closed cycle (first entry == last entry, edge direction, local ids); < 0: an AASM_E_* for that graph alone."""
    g_voff, rowptr, col, src, _, w5, _ = graph_inputs(g_voff, rowptr, col, src, w5=w5)
    d, prev, status, cycle_off, cycle = bellman_ford_outputs(g_voff)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(LIB.aasm_sssp_bellman_ford(C.c_int64(len(g_voff) - 1), P(g_voff), P(rowptr), P(col), P(w5), P(src), P(d), P(prev), P(status),
                                      P(cycle_off), P(cycle), int(device)))
    return d, prev, status, unpack_cycles(cycle_off, cycle)


def topology_sort(g_voff, rowptr, col, device=0):
    """topology_sort() of the reference's solver (k_shortest_walks.hpp:132-156) on the GPU over a batch of graphs in sssp_dijkstra's
    layout.  Returns (order: [V] int32, status: [G] int32).  status 0: order[g_voff[g] ..] is the reference's vector as local ids -
    Kahn's algorithm with a FIFO: the vertices of in-degree 0 in ascending id, then each vertex when its last in-edge is processed.
    status 1: the graph holds a cycle (the reference asserts; with NDEBUG it returns an empty vector) and its order is -1."""
    g_voff, rowptr, col, _, _, _, _ = graph_inputs(g_voff, rowptr, col, None)
    order, status = dag_outputs(g_voff, relax=False)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(LIB.aasm_topology_sort(C.c_int64(len(g_voff) - 1), P(g_voff), P(rowptr), P(col), P(order), P(status), int(device)))
    return order, status


def sssp_dag(g_voff, rowptr, col, w5, src, order=False, device=0):
    """shortest_path_dag() of the reference's solver (k_shortest_walks.hpp:160-175) on the GPU over a batch of DAGs whose edges may
    have negative score sums.  Returns (d: [V, 5] int64, prev: [V] int32, status: [G] int32), and with order=True topology_sort()'s
    vector as a fourth.  status 0: d / prev are the reference's vectors (among equal candidates the first in (Kahn position of the
    tail, list position) stays); 1: the graph holds a cycle, d is max but IDENTITY at src, prev and order are -1."""
    g_voff, rowptr, col, src, _, w5, _ = graph_inputs(g_voff, rowptr, col, src, w5=w5)
    d, prev, od, status = dag_outputs(g_voff)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(LIB.aasm_sssp_dag(C.c_int64(len(g_voff) - 1), P(g_voff), P(rowptr), P(col), P(w5), P(src), P(d), P(prev), P(od) if order else None,
                             P(status), int(device)))
    return (d, prev, status, od) if order else (d, prev, status)


def k_shortest_walks(g_voff, rowptr, col, w, source, sink, k, walks=True, tree=False, device=0, _hooks=0, cycles=False, negative=False):
    """k_shortest_walks(source, sink, k) of the reference's solver with is_dag = true, and every walk recovered
    (k_shortest_walks.hpp:177-290), on the GPU over a batch of DAGs in sssp_dijkstra's layout.  w: [E, 5] int64
    {qry_score, ref_score, anom, qul_nonzero, qul_total} or [E] (scalar weights, taken as (w, 0, 0, 0, 1)).
    Returns a dict of numpy arrays: n_found [G], dist [G, k, 5], status [G] (0, or AASM_E_INVAL for a graph with a cycle),
    heap_nodes [G]; with walks, walk_off [G * k + 1] and walk_edges (caller CSR positions, source -> sink, walk g * k + i
    at walk_edges[walk_off[g * k + i]:walk_off[g * k + i + 1]]); with tree, d [V, 5] and best [V] (local ids).
    cycles=True solves every graph as the solver does with is_dag = false (the tree of dijkstra() from the sink): graphs may
    hold cycles, and walks may repeat vertices and pass through the sink.  status is then AASM_E_OVERFLOW for a graph that
    meets one of the limits include/alignasm_amd.h lists (a cycle that improves a distance for ever, distances out of range,
    more than 2^28 walk edges) and AASM_E_INVAL for one whose best[] is no tree into the sink.
    negative=True accepts edges whose score sum is negative; with cycles=True the tree is then the one bellman_ford() leaves
    (negative_edge = true), and a graph with a negative cycle gets AASM_E_INVAL and no walks."""
    g_voff, rowptr, col, w5, source, sink = ksw_inputs(g_voff, rowptr, col, w, source, sink)
    flags = (AASM_KSW_WALKS if walks else 0) | (AASM_KSW_TREE if tree else 0) | (AASM_KSW_CYCLES if cycles else 0) | (AASM_KSW_NEGATIVE if negative else 0) | int(_hooks)
    out = KswOut()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = LIB.aasm_k_shortest_walks(C.c_int64(len(g_voff) - 1), P(g_voff), P(rowptr), P(col), P(w5), P(source), P(sink), C.c_int64(int(k)),
                                   int(flags), int(device), C.byref(out))
    _check(rc)
    try:
        return unpack_ksw(out, int(g_voff[-1]), flags)
    finally:
        LIB.aasm_ksw_free(C.byref(out))


def sssp_dial(g_voff, rowptr, col, cost, src, lim=2, device=0):
    """k_weighted_bfs() of the reference (Dial's bucketed BFS, k_weighted_bfs.hpp:16-37) on the GPU over a batch of digraphs.
    Returns (dist: [V] int64, -1 = unreachable; pre: [V] int64 local ids, -1 = none)."""
    g_voff, rowptr, col, src, _, _, cost = graph_inputs(g_voff, rowptr, col, src, cost=cost)
    VT = int(g_voff[-1])
    dist, pre = np.zeros(VT, np.int64), np.zeros(VT, np.int64)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    _check(LIB.aasm_sssp_dial(C.c_int64(len(g_voff) - 1), P(g_voff), P(rowptr), P(col), P(cost), P(src), int(lim), P(dist), P(pre), int(device)))
    return dist, pre


class GraphResult(dict):
    """What GraphBatch's methods return: a dict of torch tensors on the device, by the host entries' names; torch_to_numpy knows it."""


class GraphBatch:
    """A checked graph batch (sssp_dijkstra's layout) resident on one device: the five graph entries over it take their sources and
    leave their results on the device, without the checks, the upload and the download of a host-pointer call.  The methods return
    GraphResult dicts of torch tensors in the host entries' shapes - word for word what sssp_dijkstra / sssp_bellman_ford / topology_sort /
    sssp_dag / sssp_dial return for the same graphs and sources (bellman_ford's cycles packed as cycle_off / cycle; dial with a
    status per graph) - made on the current torch stream of the device (or stream=) and tied to it with record_stream;
    torch_to_numpy brings such a dict to the host.  src: a numpy array (uploaded on that stream) or a contiguous int32 device
    tensor that is ready on it.  dijkstra waits for its result; the others return once their sources are checked."""

    def __init__(self, handle, device, keep=None):
        self._h, self.device, self._keep = handle, int(device), keep
        v = GraphsIn()
        _check(LIB.aasm_graphs_view(self._h, C.byref(v)))
        self.dev_view, self.n_graphs, self.n_vertices, self.n_edges = v, int(v.n_graphs), int(v.n_vertices), int(v.n_edges)

    @classmethod
    def upload(cls, g_voff, rowptr, col, w5=None, cost=None, lim=2, device=0):
        """From numpy arrays (aasm_graphs_upload: checked on the host, copied).  w5 / cost: what the batch will be asked for -
        dijkstra, bellman_ford and dag need w5, dial needs cost (0 .. lim <= 7)."""
        g_voff, rowptr, col, _, _, w5, cost = graph_inputs(g_voff, rowptr, col, None, w5=w5, cost=cost)
        P = lambda a: None if a is None else a.ctypes.data   # noqa: E731
        ne = len(col)
        if not ne:                                                   # (col must not be NULL)
            col = np.zeros(1, np.int32)
        gi = GraphsIn(len(g_voff) - 1, len(rowptr) - 1, ne, P(g_voff), P(rowptr), P(col), P(w5), P(cost), int(lim), 0)
        h = C.c_void_p()
        _check(LIB.aasm_graphs_upload(C.byref(gi), int(device), C.byref(h)))
        return cls(h, device)

    @classmethod
    def from_torch(cls, g_voff, rowptr, col, w5=None, cost=None, lim=2):
        """Over contiguous tensors that are already on a device (aasm_graphs_wrap_device): g_voff, rowptr int64, col int32, w5 int64
        [E, 5] or flat, cost int32.  The tensors are borrowed - never written; the batch keeps references, and they must stay
        unchanged while it lives - and checked on the device.  The tensors' current stream is waited for first."""
        import torch
        _check_one_hip_runtime()
        want = (("g_voff", g_voff, torch.int64), ("rowptr", rowptr, torch.int64), ("col", col, torch.int32), ("w5", w5, torch.int64), ("cost", cost, torch.int32))
        for name, t, dt in want:
            if t is not None and (not t.is_cuda or t.dtype != dt or not t.is_contiguous() or t.device != g_voff.device):
                raise AlignasmError(AASM_E_INVAL, f"from_torch: {name} must be a contiguous {dt} tensor on the batch's device")
        device = g_voff.device.index if g_voff.device.index is not None else torch.cuda.current_device()
        stream = torch.cuda.current_stream(device)
        stream.synchronize()
        ne = int(col.numel())
        if (w5 is not None and w5.numel() != 5 * ne) or (cost is not None and cost.numel() != ne):
            raise ValueError("from_torch: w5 needs 5 words and cost one word per entry of col")
        P = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        keep = [g_voff, rowptr, col, w5, cost]
        if not ne:                                                   # (an empty tensor has no address; col must not be NULL)
            keep.append(torch.zeros(1, dtype=torch.int32, device=g_voff.device))
        gi = GraphsIn(int(g_voff.numel()) - 1, int(rowptr.numel()) - 1, ne, P(g_voff), P(rowptr), P(col) if ne else keep[-1].data_ptr(), P(w5) if ne else None,
                      P(cost) if ne else None, int(lim), 0)
        if not ne:                                                   # (what the batch may be asked for is kept: empty arrays of their own)
            gi.w5 = keep[-1].data_ptr() if w5 is not None else None
            gi.cost = keep[-1].data_ptr() if cost is not None else None
        h = C.c_void_p()
        _check(LIB.aasm_graphs_wrap_device(C.byref(gi), int(device), C.c_void_p(stream.cuda_stream or 0), C.byref(h)))
        return cls(h, device, keep)

    def _begin(self, src, stream):
        import torch
        _check_one_hip_runtime()
        if not self._h:
            raise AlignasmError(AASM_E_INVAL, "the graph batch is closed")
        dev = torch.device("cuda", self.device)
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        if src is not None and not isinstance(src, torch.Tensor):
            src = np.ascontiguousarray(src, np.int32).reshape(-1)
            if len(src) != self.n_graphs:
                raise ValueError(f"src: {len(src)} entries, {self.n_graphs} needed")
            with torch.cuda.device(dev), torch.cuda.stream(stream):
                src = torch.from_numpy(src).to(dev)
        elif src is not None and (not src.is_cuda or src.dtype != torch.int32 or not src.is_contiguous() or src.numel() != self.n_graphs):
            raise AlignasmError(AASM_E_INVAL, "src must be a contiguous int32 device tensor with one entry per graph")
        if src is not None:
            src.record_stream(stream)

        def empty(shape, dtype):
            with torch.cuda.device(dev), torch.cuda.stream(stream):
                t = torch.empty(shape, dtype=dtype, device=dev)
            t.record_stream(stream)                                  # (the caching allocator hands a freed block to other work)
            return t
        return torch, src, stream, empty

    @staticmethod
    def _p(t):
        return None if t is None or not t.numel() else t.data_ptr()

    def dijkstra(self, src, stream=None):
        """-> {"d": [V, 5] int64, "prev": [V] int32}; waits for the result (its heap room grows while a graph runs out of it)."""
        torch, src, stream, empty = self._begin(src, stream)
        d, prev = empty((self.n_vertices, 5), torch.int64), empty(self.n_vertices, torch.int32)
        _check(LIB.aasm_sssp_dijkstra_device(self._h, self._p(src), self._p(d), self._p(prev), stream.cuda_stream or None))
        return GraphResult(d=d, prev=prev)

    def bellman_ford(self, src, stream=None):
        """-> {"d", "prev", "status": [G] int32, "cycle_off": [G + 1] int64, "cycle": [V + G] int32}: graph g's closed cycle (status 1)
        is cycle[cycle_off[g]:cycle_off[g + 1]]; the list is packed on the device, and cycle beyond cycle_off[G] is not written."""
        torch, src, stream, empty = self._begin(src, stream)
        G, V = self.n_graphs, self.n_vertices
        out = GraphResult({"d": empty((V, 5), torch.int64), "prev": empty(V, torch.int32), "status": empty(G, torch.int32), "cycle_off": empty(G + 1, torch.int64),
                           "cycle": empty(V + G, torch.int32)})
        _check(LIB.aasm_sssp_bellman_ford_device(self._h, self._p(src), *(self._p(out[k]) for k in ("d", "prev", "status", "cycle_off", "cycle")),
                                                 stream.cuda_stream or None))
        return out

    def topology_sort(self, stream=None):
        """-> {"order": [V] int32, "status": [G] int32}."""
        torch, _, stream, empty = self._begin(None, stream)
        out = GraphResult(order=empty(self.n_vertices, torch.int32), status=empty(self.n_graphs, torch.int32))
        _check(LIB.aasm_topology_sort_device(self._h, self._p(out["order"]), self._p(out["status"]), stream.cuda_stream or None))
        return out

    def dag(self, src, order=False, stream=None):
        """-> {"d", "prev", "status"}, and with order=True "order"."""
        torch, src, stream, empty = self._begin(src, stream)
        G, V = self.n_graphs, self.n_vertices
        out = GraphResult(d=empty((V, 5), torch.int64), prev=empty(V, torch.int32), status=empty(G, torch.int32))
        if order:
            out["order"] = empty(V, torch.int32)
        _check(LIB.aasm_sssp_dag_device(self._h, self._p(src), self._p(out["d"]), self._p(out["prev"]), self._p(out.get("order")), self._p(out["status"]),
                                        stream.cuda_stream or None))
        return out

    def dial(self, src, stream=None):
        """-> {"dist": [V] int64, "pre": [V] int64, "status": [G] int32 (0; AASM_E_INTERNAL for a bucket overflow, which must not happen)}."""
        torch, src, stream, empty = self._begin(src, stream)
        out = GraphResult(dist=empty(self.n_vertices, torch.int64), pre=empty(self.n_vertices, torch.int64), status=empty(self.n_graphs, torch.int32))
        _check(LIB.aasm_sssp_dial_device(self._h, self._p(src), self._p(out["dist"]), self._p(out["pre"]), self._p(out["status"]), stream.cuda_stream or None))
        return out

    def k_shortest_walks(self, source, sink, k, walks=True, tree=False, cycles=False, negative=False, stream=None):
        """k_shortest_walks (the host entry of that name: its flags, statuses and limits) over the batch, which must carry w5; source,
        sink: numpy arrays or contiguous int32 device tensors, one entry per graph.  -> tensors packed by n_found, never padded to k:
        {"n_found": [G], "found_off": [G + 1] (its prefix sums), "dist5": [n_walks, 5], "heap_nodes": [G], "status": [G] int32}; with
        walks, "walk_off": [n_walks + 1] and "walk_edges" (caller CSR positions, source -> sink); with tree, "d5": [V, 5] and "best": [V].
        Walk i of graph g is walk found_off[g] + i; it equals walk g * k + i of api.k_shortest_walks.  The solve waits for its sizes (a
        few words read back, whatever G is); the export into the tensors is enqueued on the stream."""
        sz = self.ksw_solve(source, sink, k, walks=walks, tree=tree, cycles=cycles, negative=negative, stream=stream)
        return self.ksw_export(sz, stream=stream)

    def ksw_solve(self, source, sink, k, walks=True, tree=False, cycles=False, negative=False, stream=None):
        """The first half of k_shortest_walks (aasm_k_shortest_walks_device): -> KswSizes, final when it returns.  The result stays in
        the batch's working memory until the next call on the batch other than ksw_export."""
        _, source, stream, _ = self._begin(source, stream)
        sink = self._begin(sink, stream)[1]
        flags = (AASM_KSW_WALKS if walks else 0) | (AASM_KSW_TREE if tree else 0) | (AASM_KSW_CYCLES if cycles else 0) | (AASM_KSW_NEGATIVE if negative else 0)
        sz = KswSizes()
        _check(LIB.aasm_k_shortest_walks_device(self._h, self._p(source), self._p(sink), int(k), flags, stream.cuda_stream or None, C.byref(sz)))
        return sz

    def ksw_export(self, sz, stream=None):
        """The second half (aasm_ksw_export_device): tensors allocated from the sizes, the export into them enqueued on the stream.
        May be called again for the same solve; AlignasmError(AASM_E_INVAL) once another call has taken the working memory."""
        torch, _, stream, empty = self._begin(None, stream)
        G, V, NW = self.n_graphs, self.n_vertices, int(sz.n_walks)
        out = GraphResult(n_found=empty(G, torch.int64), found_off=empty(G + 1, torch.int64), dist5=empty((NW, 5), torch.int64),
                          heap_nodes=empty(G, torch.int64), status=empty(G, torch.int32))
        if sz.flags & AASM_KSW_WALKS:
            out.update(walk_off=empty(NW + 1, torch.int64), walk_edges=empty(int(sz.n_walk_edges), torch.int64))
        if sz.flags & AASM_KSW_TREE:
            out.update(d5=empty((V, 5), torch.int64), best=empty(V, torch.int32))
        dst = KswDevOut(**{name: self._p(out.get(name)) for name, _ in KswDevOut._fields_})
        _check(LIB.aasm_ksw_export_device(self._h, C.byref(sz), C.byref(dst), stream.cuda_stream or None))
        return out

    def close(self):
        """Waits for the batch's work in flight, then frees what it owns (borrowed tensors are only released)."""
        if self._h:
            LIB.aasm_graphs_free(self._h)
            self._h = None
            self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def debug_counter(name):
    """Process-wide diagnostic counter: "range_splits", "device_mallocs", "stream_syncs", "read_slow_rows", "read_host_fallbacks", "read_containers"."""
    return int(LIB.aasm_debug_counter(name.encode()))


def debug_poison(byte):
    """Process-wide debug switch: 0 = off (production); 1..255 = the byte the workspace arena (whole, at the start of every
    device solve), the generic graph entries' blocks and the device reader's blocks are filled with before use, so that a
    kernel reading a never-written cell meets it.  Returns the previous value; -1 (nothing changed) outside 0..255."""
    return int(LIB.aasm_debug_poison(int(byte)))


def reserve_workspace(device=0, nbytes=0):
    """Create the device context and grow its workspace arena to `nbytes` ahead of the first solve (a fresh process
    otherwise pays HIP's start-up and the arena's hipMalloc calls inside it).  Returns the C-ABI code (0 = ok;
    AASM_E_NOMEM only means the solve will allocate for itself)."""
    return int(LIB.aasm_reserve_workspace(C.c_int(int(device)), C.c_int64(int(nbytes))))


class Paf:
    """Parsed (or synthesised) PAF file held by the library."""

    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def read(path, device_ranges=False):
        """device_ranges: leave the cs -> match-range conversion to the GPU (AASM_READ_DEVICE_RANGES)."""
        h = C.c_void_p()
        _check(LIB.aasm_paf_read_opts(os.fsencode(path), 1 if device_ranges else 0, C.byref(h)))
        return Paf(h)

    @staticmethod
    def parse(text: bytes, device_ranges=False):
        h = C.c_void_p()
        _check(LIB.aasm_paf_parse_mem_opts(text, C.c_int64(len(text)), 1 if device_ranges else 0, C.byref(h)))
        return Paf(h)

    @staticmethod
    def synth(n_contigs, recs_per_contig, seed, dense=False, heavy_tail=False, dup_every=0, shuffle=False, no_cs=False,
              first=0, count=None, records_only=False):
        """The synthetic file (n_contigs, ...), or its contigs [first, first + count); records_only: no match ranges / cs
        tags (enough for the contig cost model that cuts the file into shards)."""
        cfg = SynthCfg(n_contigs, recs_per_contig, seed, 1 if dense else 0, 1 if heavy_tail else 0, dup_every,
                       (1 if shuffle else 0) | (2 if no_cs else 0) | (4 if records_only else 0))
        h = C.c_void_p()
        if first == 0 and count is None:
            _check(LIB.aasm_synth_paf(C.byref(cfg), C.byref(h)))
        else:
            _check(LIB.aasm_synth_paf_range(C.byref(cfg), C.c_int64(int(first)), C.c_int64(int(n_contigs - first if count is None else count)), C.byref(h)))
        return Paf(h)

    @staticmethod
    def parse_device(text: bytes, device=0, _flags=0, container=True):
        """The device reader (aasm_paf_parse_device): PAF text in host memory -> (Paf, DeviceBatch).  The rows are framed and parsed
        on the GPU; the batch is resident in its cs form, as DeviceBatch(Paf.parse(text, device_ranges=True)) would leave it, and
        the Paf equals that parse.  _flags: AASM_READ_H_WEAK_HASH, AASM_READ_H_FEW_BLOCKS (tests).
        container=False (aasm_paf_parse_device_rows without a container): -> (None, DeviceBatch); the batch carries its row columns
        and names on the device (row_cols()), so to_torch(cuts=db, rows=True) and db.write_outputs work without a Paf."""
        if not container:
            return None, DeviceBatch._read_rows(lambda *out: LIB.aasm_paf_parse_device_rows(C.cast(C.c_char_p(text), C.c_void_p), len(text), int(_flags), int(device), None, *out), device)
        h, up, view = C.c_void_p(), C.c_void_p(), BatchIn()
        _check(LIB.aasm_paf_parse_device(text, len(text), int(_flags), int(device), C.byref(h), C.byref(up), C.byref(view)))
        paf = Paf(h)
        return paf, DeviceBatch._from_upload(up, view, device, paf)

    @staticmethod
    def read_device(path, device=0, _flags=0, container=True):
        """parse_device on a file (aasm_paf_read_device / aasm_paf_read_device_rows: the file is mapped, not copied)."""
        if not container:
            return None, DeviceBatch._read_rows(lambda *out: LIB.aasm_paf_read_device_rows(os.fsencode(path), int(_flags), int(device), None, *out), device)
        h, up, view = C.c_void_p(), C.c_void_p(), BatchIn()
        _check(LIB.aasm_paf_read_device(os.fsencode(path), int(_flags), int(device), C.byref(h), C.byref(up), C.byref(view)))
        paf = Paf(h)
        return paf, DeviceBatch._from_upload(up, view, device, paf)

    def merge_alt(self, text: bytes, alt_baseline=0.5):
        """--alt: merge a second PAF (sub-contig re-alignments), alignasm.cpp:186-332."""
        _check(LIB.aasm_paf_merge_alt_mem(self._h, text, C.c_int64(len(text)), C.c_double(alt_baseline)))

    @property
    def n_contigs(self):
        return int(LIB.aasm_paf_n_contigs(self._h))

    def view(self) -> BatchIn:
        v = BatchIn()
        _check(LIB.aasm_paf_batch(self._h, C.byref(v)))
        return v

    def batch(self) -> HostBatch:
        return HostBatch.from_view(self.view())

    def to_text(self) -> bytes:
        p = C.c_void_p()
        n = C.c_int64()
        _check(LIB.aasm_paf_to_text(self._h, C.byref(p), C.byref(n)))
        try:
            return C.string_at(p, n.value)
        finally:
            C.CDLL(None).free(p)

    def save(self, path):
        """Write the batch as PAF text (rows with cs tags) to `path`."""
        _check(LIB.aasm_paf_save(self._h, os.fsencode(path)))

    def write_outputs(self, out: BatchOut, main_path, alt_path, all_path, cuts=None):
        """The three output files.  cuts: {"main", "alt", "all"} -> numpy CUT_DT arrays parallel to out's element lists (cut plans
        fetched from the device, cuts_to_numpy): the rows are written from them (aasm_writer_append_cuts), byte for byte the same."""
        if cuts is None:
            _check(LIB.aasm_paf_write_outputs(self._h, C.byref(out), os.fsencode(main_path), os.fsencode(alt_path), os.fsencode(all_path)))
            return
        arr = [np.ascontiguousarray(cuts[k], dtype=CUT_DT) for k in ("main", "alt", "all")]
        cs = Cuts(*(len(a) for a in arr), *(a.ctypes.data if len(a) else None for a in arr))
        w = C.c_void_p()
        _check(LIB.aasm_writer_open(os.fsencode(main_path), os.fsencode(alt_path), os.fsencode(all_path), C.byref(w)))
        rc = LIB.aasm_writer_append_cuts(w, self._h, C.byref(out), C.byref(cs), C.c_int64(0))
        msg = (LIB.aasm_last_error() or b"").decode(errors="replace")
        rc2 = LIB.aasm_writer_close(w, 1 if rc == AASM_OK else 0)     # (a failed append leaves no file behind)
        if rc != AASM_OK:
            raise AlignasmError(rc, msg)
        _check(rc2)

    def write_outputs_device(self, db, res, main_path, alt_path, all_path, piece_bytes=0):
        """The three output files with the rows formatted on the device (aasm_writer_append_device).  db: the DeviceBatch of this
        container (its tags on the device); res: a DeviceResult solved from it, or the dict of its to_torch(cuts=db).  Errors as
        write_outputs: a row that cannot be formatted raises with the host codec's code and message and leaves no file behind."""
        _write_outputs_device(self, db, res, main_path, alt_path, all_path, piece_bytes)

    def close(self):
        if self._h:
            LIB.aasm_paf_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _write_outputs_device(paf, db, res, main_path, alt_path, all_path, piece_bytes):
    """aasm_writer_append_device in a session of its own; paf: the container, or None for a batch that has none."""
    d = res if isinstance(res, dict) else res.to_torch(cuts=db)
    if "main_cut" not in d:
        raise AlignasmError(AASM_E_INVAL, "write_outputs_device: the result dict holds no cut plans (to_torch(cuts=...))")
    sizes, dst, dc = _dev_structs(d)
    cols = db.row_cols()
    w = C.c_void_p()
    _check(LIB.aasm_writer_open(os.fsencode(main_path), os.fsencode(alt_path), os.fsencode(all_path), C.byref(w)))
    import torch
    torch.cuda.synchronize(db.device)                                # (the writer runs on the library's own streams)
    rc = LIB.aasm_writer_append_device(w, paf._h if paf is not None else None, C.byref(db.dev_view), C.byref(cols), C.byref(sizes), C.byref(dst), C.byref(dc),
                                       C.c_int64(0), C.c_int64(int(piece_bytes)), int(db.device))
    msg = (LIB.aasm_last_error() or b"").decode(errors="replace")
    rc2 = LIB.aasm_writer_close(w, 1 if rc == AASM_OK else 0)         # (a failed append leaves no file behind)
    if rc != AASM_OK:
        raise AlignasmError(rc, msg)
    _check(rc2)


def solve_batch_raw(view: BatchIn, opts: Opts) -> BatchOut:
    out = BatchOut()
    _check(LIB.aasm_solve_batch(C.byref(view), C.byref(opts), C.byref(out)))
    return out


def free_out(out: BatchOut):
    LIB.aasm_free_out(C.byref(out))


def solve_batch(batch, max_paths=10000, non_skip_linkable=False, device=0, timing=False, n_devices=1, **hooks):
    """solve_ctg_read over a batch (HostBatch or Paf).  Returns a dict of numpy arrays.  hooks: _abi.HOOKS."""
    view = batch.view if isinstance(batch, HostBatch) else batch.view()
    opts = make_opts(max_paths, non_skip_linkable, device, timing, False, **hooks)
    if n_devices > 1:
        out = BatchOut()
        _check(LIB.aasm_solve_batch_multi(C.byref(view), C.byref(opts), int(n_devices), C.byref(out)))
    else:
        out = solve_batch_raw(view, opts)
    try:
        return unpack_out(out)
    finally:
        free_out(out)


class DeviceBatch:
    """A batch uploaded once to HBM; solve() can then be timed without PCIe traffic."""

    def __init__(self, batch, device=0, cs_only=False):
        """cs_only: upload the batch in its cs form - the cs text and no match ranges, as a Paf read with device_ranges - also
        when the batch holds match ranges as well (a synthetic Paf): the solve derives them on the GPU, and the tags are on the
        device for DeviceResult.to_torch(cuts=...)."""
        view = batch.view if isinstance(batch, HostBatch) else batch.view()
        if cs_only:
            if not view.cs_text or not view.rec_cs_off:
                raise AlignasmError(AASM_E_INVAL, "cs_only: the batch holds no cs text")
            view = BatchIn.from_buffer_copy(view)
            view.rng_qry_l = view.rng_qry_r = view.rng_ref_l = None
        self._keep = batch
        self.device = device
        self._up = C.c_void_p()
        self.dev_view = BatchIn()
        _check(LIB.aasm_upload_batch(C.byref(view), int(device), C.byref(self._up), C.byref(self.dev_view)))
        self.n_contigs = int(view.n_contigs)
        self.n_records = int(view.n_records)

    @classmethod
    def _from_upload(cls, up, dev_view, device, keep=None):
        """A batch some other entry left on the device (the device reader): the upload handle and its view."""
        self = object.__new__(cls)
        self._keep, self.device, self._up, self.dev_view = keep, device, up, dev_view
        self.n_contigs, self.n_records = int(dev_view.n_contigs), int(dev_view.n_records)
        return self

    @classmethod
    def _read_rows(cls, call, device):
        """A batch read by aasm_paf_*_device_rows without a container: call(up, view, cols) -> code.  One handle owns the batch's
        arrays and the row columns'."""
        up, view, cols = C.c_void_p(), BatchIn(), RowCols()
        _check(call(C.byref(up), C.byref(view), C.byref(cols)))
        self = cls._from_upload(up, view, device)
        self._row_cols = cols
        return self

    @classmethod
    def from_device_text(cls, tensor, _flags=0):
        """PAF text that is already on the device -> a resident batch with its row columns (aasm_paf_parse_device_rows with
        AASM_READ_TEXT_ON_DEVICE, no container).  tensor: a 1-D contiguous uint8 torch tensor on a GPU whose first byte is 16-byte
        aligned; it is neither copied nor written, and may be freed after the call.  The tensor's current stream is waited for
        first: what was enqueued there to write the text has finished before the reader looks at it."""
        import torch
        _check_one_hip_runtime()
        if tensor.dtype != torch.uint8 or tensor.dim() != 1 or not tensor.is_cuda or not tensor.is_contiguous():
            raise AlignasmError(AASM_E_INVAL, "from_device_text: a 1-D contiguous uint8 tensor on the device is needed")
        device = tensor.device.index if tensor.device.index is not None else torch.cuda.current_device()
        torch.cuda.current_stream(device).synchronize()
        n = int(tensor.numel())
        return cls._read_rows(lambda *out: LIB.aasm_paf_parse_device_rows(C.c_void_p(tensor.data_ptr() if n else 0), n, int(_flags) | AASM_READ_TEXT_ON_DEVICE,
                                                                          int(device), None, *out), device)

    def write_outputs(self, res, main_path, alt_path, all_path, piece_bytes=0):
        """The three output files from a batch that has no container (parse_device(container=False), from_device_text): the rows
        are formatted on the device (aasm_writer_append_device with paf = NULL).  res: a DeviceResult solved from this batch, or the
        dict of its to_torch(cuts=self).  A row that cannot be formatted raises AASM_E_PARSE / AASM_E_INVAL with
        rows_flagged_error's message and leaves no file behind."""
        _write_outputs_device(None, self, res, main_path, alt_path, all_path, piece_bytes)

    def solve(self, max_paths=10000, non_skip_linkable=False, timing=False, keep_debug=False, stream=None, **hooks):
        """hooks: _abi.HOOKS, except the two aasm_solve_device never reads (the range limit, device wrap)."""
        for name in ("test_max_contigs", "wrap_devices"):
            if name in hooks:
                raise TypeError(f"{name} has no effect on a device batch")
        res = C.c_void_p()
        opts = make_opts(max_paths, non_skip_linkable, self.device, timing, keep_debug, **hooks)
        _check(LIB.aasm_solve_device(C.byref(self.dev_view), C.byref(opts), C.c_void_p(stream or 0), C.byref(res)))
        return DeviceResult(res, self.device)

    def merge_alt(self, text: bytes, alt_baseline=0.5, _flags=0):
        """--alt on the device (aasm_paf_merge_alt_device): the second PAF joins this batch, which must be in its cs form -> a new
        DeviceBatch without a container that carries its row columns (solve, row_cols, write_outputs, to_torch(cuts=..., rows=True)).
        This batch stays valid.  A text the device declines (a zeroed group, a piece name off the fast path, a row the reader does
        not take) raises AASM_E_PARSE - with the host's message where the host finds the text bad - and leaves this batch as it
        was.  A malformed cs tag in a well-formed alt row is reported by the merged batch's solve.  _flags: AASM_READ_H_* (tests)."""
        if getattr(self, "_row_cols", None) is None and not isinstance(self._keep, Paf):
            raise AlignasmError(AASM_E_INVAL, "merge_alt: the batch has no row columns and no Paf to make them from")
        cols = self.row_cols()
        up, view, merged = C.c_void_p(), BatchIn(), RowCols()
        _check(LIB.aasm_paf_merge_alt_device(C.byref(self.dev_view), C.byref(cols), text, C.c_int64(len(text)), C.c_double(alt_baseline), int(_flags), int(self.device),
                                             C.byref(up), C.byref(view), C.byref(merged)))
        db = DeviceBatch._from_upload(up, view, self.device)
        db._row_cols = merged
        return db

    def row_cols(self) -> RowCols:
        """What an output row prints beyond the batch: resident already where the device reader left it (container=False,
        from_device_text), else uploaded once from the Paf the batch was made from (aasm_paf_upload_rows) and freed with the batch."""
        if getattr(self, "_row_cols", None) is None:
            if not isinstance(self._keep, Paf):
                raise AlignasmError(AASM_E_INVAL, "row_cols: the batch was not made from a Paf (names and row columns are the container's)")
            up, cols = C.c_void_p(), RowCols()
            _check(LIB.aasm_paf_upload_rows(self._keep._h, C.c_int64(0), C.c_int64(self.n_contigs), int(self.device), C.byref(up), C.byref(cols)))
            self._row_up, self._row_cols = up, cols
        return self._row_cols

    def close(self):
        if getattr(self, "_row_up", None):
            LIB.aasm_upload_free(self._row_up)
            self._row_up = self._row_cols = None
        if self._up:
            LIB.aasm_upload_free(self._up)
            self._up = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceResult:
    def __init__(self, handle, device=0):
        self._h = handle
        self.device = device

    def stats(self):
        st = Stats()
        _check(LIB.aasm_result_stats(self._h, C.byref(st)))
        return st.as_dict()

    def fetch(self):
        out = self.fetch_raw()
        try:
            return unpack_out(out)
        finally:
            free_out(out)

    def fetch_raw(self) -> BatchOut:
        """D2H + ragged pack into the C structure (what a C caller gets); release it with free_out()."""
        out = BatchOut()
        _check(LIB.aasm_result_fetch(self._h, C.byref(out)))
        return out

    def sizes(self):
        """aasm_result_sizes: {n_contigs, n_main, n_alt, n_all_paths, n_all_elems} (counts the .all paths on the device; one small
        read-back and a wait on the result's stream)."""
        sz = OutSizes()
        _check(LIB.aasm_result_sizes(self._h, C.byref(sz)))
        return {n: int(getattr(sz, n)) for n, _ in OutSizes._fields_}

    def export_raw(self, sizes: OutSizes, dst: DevOut, stream=0):
        """aasm_result_export as is: returns the C-ABI code (0 = enqueued on `stream`, a hipStream_t handle or 0)."""
        return int(LIB.aasm_result_export(self._h, C.byref(sizes), C.byref(dst), C.c_void_p(stream or 0)))

    def to_torch(self, stream=None, cuts=None, rows=False):
        """The result in torch tensors on its device, packed there (aasm_result_export): the keys of unpack_out() without
        `stats`; element lists are int64 [n, 5] tensors holding the 40-byte rows (column 4 is ctg_index / is_alt as two int32:
        `.view(torch.int32)`).  Asynchronous on `stream` (default: the device's current torch stream); the tensors outlive the
        next solve on the device.
        cuts: the DeviceBatch the result was solved from (one with cs tags on the device: a Paf read with device_ranges) - the
        dict then also holds `main_cut`, `alt_cut`, `all_cut`, int64 [n, 6] tensors of the elements' 48-byte cut plans
        (aasm_cut_plans_device; `cuts_to_numpy`), made on the same stream right behind the export.
        rows (with cuts): the dict also holds the three files' text, `main_text`, `alt_text`, `all_text` (uint8), and the rows'
        offsets in it, `main_row_off`, `alt_row_off`, `all_row_off` (int64, one more entry than rows), formatted on the same
        stream right behind the plans (one wait for the sizes).  A result with an element that cannot be formatted raises
        AlignasmError: AASM_E_PARSE, or AASM_E_INVAL for a record or plan fault; the message names list, element and flags."""
        import torch
        _check_one_hip_runtime()
        dev = torch.device("cuda", self.device)
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        sz = self.sizes()
        c, npth = sz["n_contigs"], sz["n_all_paths"]
        with torch.cuda.device(dev):
            i64 = lambda n: torch.empty(n, dtype=torch.int64, device=dev)   # noqa: E731
            el = lambda n: torch.empty((n, 5), dtype=torch.int64, device=dev)   # noqa: E731
            d = {"main_off": i64(c + 1), "alt_off": i64(c + 1), "all_path_off": i64(c + 1), "all_elem_off": i64(npth + 1),
                 "main": el(sz["n_main"]), "alt": el(sz["n_alt"]), "all": el(sz["n_all_elems"]),
                 "status": torch.empty(c, dtype=torch.int32, device=dev)}
        # the caching allocator hands these blocks to other work once they are freed: tie them to the export's stream
        for t in d.values():
            t.record_stream(stream)
        ptr = lambda t: t.data_ptr() if t.numel() else None   # noqa: E731
        dst = DevOut(ptr(d["main_off"]), ptr(d["alt_off"]), ptr(d["all_path_off"]), ptr(d["all_elem_off"]), ptr(d["main"]),
                     ptr(d["alt"]), ptr(d["all"]), ptr(d["status"]))
        csz = OutSizes(*(sz[n] for n, _ in OutSizes._fields_))
        _check(self.export_raw(csz, dst, stream.cuda_stream))
        if cuts is not None:
            with torch.cuda.device(dev):
                plans = {k: torch.empty((sz[n], 6), dtype=torch.int64, device=dev) for k, n in (("main_cut", "n_main"), ("alt_cut", "n_alt"), ("all_cut", "n_all_elems"))}
            for t in plans.values():
                t.record_stream(stream)
            dc = DevCuts(ptr(plans["main_cut"]), ptr(plans["alt_cut"]), ptr(plans["all_cut"]))
            _check(cut_plans_raw(cuts.dev_view, csz, dst, dc, self.device, stream.cuda_stream))
            d.update(plans)
            if rows:
                d.update(_rows_to_torch(cuts, csz, dst, dc, sz, dev, stream))
        elif rows:
            raise AlignasmError(AASM_E_INVAL, "to_torch(rows=True) needs cuts=: the DeviceBatch the result was solved from")
        d["n_contigs"] = c
        return d

    def debug(self, name, dtype):
        n = LIB.aasm_debug_fetch(self._h, name.encode(), None, C.c_int64(0))
        if n < 0:
            raise KeyError(name)
        buf = np.zeros(n // np.dtype(dtype).itemsize, dtype)
        LIB.aasm_debug_fetch(self._h, name.encode(), buf.ctypes.data_as(C.c_void_p), C.c_int64(buf.nbytes))
        return buf

    def close(self):
        if self._h:
            LIB.aasm_result_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cut_plans_raw(dev_view: BatchIn, sizes: OutSizes, dev_out: DevOut, dst: DevCuts, device=0, stream=0):
    """aasm_cut_plans_device as is: returns the C-ABI code (0 = enqueued on `stream`, a hipStream_t handle or 0)."""
    return int(LIB.aasm_cut_plans_device(C.byref(dev_view), C.byref(sizes), C.byref(dev_out), C.byref(dst), int(device), C.c_void_p(stream or 0)))


def rows_sizes_raw(dev_view: BatchIn, cols: RowCols, sizes: OutSizes, dev_out: DevOut, cuts: DevCuts, row_off: DevRows, info: RowsInfo, flags=0, device=0, stream=0):
    """aasm_rows_sizes_device as is: returns the C-ABI code; info is filled."""
    return int(LIB.aasm_rows_sizes_device(C.byref(dev_view), C.byref(cols), C.byref(sizes), C.byref(dev_out), C.byref(cuts), C.byref(row_off), int(flags), int(device),
                                          C.c_void_p(stream or 0), C.byref(info)))


def rows_format_raw(dev_view: BatchIn, cols: RowCols, sizes: OutSizes, dev_out: DevOut, cuts: DevCuts, row_off: DevRows, info: RowsInfo, lst, e0, e1, text_ptr,
                    flags=0, device=0, stream=0):
    """aasm_rows_format_device as is: returns the C-ABI code (0 = enqueued on `stream`)."""
    return int(LIB.aasm_rows_format_device(C.byref(dev_view), C.byref(cols), C.byref(sizes), C.byref(dev_out), C.byref(cuts), C.byref(row_off), C.byref(info), int(lst),
                                           C.c_int64(int(e0)), C.c_int64(int(e1)), C.c_void_p(text_ptr or 0), int(flags), int(device), C.c_void_p(stream or 0)))


ROW_LISTS = ("main", "alt", "all")


def rows_flagged_error(info: RowsInfo):
    """The AlignasmError of a result whose rows cannot all be formatted."""
    f = int(info.bad_flags)
    code = AASM_E_PARSE if f & (AASM_CUT_ERRORS & ~AASM_CUT_E_RECORD) else AASM_E_INVAL
    return AlignasmError(code, "%d output elements cannot be formatted; the first: list %s, element %d, flags 0x%x"
                         % (int(info.n_flagged), ROW_LISTS[int(info.bad_list)], int(info.bad_elem), f))


def _rows_to_torch(db, csz, dst, dc, sz, dev, stream):
    import torch
    ptr = lambda t: t.data_ptr() if t.numel() else None   # noqa: E731
    n = {"main": sz["n_main"], "alt": sz["n_alt"], "all": sz["n_all_elems"]}
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        off = {k: torch.empty(n[k] + 1, dtype=torch.int64, device=dev) for k in ROW_LISTS}
    ro = DevRows(*(ptr(off[k]) for k in ROW_LISTS))
    cols, info = db.row_cols(), RowsInfo()
    _check(rows_sizes_raw(db.dev_view, cols, csz, dst, dc, ro, info, 0, db.device, stream.cuda_stream))
    if info.n_flagged:
        raise rows_flagged_error(info)
    out = {}
    for l, k in enumerate(ROW_LISTS):
        with torch.cuda.device(dev), torch.cuda.stream(stream):
            text = torch.empty(int(info.bytes[l]), dtype=torch.uint8, device=dev)
        _check(rows_format_raw(db.dev_view, cols, csz, dst, dc, ro, info, l, 0, n[k], ptr(text), 0, db.device, stream.cuda_stream))
        out[k + "_text"], out[k + "_row_off"] = text, off[k]
    return out


def _dev_structs(d):
    """to_torch(cuts=...)'s dict as the C structures over its tensors."""
    ptr = lambda t: t.data_ptr() if t.numel() else None   # noqa: E731
    sizes = OutSizes(int(d["n_contigs"]), d["main"].shape[0], d["alt"].shape[0], d["all_elem_off"].shape[0] - 1, d["all"].shape[0])
    dst = DevOut(ptr(d["main_off"]), ptr(d["alt_off"]), ptr(d["all_path_off"]), ptr(d["all_elem_off"]), ptr(d["main"]), ptr(d["alt"]), ptr(d["all"]), ptr(d["status"]))
    dc = DevCuts(ptr(d["main_cut"]), ptr(d["alt_cut"]), ptr(d["all_cut"]))
    return sizes, dst, dc


def cuts_to_numpy(d):
    """The cut plans of DeviceResult.to_torch(cuts=...)'s dict as {"main", "alt", "all"} -> numpy CUT_DT arrays (what
    Paf.write_outputs takes).  The copies are ordered on the device's current torch stream, as torch_to_numpy's."""
    out = {}
    for k in ("main", "alt", "all"):
        t = d[k + "_cut"].contiguous().cpu().numpy()
        out[k] = np.ascontiguousarray(t).view(CUT_DT).reshape(-1) if t.size else np.zeros(0, CUT_DT)
    return out


_ONE_RUNTIME = False


def _check_one_hip_runtime():
    """Torch's tensors and streams mean something to this library only when both use the same HIP runtime (see _load)."""
    global _ONE_RUNTIME
    if _ONE_RUNTIME:
        return
    try:
        with open("/proc/self/maps") as f:
            maps = set(line.split()[-1] for line in f if "libamdhip64" in line)
    except OSError:
        return
    if len(maps) > 1:
        raise AlignasmError(AASM_E_INVAL, "this process has two HIP runtimes mapped (%s): torch's tensors and streams cannot be "
                            "handed to alignasm_amd; load the same libamdhip64 for both (INTEGRATION.md)" % ", ".join(sorted(maps)))
    _ONE_RUNTIME = True


def torch_to_numpy(d):
    """DeviceResult.to_torch()'s dict -> unpack_out()'s numpy form (without `stats`).  The copies to the host are ordered on
    the device's current torch stream: export on another stream, and that stream has to be waited for first.
    A GraphResult (what GraphBatch's methods return): every tensor as the numpy array the host entry returns."""
    if isinstance(d, GraphResult):
        return {k: t.cpu().numpy() for k, t in d.items()}
    out = {"n_contigs": int(d["n_contigs"])}
    for k in ("main_off", "alt_off", "all_path_off", "all_elem_off", "status"):
        out[k] = d[k].cpu().numpy()
    for k in ("main", "alt", "all"):
        t = d[k].contiguous().cpu().numpy()
        out[k] = np.ascontiguousarray(t).view(OUT_ELEM_DTYPE).reshape(-1) if t.size else np.zeros(0, OUT_ELEM_DTYPE)
    return out
