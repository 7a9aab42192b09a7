"""GPU tier of resident graph batches (api.GraphBatch over aasm_graphs_upload / aasm_graphs_wrap_device and the five *_device entries),
under poisoned working memory as tests/test_gpu_dag.py: every result, fetched with torch_to_numpy, is word for word the host entry's
of the same name for the same graphs and sources (dial's status is 0, bellman_ford's cycles are compared packed).  The 64-lane forms
of the solve kernels, the check kernels' ballots and atomics and the stream ordering exist only on the card."""
import ctypes as C

import numpy as np
import pytest

import bf_cases as BC
import dag_cases as DC
import graphs_resident_cases as GR
import ksw_cases as KC
import test_dial as TD
import test_dijkstra as TJ
import test_sssp_cpu as TS
from poison_testlib import BYTE_IDS, BYTES, cached, guarded, poisoned

pytestmark = pytest.mark.gpu

both_bytes = pytest.mark.parametrize("byte", BYTES, ids=BYTE_IDS)
ALL = ("dijkstra", "bellman_ford", "topology_sort", "dag", "dial")
NO_DJ = ALL[1:]


def _tuple_batch(cs, key):
    voff, rowptr, col, x, src = TS.batch(cs)
    return {"g_voff": voff, "rowptr": rowptr, "col": col, key: x, "src": src}


def _tiny(count=300):
    """`count` graphs of 1-3 vertices, self-loops and two-cycles among them, every score sum positive: all five entries take them,
    and no cycle improves a distance (round a cycle whose sum is 0 the mapq ratio alone can improve for ever, and dijkstra - the
    reference's and the kernel's - does not return before the counters wrap)."""
    rng = np.random.default_rng(77)
    gs = []
    for _ in range(count):
        n = int(rng.integers(1, 4))
        rows = [[int(x) for x in rng.integers(0, n, int(rng.integers(0, 3)))] for _ in range(n)]
        rp = np.zeros(n + 1, np.int64)
        rp[1:] = np.cumsum([len(r) for r in rows])
        E = int(rp[-1])
        w = np.stack([rng.integers(1, 5, E), rng.integers(0, 5, E), rng.integers(0, 3, E), rng.integers(0, 2, E), rng.integers(0, 2, E)], 1)
        gs.append(KC.graph(n, rp, [v for r in rows for v in r], w.reshape(-1, 5) if E else np.zeros((0, 5), np.int64), int(rng.integers(0, n)), 0))
    return gs


def _sets():
    """name -> (batch, the entries it can serve); graphs under 400 vertices."""
    def make():
        dial = [c for c in TD.cases() if c[0] < 400]
        dj = _tuple_batch(TJ.cases() + [TS.heap_retry_graph()], "w")
        out = {
            "dag": (GR.with_cost(KC.make_batch(DC.golden_graphs() + DC.random_graphs(4713, 60))), NO_DJ),
            "bellman_ford": (GR.with_cost(KC.make_batch(BC.golden_graphs()), lim=3), NO_DJ),
            "dijkstra": (GR.with_cost(dict(dj, w=dj["w"].reshape(-1, 5)), lim=1), ALL),
            **{f"dial_{lim}": (dict(_tuple_batch([c[:5] for c in dial if c[5] == lim], "cost"), lim=lim), ("topology_sort", "dial"))
               for lim in (0, 1, 2, 5, 7)},                          # every dial case under 400 vertices, a batch per lim
            "tiny_300": (GR.with_cost(KC.make_batch(_tiny())), ALL),
            "one_vertex": (GR.with_cost(KC.make_batch([KC.graph(1, [0, 0], [], np.zeros((0, 5), np.int64), 0, 0)])), ALL),
        }
        return {k: (GR.typed(b) | {"w": None if b.get("w") is None else np.asarray(b["w"], np.int64).reshape(-1, 5)}, e) for k, (b, e) in out.items()}
    return cached("graphs resident sets", make)


def _want(api, name, b, entry, src=None):
    """The host entry's answer, computed once per (set, entry, sources)."""
    key = ("graphs resident want", name, entry, None if src is None else bytes(np.asarray(src, np.int32)))
    return cached(key, lambda: GR.host_results(GR.api_call(api), b if src is None else dict(b, src=np.asarray(src, np.int32)), entry))


def _tensors(b):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    return {k: t(b[k] if k != "w" or b[k] is None else b[k].reshape(-1)) for k in ("g_voff", "rowptr", "col", "w", "cost")}


def _make(api, b, how):
    if how == "upload":
        return api.GraphBatch.upload(b["g_voff"], b["rowptr"], b["col"], w5=b["w"], cost=b["cost"], lim=b["lim"])
    t = _tensors(b)
    return api.GraphBatch.from_torch(t["g_voff"], t["rowptr"], t["col"], w5=t["w"], cost=t["cost"], lim=b["lim"])


def _run(api, gb, entry, src, **kw):
    d = guarded(api, getattr(gb, entry), **kw) if entry == "topology_sort" else guarded(api, getattr(gb, entry), src, **({"order": True} if entry == "dag" else {}), **kw)
    return d


@both_bytes
@pytest.mark.parametrize("how", ("upload", "from_torch"))
def test_resident_entries_equal_the_host_entries(T, byte, how):
    """Every set through one constructor, all the entries it can serve; the dijkstra set holds tests/test_sssp_cpu.py's
    heap_retry_graph, which needs the 4x round."""
    api = T.api()
    for name, (b, entries) in _sets().items():
        want = {e: _want(api, name, b, e) for e in entries}
        with poisoned(api, byte):
            gb = guarded(api, _make, api, b, how)
            try:
                for e in entries:
                    got = api.torch_to_numpy(_run(api, gb, e, b["src"]))
                    assert GR.same(got, want[e]) == [], (name, e)
            finally:
                gb.close()
    assert any("hub_" in g["name"] or "fan_in_" in g["name"] for g in DC.golden_graphs())


@both_bytes
def test_one_handle_six_source_vectors(T, byte):
    """Working memory is the handle's and is poisoned again before every call: a cell the previous query left cannot help."""
    api = T.api()
    rng = np.random.default_rng(5)
    for name in ("dag", "dijkstra"):
        b, entries = _sets()[name]
        sizes = np.diff(b["g_voff"])
        srcs = [(rng.integers(0, 1 << 30, len(sizes)) % sizes).astype(np.int32) for _ in range(6)]
        with poisoned(api, byte):
            gb = guarded(api, _make, api, b, "upload")
            try:
                for i, src in enumerate(srcs):
                    for e in entries:                                # (topology_sort takes no sources: the same answer from memory poisoned again)
                        want = _want(api, name, b, e, src)
                        assert GR.same(api.torch_to_numpy(_run(api, gb, e, src)), want) == [], (name, e, i)
            finally:
                gb.close()


def test_borrowed_arrays_stay_and_outputs_stay_inside(T):
    """from_torch's tensors are byte-identical after all five entries; outputs placed inside larger tensors leave the sentinel words on
    both sides alone (the raw entries, with pointers 16 bytes into each tensor)."""
    import torch
    api = T.api()
    b, _ = _sets()["dijkstra"]
    t = _tensors(b)
    before = {k: v.clone() for k, v in t.items()}
    G, V = len(b["src"]), b["n_vertices"]
    pad = {torch.int64: 2, torch.int32: 4}
    dev = t["col"].device

    def framed(n, dtype):
        big = torch.full((n + 2 * pad[dtype],), -7777, dtype=dtype, device=dev)
        return big, big[pad[dtype]:pad[dtype] + n]
    with poisoned(api, BYTES[0]):
        gb = api.GraphBatch.from_torch(t["g_voff"], t["rowptr"], t["col"], w5=t["w"], cost=t["cost"], lim=b["lim"])
        src = torch.from_numpy(b["src"]).to(dev)
        torch.cuda.synchronize()
        P = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
        shapes = {"d": (5 * V, torch.int64), "prev": (V, torch.int32), "status": (G, torch.int32), "cycle_off": (G + 1, torch.int64), "cycle": (V + G, torch.int32),
                  "order": (V, torch.int32), "dist": (V, torch.int64), "pre": (V, torch.int64)}
        calls = {"dijkstra": ("d", "prev"), "bellman_ford": ("d", "prev", "status", "cycle_off", "cycle"), "topology_sort": ("order", "status"),
                 "dag": ("d", "prev", "order", "status"), "dial": ("dist", "pre", "status")}
        for e, keys in calls.items():
            fr = {k: framed(*shapes[k]) for k in keys}
            args = [gb._h] + ([] if e == "topology_sort" else [P(src)]) + [P(fr[k][1]) for k in keys] + [None]
            rc = guarded(api, getattr(api.LIB, {"topology_sort": "aasm_topology_sort_device"}.get(e, f"aasm_sssp_{e}_device")), *args)
            assert rc == 0, (e, api.LIB.aasm_last_error())
            torch.cuda.synchronize()
            want = _want(api, "dijkstra", b, e)
            for k in keys:
                big, inner = fr[k]
                p = pad[big.dtype]
                assert (big[:p] == -7777).all() and (big[-p:] == -7777).all(), (e, k)
                got = inner.cpu().numpy()
                if k == "cycle":
                    n = int(want["cycle_off"][-1])
                    assert np.array_equal(got[:n], want["cycle"][:n]) and (got[n:] == -7777).all()
                else:
                    assert np.array_equal(got, want[k].reshape(-1)), (e, k)
        gb.close()
    for k, v in t.items():
        assert v is None or torch.equal(v, before[k]), k


def test_single_defects_through_from_torch(T):
    """The check kernels on the card against the host checks (aasm_graphs_upload answers from them before it touches a device): code
    and message text.  The same inputs run clean through the sanitizer program in tests/test_graphs_resident_cpu.py."""
    api = T.api()
    seen = 0
    for name, bad in GR.defects():
        gi, keep = GR.graphs_in(bad)                                 # (the C entry itself: GraphBatch.upload has length checks of its own)
        h = C.c_void_p()
        rc = api.LIB.aasm_graphs_upload(C.byref(gi), 0, C.byref(h))
        text = api.LIB.aasm_last_error().decode().split("aasm_graphs_upload: ")[1]
        assert rc in (GR.E_INVAL, GR.E_OVERFLOW), name
        with pytest.raises(api.AlignasmError) as dev:
            guarded(api, _make, api, dict(bad, w=bad["w"].reshape(-1, 5)), "from_torch")
        assert dev.value.code == rc and str(dev.value).split("aasm_graphs_wrap_device: ")[1] == text, name
        seen += 1
    assert seen == len(GR.defects()) >= 45
    for ok in GR.corners():
        _make(api, dict(ok, w=ok["w"].reshape(-1, 5)), "from_torch").close()


def test_other_refusals(T):
    import torch
    api = T.api()
    b = GR.valid_batch()
    b["w"] = b["w"].reshape(-1, 5)
    gb = _make(api, b, "from_torch")
    G, V = len(b["src"]), b["n_vertices"]
    src = b["src"].copy()
    src[G - 1] = int(np.diff(b["g_voff"])[-1])                      # outside the LAST graph
    for e in ("bellman_ford", "dag", "dial"):
        with pytest.raises(api.AlignasmError) as ei:
            _run(api, gb, e, src)
        assert ei.value.code == GR.E_INVAL and str(ei.value).endswith(f"graph {G - 1}: source outside it"), e
    first = int(np.flatnonzero(b["w"][:, 0] + b["w"][:, 1] < 0)[0])
    with pytest.raises(api.AlignasmError) as ei:
        gb.dijkstra(b["src"])
    assert ei.value.code == GR.E_OVERFLOW and f"edge {first}: weight outside the supported range (score sum >= 0, " in str(ei.value)
    no_w = _make(api, dict(b, w=None), "upload")
    with pytest.raises(api.AlignasmError) as ei:
        no_w.dag(b["src"])
    assert ei.value.code == GR.E_INVAL and "no w5" in str(ei.value)
    no_w.close()
    # output pointers: host memory, NULL, misaligned - AASM_E_INVAL, and the good arrays of the same call are not written
    dev = torch.device("cuda", 0)
    s = torch.from_numpy(b["src"]).to(dev)
    d = torch.full((5 * V + 2,), -7777, dtype=torch.int64, device=dev)
    prev = torch.full((V,), -7777, dtype=torch.int32, device=dev)
    status = torch.full((G,), -7777, dtype=torch.int32, device=dev)
    host = np.zeros(5 * V, np.int64)
    for bad_d in (C.c_void_p(host.ctypes.data), None, C.c_void_p(d.data_ptr() + 4)):
        rc = api.LIB.aasm_sssp_dag_device(gb._h, C.c_void_p(s.data_ptr()), bad_d, C.c_void_p(prev.data_ptr()), None, C.c_void_p(status.data_ptr()), None)
        assert rc == GR.E_INVAL and b"misaligned" in api.LIB.aasm_last_error()
    assert api.LIB.aasm_sssp_dag_device(gb._h, C.c_void_p(b["src"].ctypes.data), C.c_void_p(d.data_ptr()), C.c_void_p(prev.data_ptr()), None, C.c_void_p(status.data_ptr()), None) == GR.E_INVAL
    torch.cuda.synchronize()
    assert (d == -7777).all() and (prev == -7777).all() and (status == -7777).all() and not host.any()
    gb.close()


def test_first_negative_edge_beyond_the_first_wave_and_the_first_pass(T):
    """The check kernel reports the first edge with a negative score sum with one atomic per wave - the lowest lane of a ballot - and
    takes edges beyond GR_MAX_BLOCKS (4096) blocks of 256 in further grid-stride passes.  One graph of 2 vertices and 4096 * 256 + 1000
    edges, its first negative edge in the sixth wave of the first block, or in the second pass at a lane that is not a wave's first,
    with later negative edges in the same wave, in other waves and in other blocks: dijkstra names that edge, as after an upload,
    whose host loop found it."""
    api = T.api()
    E = 4096 * 256 + 1000
    for first in (64 * 5 + 17, 4096 * 256 + 300):
        w = np.zeros((E, 5), np.int64)
        w[:, 0] = 1; w[:, 4] = 1
        w[first::97, 0] = -3
        w[first + 1:first + 4, 0] = -2
        b = {"g_voff": np.array([0, 2], np.int64), "rowptr": np.array([0, E, E], np.int64), "col": np.ones(E, np.int32), "w": w, "cost": None, "lim": 2}
        src = np.zeros(1, np.int32)
        texts = []
        for how in ("from_torch", "upload"):
            gb = _make(api, b, how)
            with pytest.raises(api.AlignasmError) as ei:
                gb.dijkstra(src)
            assert ei.value.code == GR.E_OVERFLOW and f": edge {first}: weight outside the supported range (score sum >= 0, " in str(ei.value), (first, how)
            texts.append(str(ei.value))
            got = api.torch_to_numpy(gb.bellman_ford(src))           # accepted there: vertex 1 by the first best edge
            assert list(got["d"][1]) == [-3, 0, 0, 0, 1] and list(got["prev"]) == [-1, 0] and not got["status"].any()
            gb.close()
        assert texts[0] == texts[1]


@both_bytes
def test_two_streams_share_one_handle(T, byte):
    import torch
    api = T.api()
    b, _ = _sets()["dag"]
    sizes = np.diff(b["g_voff"])
    rng = np.random.default_rng(9)
    srcs = [(rng.integers(0, 1 << 30, len(sizes)) % sizes).astype(np.int32) for _ in range(2)]
    streams = [torch.cuda.Stream(device=0) for _ in range(2)]
    with poisoned(api, byte):
        gb = guarded(api, _make, api, b, "upload")
        try:
            got = [_run(api, gb, e, src, stream=st) for e in ("dag", "dial") for src, st in zip(srcs, streams)]
            for st in streams:
                st.synchronize()
            for i, (e, src) in enumerate((e, src) for e in ("dag", "dial") for src in srcs):
                assert GR.same(api.torch_to_numpy(got[i]), _want(api, "dag", b, e, src)) == [], (e, i)
        finally:
            gb.close()
