"""CPU tier of k shortest walks on a resident graph batch (alignasm_amd/csrc/aasm_graphs.h: graphs_ksw / graphs_ksw_export) in the host
emulation (tests/host_emul/graphs_emul.cpp): the resident driver against the emulated host driver (which existing tests pin to
the oracle and the reference's recorded runs) through both creation paths, for whole batches and for every graph alone; the heap
retry chosen on the device; sizes and host read-backs that do not depend on k or on G; every refusal with code and message; guard
words round every output; the sanitizer program; the surface.  Every comparison is exact."""
import ctypes as C
import inspect
import os
import re
import time

import numpy as np
import pytest

import bf_cases as BC
import ksw_cases as KC
import ksw_cyclic_cases as CC
import ksw_resident_cases as KR
from alignasm_amd._abi import AASM_KSW_CYCLES, AASM_KSW_HOOK_ARENA, AASM_KSW_NEGATIVE, AASM_KSW_TREE, AASM_KSW_WALKS

KS = (1, 2, 7, 100)
MAX_K = 1 << 24


@pytest.fixture(scope="module")
def built():
    return KC.build_emul(san=True)


@pytest.fixture(scope="module")
def emw(built):
    return built[0]


def _host(emw, b, k, flags):
    rc, want = KC.emul_run(emw, b, k, flags)
    assert rc == 0
    return want


def _check_set(emw, b, flags, ks=KS):
    """A batch through both creation paths, and every graph alone, against the emulated host driver; -> the host's whole-batch
    result at the last k."""
    G = len(b["src"])
    whole = None
    for k in ks:
        for sub in [b] + ([KR.sub_batch(b, gi) for gi in range(G)] if G > 1 else []):
            n = len(sub["src"])
            want = _host(emw, sub, k, flags)
            whole = want if sub is b else whole
            for wrap in (True, False) if sub is b else (True,):
                eb = KR.EmwBatch(emw, sub, wrap)
                sz, o = eb.run(k, flags)
                assert (sz.n_graphs, sz.n_vertices, sz.k, sz.flags) == (n, int(sub["g_voff"][-1]), k, flags)
                assert sz.n_walks == want["n_found"].sum() and sz.n_walk_edges == (want["walk_off"][-1] if flags & AASM_KSW_WALKS else 0)
                assert KR.differ(KR.unpack(o, n, k, flags), want) == [], (k, wrap, n)
                eb.close()
    return whole


# ---- the resident driver against the host driver ------------------------------------------------------------------------------------------
def test_dag_cases(emw):
    _check_set(emw, KC.make_batch(KC.golden_graphs() + KC.random_graphs(20271, 24)), KR.WT)


def test_dag_cases_without_walks_or_tree(emw):
    b = KC.make_batch(KC.random_graphs(20272, 12))
    for flags in (0, AASM_KSW_WALKS, AASM_KSW_TREE):
        _check_set(emw, b, flags, ks=(7,))


def test_cyclic_cases(emw):
    gs = CC.golden_graphs() + CC.random_graphs(20273, 16) + [CC.ever_improving(), CC.sink_improves()]
    want = _check_set(emw, KC.make_batch(gs), KR.WT | AASM_KSW_CYCLES)
    assert want["status"][-2] == KR.E_OVERFLOW and want["status"][-1] == KR.E_INVAL and want["n_found"][-2:].sum() == 0
    assert (want["n_found"] == 100).any()                              # a cycle between source and sink: as many walks as asked for


def test_negative_cases(emw):
    gs = BC.golden_graphs()
    want = _check_set(emw, KC.make_batch(gs), KR.WT | AASM_KSW_CYCLES | AASM_KSW_NEGATIVE)
    cyc = [i for i, g in enumerate(gs) if g["want"] is None]
    assert len(cyc) >= 3 and (want["status"][cyc] == KR.E_INVAL).all() and (want["n_found"][cyc] == 0).all()
    voff = np.concatenate([[0], np.cumsum([g["n"] for g in gs])])
    for i in cyc:                                                    # d5 / best as max / -1
        assert (want["d"][voff[i]:voff[i + 1]] == [-1, -1, -1, -1, 0]).all() and (want["best"][voff[i]:voff[i + 1]] == -1).all()


def test_negative_dags_in_dag_mode(emw):
    gs = [g for g in BC.golden_graphs() if g["want_dag"] is not None]
    assert gs
    _check_set(emw, KC.make_batch(gs), KR.WT | AASM_KSW_NEGATIVE, ks=(7,))


def test_a_cycle_between_dags_gets_no_room(emw):
    """DAG mode with KC.cycle_graph() between good graphs: its status is AASM_E_INVAL, and the scans step over a graph without arena,
    queue, results or walks."""
    gs = KC.random_graphs(20274, 5)
    gs = gs[:2] + [KC.cycle_graph()] + gs[2:4] + [KC.cycle_graph()] + gs[4:] + [KC.cycle_graph()]
    want = _check_set(emw, KC.make_batch(gs), KR.WT, ks=(2, 100))
    assert [int(s) for s in want["status"][[2, 5, 7]]] == [KR.E_INVAL] * 3 and (want["status"][[0, 1, 3, 4, 6]] == 0).all() and want["n_found"].sum() > 0


def test_heap_retry_is_chosen_on_the_device(emw):
    """One graph needs the 4x round of the tree's dijkstra, its neighbours do not: one word more is read back, the graph comes out
    as the host driver's, and the neighbours are what they are without it."""
    retry = KR.reversed_heap_retry_graph()
    near = CC.random_graphs(20275, 4)
    flags = KR.WT | AASM_KSW_CYCLES
    b = KC.make_batch(near[:2] + [retry] + near[2:])
    want = _check_set(emw, b, flags, ks=(7,))
    assert want["status"][2] == 0 and want["n_found"][2] >= 1
    reads = {}
    for name, gs in (("with", near[:2] + [retry] + near[2:]), ("without", near), ("alone", [retry])):
        eb = KR.EmwBatch(emw, KC.make_batch(gs), True)
        rc, sz = eb.solve(7, flags)
        reads[name] = emw.emw_read_bytes()
        assert rc == 0
        if name != "alone":
            reads[name + "_result"] = KR.unpack(eb.export(sz)[1], len(gs), 7, flags)
        eb.close()
    # verdict 8, one word after the first round - and after the second where there is one -, three totals, two totals
    assert reads["without"] == 8 + 8 + 24 + 16 and reads["with"] == reads["alone"] == reads["without"] + 8
    a, c = reads["with_result"], reads["without_result"]
    for i, j in ((0, 0), (1, 1), (3, 2), (4, 3)):                     # the neighbours, unchanged by the second round
        assert a["n_found"][i] == c["n_found"][j] and a["status"][i] == c["status"][j] and a["heap_nodes"][i] == c["heap_nodes"][j]
        assert np.array_equal(a["dist"][i], c["dist"][j])
        wa, wc = a["walk_off"][7 * i:7 * i + 8], c["walk_off"][7 * j:7 * j + 8]
        assert np.array_equal(np.diff(wa), np.diff(wc))


# ---- sizes and waits --------------------------------------------------------------------------------------------------------------------
def test_sizes_do_not_depend_on_k(emw):
    """300 graphs of 1 - 3 vertices at k = 2^24: nothing is sized by G * k (the host entry's dist5 alone would be 200 GB)."""
    b = KC.make_batch(KR.tiny_graphs(300, 20276, loops=False))
    want = _host(emw, b, 64, KR.WT)
    assert want["n_found"].max() < 64 and want["n_found"].sum() > 200
    eb = KR.EmwBatch(emw, b, True)
    t0 = time.perf_counter()
    sz, o = eb.run(MAX_K, KR.WT)
    assert time.perf_counter() - t0 < 1.0
    assert sz.k == MAX_K and sz.n_walks == want["n_found"].sum() and emw.emr_work_bytes(eb.h) < 1 << 20
    o2 = eb.export(sz)[1]                                             # a second export of the same solve
    assert all(np.array_equal(o[name], o2[name]) for name in o)
    assert KR.differ(KR.unpack(o, 300, 64, KR.WT), want) == []
    eb.close()


def test_read_back_does_not_grow_with_the_batch(emw):
    gs = KR.tiny_graphs(300, 20277, loops=False)
    counts = []
    for n in (1, 300):
        eb = KR.EmwBatch(emw, KC.make_batch(gs[:n]), True)
        rc, sz = eb.solve(5, KR.WT)
        counts.append(emw.emw_read_bytes())
        assert rc == 0 and eb.export(sz)[0] == 0 and emw.emw_read_bytes() == 0
        eb.close()
    assert counts == [8 + 24 + 16] * 2                               # the verdict, three totals, two totals


def test_tiny_batches_across_scan_steps(emw):
    """Many graphs with empty shares: offsets of every scan, in DAG mode and with self-loops under AASM_KSW_CYCLES."""
    for loops, flags in ((False, KR.WT), (True, KR.WT | AASM_KSW_CYCLES)):
        b = KC.make_batch(KR.tiny_graphs(300, 20278, loops))
        want = _host(emw, b, 7, flags)
        eb = KR.EmwBatch(emw, b, False)
        sz, o = eb.run(7, flags)
        assert KR.differ(KR.unpack(o, 300, 7, flags), want) == [] and (want["n_found"] == 0).any() and (want["n_found"] == 7).any() == loops
        eb.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _msg(emw):
    return emw.emr_last_error().decode()


def test_refusals_of_the_solve(emw):
    b = KC.make_batch(KC.random_graphs(20279, 6))
    G = len(b["src"])
    eb = KR.EmwBatch(emw, b, True)
    bad_ptr = "an array is NULL, not device memory of the batch's device, or misaligned"
    for raw in ({"source": None}, {"sink": None}, {"source": C.c_void_p(eb.src.ctypes.data + 2)}, {"sink": C.c_void_p(eb.sink.ctypes.data + 1)}):
        assert eb.solve(3, KR.WT, raw=raw)[0] == KR.E_INVAL and _msg(emw) == bad_ptr, raw
    assert eb.solve(3, KR.WT, raw={"sz": None})[0] == KR.E_INVAL and _msg(emw) == "empty batch or NULL pointer"
    for k in (0, -1, MAX_K + 1):
        assert eb.solve(k, KR.WT)[0] == KR.E_INVAL and _msg(emw) == "k outside 1 .. 2^24", k
    for flags in (0x10, KR.WT | 0x40, AASM_KSW_HOOK_ARENA, KR.WT | AASM_KSW_HOOK_ARENA):
        assert eb.solve(3, flags)[0] == KR.E_INVAL and _msg(emw) == "unknown flag", flags
    sizes = np.diff(b["g_voff"])
    for g, who, val in ((1, "source", -1), (4, "source", int(sizes[4])), (2, "sink", int(sizes[2])), (G - 1, "sink", -7)):
        src, sink = b["src"].copy(), b["sink"].copy()
        (src if who == "source" else sink)[g] = val
        assert eb.solve(3, KR.WT, src=src, sink=sink)[0] == KR.E_INVAL and _msg(emw) == f"graph {g}: {who} outside it"
    # the lowest graph is named, its source before its sink
    src, sink = b["src"].copy(), b["sink"].copy()
    sink[1] = src[3] = sink[3] = src[5] = -1
    assert eb.solve(3, KR.WT, src=src, sink=sink)[0] == KR.E_INVAL and _msg(emw) == "graph 1: sink outside it"
    sink[1] = 0
    assert eb.solve(3, KR.WT, src=src, sink=sink)[0] == KR.E_INVAL and _msg(emw) == "graph 3: source outside it"
    assert eb.solve(3, KR.WT)[0] == 0                                 # the handle is as good as before
    eb.close()
    # a batch without w5
    eb = KR.EmwBatch(emw, dict(b, w=None), True)
    assert eb.solve(3, KR.WT)[0] == KR.E_INVAL and _msg(emw) == "the batch carries no w5 weights"
    eb.close()
    # a negative edge: refused without AASM_KSW_NEGATIVE with the host entry's message, accepted with it
    w = np.asarray(b["w"], np.int64).copy()
    w[5] = (-3, 1, 0, 0, 0)
    for wrap in (True, False):
        eb = KR.EmwBatch(emw, dict(b, w=w), wrap)
        assert eb.solve(3, KR.WT)[0] == KR.E_OVERFLOW
        assert _msg(emw) == "edge 5: weight outside the supported range (score sum >= 0, |scores| < 2^39, anom 0..2, mapq counts 0..1)"
        assert KC.emul_run(emw, dict(b, w=w), 3, KR.WT)[0] == KR.E_OVERFLOW
        assert eb.solve(3, KR.WT | AASM_KSW_NEGATIVE)[0] == 0
        eb.close()


def test_refusals_of_the_export(emw):
    b = KC.make_batch(KC.random_graphs(20280, 6))
    eb = KR.EmwBatch(emw, b, True)
    rc, sz = eb.solve(5, KR.WT)
    assert rc == 0 and sz.n_walks > 0 and sz.n_walk_edges > 0 and sz.serial == 1
    bad_ptr = "an array is NULL, not device memory of the batch's device, or misaligned"
    for name in KR.OUT_TYPES:
        for kw in ({"null": (name,)}, {"odd": (name,)}):
            assert eb.export(sz, **kw)[0] == KR.E_INVAL and _msg(emw) == bad_ptr, (name, kw)
    assert emw.emw_export(eb.h, None, None) == KR.E_INVAL
    rc, first = eb.export(sz)
    assert rc == 0
    stale = "the sizes are not those of the handle's latest k-walk solve, or a later call has reused its working memory"
    for field, value in (("serial", 2), ("serial", 0), ("n_walks", sz.n_walks + 1), ("flags", sz.flags & ~AASM_KSW_WALKS), ("k", 6)):
        other = type(sz).from_buffer_copy(sz)
        setattr(other, field, value)
        assert eb.export(other)[0] == KR.E_INVAL and _msg(emw) == stale, field
    # walk arrays are not asked for without AASM_KSW_WALKS, tree arrays not without AASM_KSW_TREE
    rc, sz2 = eb.solve(5, 0)
    assert rc == 0 and sz2.serial == 2 and sz2.n_walk_edges == 0
    assert eb.export(sz2, null=("walk_off", "walk_edges", "d5", "best"))[0] == 0
    assert eb.export(sz)[0] == KR.E_INVAL and _msg(emw) == stale      # the first solve's sizes, after the second solve
    # another entry on the handle takes the working memory
    rc, sz3 = eb.solve(5, KR.WT)
    order, status = np.zeros(eb.V, np.int32), np.zeros(eb.G, np.int32)
    assert rc == 0 and emw.emr_topology_sort(eb.h, order.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.c_void_p)) == 0
    assert eb.export(sz3)[0] == KR.E_INVAL and _msg(emw) == stale
    rc, sz4 = eb.solve(5, KR.WT)                                      # ... and a new solve is as the first
    rc2, again = eb.export(sz4)
    assert rc == 0 and rc2 == 0 and all(np.array_equal(first[n], again[n]) for n in first)
    eb.close()


def test_refused_allocation_leaves_the_handle_usable(emw):
    gs = KC.random_graphs(20281, 12)
    b, small = KC.make_batch(gs), KC.make_batch(gs)
    eb = KR.EmwBatch(emw, b, True)
    rc, sz = eb.solve(2, 0)
    need_small = emw.emr_work_bytes(eb.h)
    assert rc == 0
    try:
        emw.emw_alloc_limit(need_small)                              # what k = 2 took is the most the "device" gives
        rc, _ = eb.solve(100, KR.WT)
        assert rc == KR.E_NOMEM and emw.emr_work_bytes(eb.h) <= need_small
        rc, sz = eb.solve(2, KR.WT)                                  # the smaller solve on the same handle
        assert rc == 0
        got = KR.unpack(eb.export(sz)[1], len(gs), 2, KR.WT)
    finally:
        emw.emw_alloc_limit(0)
    assert KR.differ(got, _host(emw, small, 2, KR.WT)) == []
    rc, sz = eb.solve(100, KR.WT)
    assert rc == 0 and emw.emr_work_bytes(eb.h) > need_small
    eb.close()


def test_guard_words_round_every_output(emw):
    """EmwBatch.export puts every array between sentinel words and checks them; here on results with empty arrays too."""
    for gs, flags in ((KC.random_graphs(20282, 5), KR.WT), ([KC.cycle_graph()], KR.WT), (KR.tiny_graphs(70, 20283, True), KR.WT | AASM_KSW_CYCLES)):
        eb = KR.EmwBatch(emw, KC.make_batch(gs), True)
        sz, o = eb.run(9, flags)
        assert len(o["dist5"]) == 5 * sz.n_walks and len(o["walk_off"]) == sz.n_walks + 1 and len(o["walk_edges"]) == sz.n_walk_edges
        eb.close()


# ---- the sanitizer program ------------------------------------------------------------------------------------------------------------------
def test_sanitizer_program_on_the_golden_sets(built, tmp_path):
    emw, prog = built
    sets = ((KC.golden_graphs(), KR.WT), (CC.golden_graphs() + [CC.ever_improving(), CC.sink_improves()], KR.WT | AASM_KSW_CYCLES),
            (BC.golden_graphs(), KR.WT | AASM_KSW_CYCLES | AASM_KSW_NEGATIVE), ([KR.reversed_heap_retry_graph()] + KR.tiny_graphs(70, 20284, True), AASM_KSW_WALKS | AASM_KSW_CYCLES))
    for gs, flags in sets:
        b = KC.make_batch(gs)
        for k in (1, 7, 100):
            out, _ = KR.san_run(prog, tmp_path, b, k, flags)
            eb = KR.EmwBatch(emw, b, True)
            sz, o = eb.run(k, flags)
            eb.close()
            assert np.array_equal(out, KR.san_expected(sz, o, flags)), (k, flags)


def test_sanitizer_program_on_the_refusals(built, tmp_path):
    _, prog = built
    b = KC.make_batch(KC.random_graphs(20285, 6))
    neg = np.asarray(b["w"], np.int64).copy()
    neg[0] = (-3, 1, 0, 0, 0)
    stale = "the sizes are not those of the handle's latest k-walk solve, or a later call has reused its working memory"
    cases = [(b, 0, KR.WT, 0, KR.E_INVAL, "k outside 1 .. 2^24"), (b, MAX_K + 1, KR.WT, 0, KR.E_INVAL, "k outside 1 .. 2^24"),
             (b, 3, 0x20, 0, KR.E_INVAL, "unknown flag"), (b, 3, AASM_KSW_HOOK_ARENA, 0, KR.E_INVAL, "unknown flag"),
             (dict(b, w=None), 3, KR.WT, 0, KR.E_INVAL, "the batch carries no w5 weights"),
             (dict(b, src=np.array([0, 0, 99, 0, 0, 0])), 3, KR.WT, 0, KR.E_INVAL, "graph 2: source outside it"),
             (dict(b, sink=np.array([0, -1, 99, 0, 0, 0])), 3, KR.WT, 0, KR.E_INVAL, "graph 1: sink outside it"),
             (dict(b, w=neg), 3, KR.WT, 0, KR.E_OVERFLOW, "edge 0: weight outside the supported range (score sum >= 0, |scores| < 2^39, anom 0..2, mapq counts 0..1)"),
             (b, 3, KR.WT, 1, KR.E_INVAL, stale), (b, 3, KR.WT, 2, KR.E_INVAL, stale),
             (b, 3, KR.WT, 4, KR.E_INVAL, "an array is NULL, not device memory of the batch's device, or misaligned")]
    for bb, k, flags, mode, rc, msg in cases:
        out, said = KR.san_run(prog, tmp_path, bb, k, flags, mode)
        assert list(out) == [rc] and said == msg, (k, flags, mode)


# ---- surface ----------------------------------------------------------------------------------------------------------------------------------
def test_header_abi_and_api_agree(T):
    from alignasm_amd import _abi
    src = open(os.path.join(KC.ROOT, "include", "alignasm_amd.h")).read()
    assert re.search(r"#define AASM_ABI_VERSION 3\b", src)
    api = T.api()
    assert api.LIB.aasm_abi_version() == 3
    ctype = {"int": C.c_int, "int64_t": C.c_int64}
    assert set(_abi.KSW_DEVICE_SIGS) == {"aasm_k_shortest_walks_device", "aasm_ksw_export_device"} and not set(_abi.KSW_DEVICE_SIGS) & set(_abi.GRAPHS_SIGS)
    for name, (restype, argtypes) in _abi.KSW_DEVICE_SIGS.items():
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", src, re.M)
        assert m, name
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
        assert restype is C.c_int and argtypes == [C.c_void_p if "*" in p else ctype[p.split()[0]] for p in params], name
        assert name in api.EXPORTED and getattr(api.LIB, name).argtypes == argtypes and getattr(api.LIB, name).restype is restype
    for struct, mirror, size in (("aasm_ksw_sizes", _abi.KswSizes, 56), ("aasm_ksw_dev_out", _abi.KswDevOut, 72)):
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, re.S).group(1)
        names = re.findall(r"\*?(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
        assert names == [n for n, _ in mirror._fields_] and C.sizeof(mirror) == size, struct
    sig = inspect.signature(api.GraphBatch.k_shortest_walks)
    assert list(sig.parameters) == ["self", "source", "sink", "k", "walks", "tree", "cycles", "negative", "stream"]
    assert [sig.parameters[n].default for n in ("walks", "tree", "cycles", "negative", "stream")] == [True, False, False, False, None]
    null = C.c_void_p()
    assert api.LIB.aasm_k_shortest_walks_device(null, null, null, 1, 0, null, null) == KR.E_INVAL      # a NULL handle, before any device
    assert api.LIB.aasm_ksw_export_device(null, null, null, null) == KR.E_INVAL
