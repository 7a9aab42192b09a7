"""CPU tier of resident graph batches (alignasm_amd/csrc/aasm_graphs.h) in the host emulation (tests/host_emul/graphs_emul.cpp):
the *_device drivers against the host entries' drivers on the existing case sets, through both creation paths; the check kernels
against the host checks on single-defect batches and on seeded mutations; the sanitizer program on the case sets and on every hostile
batch; what the product library answers without a device; the surface.  Every comparison is exact."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import bf_cases as BC
import dag_cases as DC
import graphs_resident_cases as GR
import ksw_cases as KC
import test_dial as TD
import test_dijkstra as TJ
import test_sssp_cpu as TS


@pytest.fixture(scope="module")
def built():
    return KC.build_emul(san=True)


@pytest.fixture(scope="module")
def emr(built):
    return built[0]


@pytest.fixture(scope="module")
def host_call(emr):
    """The emulated HOST entries by name: graphs_emul.cpp's emk_*."""
    def call(name, g_voff, rowptr, col, *rest):
        b = {"g_voff": g_voff, "rowptr": rowptr, "col": col}
        if name == "dijkstra":
            rc, d, prev = TS.emul_dijkstra(emr, g_voff, rowptr, col, rest[0], rest[1])
            out = (d, prev)
        elif name == "dial":
            rc, dist, pre = TS.emul_dial(emr, g_voff, rowptr, col, rest[0], rest[1], rest[2])
            out = (dist, pre)
        elif name == "bellman_ford":
            rc, r = BC.emul_bf(emr, dict(b, w=rest[0], src=rest[1]))
            out = (r["d"], r["prev"], r["status"], r["cycles"])
        elif name == "dag":
            rc, r = DC.emul_dag(emr, dict(b, w=rest[0], src=rest[1]))
            out = (r["d"], r["prev"], r["status"], r["order"])
        else:
            rc, r = DC.emul_topo(emr, b)
            out = (r["order"], r["status"])
        assert rc == 0, (name, rc)
        return out
    return call


def _check_set(emr, host_call, b, entries):
    """The entries on a batch through both creation paths, and on every graph alone, against the host entries."""
    b = GR.typed(b) | {"w": None if b.get("w") is None else np.asarray(b["w"], np.int64).reshape(-1)}
    for sub in [b] + [GR.typed(GR.sub_batch(b, gi)) for gi in range(len(b["src"]))]:
        want = {e: GR.host_results(host_call, sub, e) for e in entries}
        for wrap in (True, False) if sub is b else (True,):
            eb = GR.EmrBatch(emr, sub, wrap)
            for e in entries:
                rc, got = eb.run(e, sub["src"])
                assert rc == 0 and GR.same(got, want[e]) == [], (e, wrap, len(sub["src"]))
            eb.close()


# ---- the resident entries against the host entries -------------------------------------------------------------------------------
def test_dag_cases(emr, host_call):
    _check_set(emr, host_call, KC.make_batch(DC.golden_graphs()), ("topology_sort", "dag"))


def test_bellman_ford_cases(emr, host_call):
    gs = BC.golden_graphs()
    assert sum(g["bf"]["status"] == 1 for g in gs) >= 5                # the negative cycles
    _check_set(emr, host_call, KC.make_batch(gs), ("bellman_ford",))


def _tuple_batch(cs, key):
    voff, rowptr, col, x, src = TS.batch(cs)
    return {"g_voff": voff, "rowptr": rowptr, "col": col, key: x, "src": src}


def test_dijkstra_cases_and_the_heap_retry(emr, host_call):
    """test_dijkstra's digraphs with tests/test_sssp_cpu.py's heap_retry_graph among them: the batch needs the 4x round (the first
    round's one-word verdict names the graph), and working memory has grown to hold it."""
    cs = TJ.cases() + [TS.heap_retry_graph()]
    b = _tuple_batch(cs, "w")
    _check_set(emr, host_call, b, ("dijkstra",))
    eb = GR.EmrBatch(emr, b, True)
    rc, _ = eb.run("dijkstra", np.asarray(b["src"]))
    E = len(b["col"])
    assert rc == 0 and emr.emr_work_bytes(eb.h) >= 4 * (E + 2 * len(cs)) * 48
    eb.close()


def test_dial_cases(emr, host_call):
    cs = TD.cases()
    for lim in sorted({c[5] for c in cs}):
        some = [c[:5] for c in cs if c[5] == lim]
        if lim != 2:
            some = some[:2]
        _check_set(emr, host_call, dict(_tuple_batch(some, "cost"), lim=lim), ("dial",))


def test_entries_a_batch_cannot_serve_and_bad_sources(emr):
    b = GR.valid_batch()
    for drop, entries in (("w", ("dijkstra", "bellman_ford", "dag")), ("cost", ("dial",))):
        eb = GR.EmrBatch(emr, dict(b, **{drop: None}), True)
        for e in entries:
            assert eb.run(e, b["src"])[0] == GR.E_INVAL and "the batch carries no" in emr.emr_last_error().decode()
        assert eb.run("topology_sort")[0] == 0
        eb.close()
    eb, pos = GR.EmrBatch(emr, b, True), GR.EmrBatch(emr, dict(b, w=np.abs(b["w"])), True)   # (dijkstra: no negative score sum)
    G = len(b["src"])
    for g, s in ((G - 1, int(np.diff(b["g_voff"])[-1])), (0, -1)):
        src = b["src"].copy(); src[g] = s
        for e in ("dijkstra", "bellman_ford", "dag", "dial"):
            rc, o = (pos if e == "dijkstra" else eb).run(e, src)
            assert rc == GR.E_INVAL and emr.emr_last_error().decode() == f"graph {g}: source outside it", e
            assert all((a == 77).all() for a in o.values())          # nothing was written
    pos.close()
    # one edge with a negative score sum: dijkstra refuses with the host entry's message, the others run
    first = int(np.flatnonzero(b["w"][0::5] + b["w"][1::5] < 0)[0])
    assert emr.emr_first_negative(eb.h) == first
    assert eb.run("dijkstra", b["src"])[0] == GR.E_OVERFLOW and emr.emr_last_error().decode().startswith(f"edge {first}: weight outside the supported range (score sum >= 0, ")
    assert eb.run("bellman_ford", b["src"])[0] == 0 and eb.run("dag", b["src"])[0] == 0
    eb.close()


# ---- the check kernels against the host checks -------------------------------------------------------------------------------------
def test_single_defects_kernels_equal_host_checks(emr):
    seen = set()
    for name, bad in GR.defects():
        host = GR.host_verdict(emr, bad)
        assert host[0] in (GR.E_INVAL, GR.E_OVERFLOW) and host[1], name
        assert GR.emr_verdict(emr, bad, True) == host, name
        assert GR.emr_verdict(emr, bad, False) == host, name
        seen.add(re.sub(r"\d+", "#", host[1]))
    assert len(seen) == 10 and "graph offsets do not end at n_vertices" in seen and "row pointers do not end at n_edges" in seen
    for ok in [GR.valid_batch()] + GR.corners():
        assert GR.host_verdict(emr, ok) == (0, "") and GR.emr_verdict(emr, ok, True) == (0, "") and GR.emr_verdict(emr, ok, False) == (0, "")


def test_single_defects_equal_the_host_entries_messages(T, emr):
    """The product library's host entries run their checks before any device is touched: their code and their message after the
    entry's name are the creation paths' (the two new clauses apart, which the host entries have no lengths for)."""
    api = T.api()
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    n = 0
    for name, bad in GR.defects():
        if name in ("voff_end_one_more", "rowptr_end_one_less"):
            continue
        G, V = len(bad["g_voff"]) - 1, bad["n_vertices"]
        d, prev, st, coff, cyc, i64 = np.zeros(5 * V, np.int64), np.zeros(V, np.int32), np.zeros(G, np.int32), np.zeros(G + 1, np.int64), np.zeros(V + G, np.int32), np.zeros(V, np.int64)
        if name.startswith(("cost", "lim")):
            rc = api.LIB.aasm_sssp_dial(C.c_int64(G), P(bad["g_voff"]), P(bad["rowptr"]), P(bad["col"]), P(bad["cost"]), P(bad["src"]), bad["lim"], P(i64), P(i64.copy()), 0)
            entry = "aasm_sssp_dial: "
        else:
            rc = api.LIB.aasm_sssp_bellman_ford(C.c_int64(G), P(bad["g_voff"]), P(bad["rowptr"]), P(bad["col"]), P(bad["w"]), P(bad["src"]), P(d), P(prev), P(st),
                                                P(coff), P(cyc), 0)
            entry = "aasm_sssp_bellman_ford: "
        msg = api.LIB.aasm_last_error().decode()
        assert msg.startswith(entry) and (rc, msg[len(entry):]) == GR.emr_verdict(emr, bad, True), name
        n += 1
    assert n > 40


def test_fuzz_single_mutations(emr):
    rng = np.random.default_rng(20263)
    b = GR.valid_batch()
    refused = 0
    for i in range(500):
        m = GR.mutate(rng, b)
        host = GR.host_verdict(emr, m)
        assert GR.emr_verdict(emr, m, True) == host, i
        refused += host[0] != 0
    assert 150 < refused < 480


# ---- the sanitizer program -----------------------------------------------------------------------------------------------------------
def _san(prog, tmp_path, b):
    GR.san_input(b, tmp_path / "in.bin")
    r = subprocess.run([prog, "resident", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.fromfile(tmp_path / "out.bin", np.int64), r.stdout


def test_sanitizer_program_on_the_case_sets(built, tmp_path):
    emr, prog = built
    sets = [GR.with_cost(KC.make_batch(DC.golden_graphs())), GR.with_cost(KC.make_batch(BC.golden_graphs()), lim=3),
            _tuple_batch(TJ.cases() + [TS.heap_retry_graph()], "w")]
    dial = TD.cases()                                               # every dial case, a batch per lim: the long fan rows among them
    lims = sorted({c[5] for c in dial})
    assert lims == [0, 1, 2, 5, 7] and max(c[0] for c in dial) == 2500
    sets += [dict(_tuple_batch([c[:5] for c in dial if c[5] == lim], "cost"), lim=lim) for lim in lims]
    for b in sets:
        b = GR.typed(b)
        out, _ = _san(prog, tmp_path, b)
        assert np.array_equal(out, GR.san_expected(emr, b))


def test_sanitizer_program_on_the_hostile_batches(built, tmp_path):
    """Exit 0 - no cell outside an array is touched before the checks refuse the batch - with the emulation's verdict."""
    emr, prog = built
    rng = np.random.default_rng(20264)
    base = GR.valid_batch()
    for name, bad in GR.defects() + [(f"mutation_{i}", GR.mutate(rng, base)) for i in range(60)]:
        out, msg = _san(prog, tmp_path, bad)
        rc, want = GR.host_verdict(emr, bad)
        assert out[0] == rc and (msg == want if rc else len(out) > 1), name


# ---- the product library without a device --------------------------------------------------------------------------------------------
def test_product_upload_answers_a_bad_batch_from_the_host_checks(T, emr):
    api = T.api()
    for name, bad in GR.defects()[::7]:
        with pytest.raises(api.AlignasmError) as ei:
            api.GraphBatch.upload(bad["g_voff"], bad["rowptr"], bad["col"], w5=bad["w"], cost=bad["cost"], lim=bad["lim"])
        rc, msg = GR.host_verdict(emr, bad)
        assert ei.value.code == rc and str(ei.value).endswith("aasm_graphs_upload: " + msg), name
    api.LIB.aasm_graphs_free(None)                                    # harmless
    assert api.LIB.aasm_graphs_view(None, None) == GR.E_INVAL


# ---- surface ---------------------------------------------------------------------------------------------------------------------------
def test_header_abi_and_api_agree(T):
    from alignasm_amd import _abi
    src = open(os.path.join(KC.ROOT, "include", "alignasm_amd.h")).read()
    assert re.search(r"#define AASM_ABI_VERSION 3\b", src)
    api = T.api()
    ctype = {"int": C.c_int, "void": None}
    for name, (restype, argtypes) in _abi.GRAPHS_SIGS.items():
        m = re.search(r"^(int|void)\s+" + name + r"\s*\(([^;]*)\);", src, re.M)
        assert m, name
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(2)).split(",")]
        assert restype is ctype[m.group(1)] and argtypes == [C.c_int if p == "int device" else C.c_void_p for p in params], name
        assert all(("*" in p) == (t is C.c_void_p) for p, t in zip(params, argtypes))
        assert name in api.EXPORTED and getattr(api.LIB, name).argtypes == argtypes and getattr(api.LIB, name).restype is restype
    fields = re.search(r"typedef struct aasm_graphs_in \{(.*?)\} aasm_graphs_in;", src, re.S).group(1)
    names = re.findall(r"\*?(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields))
    assert names == [n for n, _ in _abi.GraphsIn._fields_] and C.sizeof(_abi.GraphsIn) == 3 * 8 + 5 * 8 + 8
    sig = lambda f: list(inspect.signature(f).parameters)   # noqa: E731
    gb = api.GraphBatch
    assert sig(gb.upload) == ["g_voff", "rowptr", "col", "w5", "cost", "lim", "device"] and sig(gb.from_torch) == ["g_voff", "rowptr", "col", "w5", "cost", "lim"]
    assert inspect.signature(gb.upload).parameters["lim"].default == 2 and inspect.signature(gb.dag).parameters["order"].default is False
    assert sig(gb.dijkstra) == sig(gb.bellman_ford) == sig(gb.dial) == ["self", "src", "stream"]
    assert sig(gb.topology_sort) == ["self", "stream"] and sig(gb.dag) == ["self", "src", "order", "stream"] and sig(gb.close) == ["self"]
