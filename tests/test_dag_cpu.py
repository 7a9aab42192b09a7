"""CPU tier of aasm_topology_sort and aasm_sssp_dag: the kernel of alignasm_amd/csrc/aasm_sssp.h with its host driver (1-lane host
emulation, tests/host_emul/graphs_emul.cpp) against the real reference's runs recorded in ref_dag.npz, against the plain-Python checker
(tests/dag_checker.py) on graphs the file does not hold, and against the tree of aasm_k_shortest_walks on reversed graphs; the
argument checks, the sanitizer program, and the surface.  The emulation walks a list one edge at a time: what a chunk of 64 edges
does is proved on the card alone (tests/test_gpu_dag.py)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import dag_cases as DC
import ksw_cases as KC

N_RECORDED = 73


@pytest.fixture(scope="module")
def built():
    return KC.build_emul(san=True)


@pytest.fixture(scope="module")
def emk(built):
    return built[0]


# ---- the product (emulated) and the checker against the recorded reference ---------------------------------------------------
def test_emulation_equals_reference_fixture(emk):
    """Every recorded graph in one batch and one by one: order, d, prv, status; the sort alone gives the same order."""
    gs = DC.golden_graphs()
    assert len(gs) == N_RECORDED == len(DC.cases())
    b = KC.make_batch(gs)
    rc, got = DC.emul_dag(emk, b)
    assert rc == 0 and DC.compare_dag(b, gs, [g["want"] for g in gs], got) == []
    rc, topo = DC.emul_topo(emk, b)
    assert rc == 0 and DC.compare_dag(b, gs, [g["want"] for g in gs], topo) == []
    for g in gs:
        b = KC.make_batch([g])
        rc, got = DC.emul_dag(emk, b)
        assert rc == 0 and DC.compare_dag(b, [g], [g["want"]], got) == [], g["name"]
    byname = {g["name"]: g["want"] for g in gs}
    assert [w["status"] for w in byname.values()].count(1) == 6
    assert list(byname["diamond_push_order"]["order"][:3]) == [0, 2, 1] and byname["diamond_push_order"]["prv"][3] == 2
    assert list(byname["parallel_equal_other_split"]["d"][5:10]) == [3, 1, 0, 0, 1]          # the first of two equal offers, its own numbers
    assert list(byname["parallel_straddle_equal"]["d"][350:355]) == [4, 1, 0, 0, 2]
    assert list(byname["parallel_straddle_better"]["d"][350:355]) == [2, 2, 0, 0, 2]
    assert list(byname["unreachable_before_src"]["d"][10:15]) == [5, 0, 0, 0, 1]             # not the -50 / -60 of the vertices at max()
    assert list(byname["cycle_src_cannot_reach"]["d"][:10]) == [0, 0, 0, 0, 0, -1, -1, -1, -1, 0]


def test_checker_equals_reference_fixture():
    for g in DC.golden_graphs():
        got = DC.checker(g)
        for key in ("status", "order", "d", "prv"):
            assert np.array_equal(got[key], g["want"][key]), (g["name"], key)


def test_recorded_graphs_are_the_cases():
    for g, (name, c) in zip(DC.golden_graphs(), DC.cases()):
        assert g["name"] == name and g["src"] == c["src"] and g["n"] == c["n"] < 400
        assert np.array_equal(g["rowptr"], c["rowptr"]) and np.array_equal(g["col"], c["col"]) and np.array_equal(g["w"], c["w"])
    degs = {name: int(np.diff(c["rowptr"]).max()) for name, c in DC.cases()}
    assert [degs[f"hub_{d}"] for d in DC.HUB_DEGREES] == list(DC.HUB_DEGREES)
    hub = dict(DC.cases())["hub_200"]
    heads = hub["col"][hub["rowptr"][1]:hub["rowptr"][2]]
    assert 2 in heads[:64] and 2 not in heads[64:128] and heads[128] == 2 and 2 not in heads[129:]   # its last in-edge: the third chunk
    assert len(set(heads[:64].tolist())) < 64 and len(set(heads.tolist()) & set(range(2, 10))) == 8


# ---- the product (emulated) against independent checks ------------------------------------------------------------------------
def test_emulation_equals_checker_random(emk):
    gs = DC.random_graphs(4711, 300)
    wants = [DC.checker(g) for g in gs]
    b = KC.make_batch(gs)
    rc, got = DC.emul_dag(emk, b)
    assert rc == 0 and DC.compare_dag(b, gs, wants, got) == []
    assert not got["status"].any() and sum((w["prv"] >= 0).sum() > 10 for w in wants) > 100


def test_reversed_graph_equals_k_walks_tree(emk):
    """d5, prev and order of emk_sssp_dag on the graph reversed in ascending edge id, from the sink, against the tree stage of
    emk_k_shortest_walks (kb_ksw_tree, which keeps its own Kahn order and relaxation): d5 and best."""
    gs = KC.random_graphs(55, 300)
    b = KC.make_batch(gs)
    rc, tree = KC.emul_run(emk, b, 4, KC.AASM_KSW_TREE)
    assert rc == 0 and not tree["status"].any()
    rgs = [DC.reversed_graph(g) for g in gs]
    rb = KC.make_batch(rgs)
    rc, got = DC.emul_dag(emk, rb)
    assert rc == 0 and not got["status"].any()
    assert np.array_equal(got["d"], tree["d"]) and np.array_equal(got["prev"], tree["best"])
    assert DC.compare_dag(rb, rgs, [DC.checker(g) for g in rgs], got) == []                   # (the order: kb_ksw_tree does not return its own)


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def _one_edge(wq, wr=0):
    return KC.make_batch([KC.graph(2, [0, 1, 1], [1], [[wq, wr, 0, 0, 1]], 0, 1)])


def test_argument_checks(emk):
    ok = _one_edge(-3, 2)                                            # a negative score sum is inside the domain
    rc, got = DC.emul_dag(emk, ok)
    assert rc == 0 and list(got["d"][1]) == [-3, 2, 0, 0, 1] and list(got["order"]) == [0, 1]
    rc, got = DC.emul_dag(emk, ok, raw={"order": None})              # order = NULL is accepted
    assert rc == 0 and list(got["d"][1]) == [-3, 2, 0, 0, 1] and list(got["prev"]) == [-1, 0]
    for name in ("g_voff", "rowptr", "col", "w5", "src", "d5", "prev", "status"):
        assert DC.emul_dag(emk, ok, raw={name: None})[0] == DC.E_INVAL, name
    for name in ("g_voff", "rowptr", "col", "order", "status"):
        assert DC.emul_topo(emk, ok, raw={name: None})[0] == DC.E_INVAL, name
    assert DC.emul_topo(emk, ok)[0] == 0                             # no src: that clause is not asked of the sort
    for s in (2, -1):
        assert DC.emul_dag(emk, dict(ok, src=np.array([s], np.int32)))[0] == DC.E_INVAL
    for head in (2, -1):
        bad = dict(ok, col=np.array([head], np.int32))
        assert DC.emul_dag(emk, bad)[0] == DC.E_INVAL and DC.emul_topo(emk, bad)[0] == DC.E_INVAL
    for big in (_one_edge(1 << 39), _one_edge(-(1 << 39) - 1), _one_edge(0, 1 << 39), KC.make_batch([KC.graph(2, [0, 1, 1], [1], [[0, 0, 3, 0, 1]], 0, 1)]),
                KC.make_batch([KC.graph(2, [0, 1, 1], [1], [[0, 0, 0, 2, 1]], 0, 1)])):
        assert DC.emul_dag(emk, big)[0] == DC.E_OVERFLOW
    assert DC.emul_dag(emk, _one_edge(-(1 << 39), (1 << 39) - 1))[0] == 0                     # the domain's corner is inside
    empty = dict(ok, g_voff=np.array([0, 0], np.int64))
    assert DC.emul_dag(emk, empty)[0] == DC.E_INVAL and DC.emul_topo(emk, empty)[0] == DC.E_INVAL


def test_vertex_limit_before_any_device(emk):
    """2^20 + 1 vertices: AASM_E_OVERFLOW from aasm_sssp_dag's checks - in the product library too, which has no device here to
    touch -, while the sort alone, which sums nothing, takes the graph; 2^20 vertices are inside."""
    n = (1 << 20) + 1
    g = KC.graph(n, np.concatenate([[0], np.ones(n, np.int64)]), [n - 1], [[1, 0, 0, 0, 1]], 0, 0)
    b = KC.make_batch([g])
    assert DC.emul_dag(emk, b)[0] == DC.E_OVERFLOW
    rc, topo = DC.emul_topo(emk, b)
    assert rc == 0 and topo["status"][0] == 0 and list(topo["order"][:3]) == [0, 1, 2] and topo["order"][-1] == n - 1
    g = KC.graph(n - 1, np.concatenate([[0], np.ones(n - 1, np.int64)]), [n - 2], [[1, 0, 0, 0, 1]], 0, 0)
    rc, got = DC.emul_dag(emk, KC.make_batch([g]))
    assert rc == 0 and list(got["d"][n - 2]) == [1, 0, 0, 0, 1]


def test_product_library_checks_before_any_device(T):
    """The product's entries run the same checks before the device context is created: they answer here, without a GPU."""
    api = T.api()
    n = (1 << 20) + 1
    g = KC.graph(n, np.concatenate([[0], np.ones(n, np.int64)]), [n - 1], [[1, 0, 0, 0, 1]], 0, 0)
    b = KC.make_batch([g])
    with pytest.raises(api.AlignasmError) as ei:
        api.sssp_dag(b["g_voff"], b["rowptr"], b["col"], b["w"], b["src"])
    assert ei.value.code == DC.E_OVERFLOW and "2^20" in str(ei.value)
    ok = _one_edge(1)
    with pytest.raises(api.AlignasmError) as ei:
        api.topology_sort(ok["g_voff"], ok["rowptr"], np.array([5], np.int32))
    assert ei.value.code == DC.E_INVAL and "edge head outside the graph" in str(ei.value)
    with pytest.raises(api.AlignasmError) as ei:
        api.sssp_dag(ok["g_voff"], ok["rowptr"], ok["col"], ok["w"], np.array([7], np.int32))
    assert ei.value.code == DC.E_INVAL and "source outside it" in str(ei.value)


# ---- the sanitizer program ----------------------------------------------------------------------------------------------------------
def test_sanitizer_program_runs_clean_and_agrees(built, tmp_path):
    emk, prog = built
    gs = DC.golden_graphs()
    b = KC.make_batch(gs)
    raw = np.concatenate([np.array([len(gs), int(b["g_voff"][-1]), len(b["col"])], np.int64), b["g_voff"], b["rowptr"], b["col"].astype(np.int64),
                          b["w"].reshape(-1).astype(np.int64), b["src"].astype(np.int64)])
    raw.tofile(tmp_path / "in.bin")
    r = subprocess.run([prog, "dag", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.fromfile(tmp_path / "out.bin", np.int64)
    rc, got = DC.emul_dag(emk, b)
    assert rc == 0
    at = 0
    for gi, g in enumerate(gs):
        vb, n = int(b["g_voff"][gi]), g["n"]
        assert out[at] == got["status"][gi], gi; at += 1
        assert np.array_equal(out[at:at + 5 * n], got["d"][vb:vb + n].reshape(-1)), gi; at += 5 * n
        assert np.array_equal(out[at:at + n], got["prev"][vb:vb + n]), gi; at += n
        assert np.array_equal(out[at:at + n], got["order"][vb:vb + n]), gi; at += n
    assert at == len(out)


# ---- surface -----------------------------------------------------------------------------------------------------------------------
def test_header_and_abi_agree(T):
    from alignasm_amd import _abi
    src = open(os.path.join(KC.ROOT, "include", "alignasm_amd.h")).read()
    assert re.search(r"#define AASM_ABI_VERSION 3\b", src)
    topo = re.search(r"int\s+aasm_topology_sort\(int64_t n_graphs, const int64_t \*g_voff, const int64_t \*rowptr, const int32_t \*col,\s+"
                     r"int32_t \*order, int32_t \*status, int device\);", src)
    dag = re.search(r"int\s+aasm_sssp_dag\(int64_t n_graphs, const int64_t \*g_voff, const int64_t \*rowptr, const int32_t \*col, const int64_t \*w5,\s+"
                    r"const int32_t \*src, int64_t \*d5, int32_t \*prev, int32_t \*order /\* may be NULL \*/, int32_t \*status, int device\);", src)
    assert topo and dag
    for m, name in ((topo, "aasm_topology_sort"), (dag, "aasm_sssp_dag")):
        params = re.sub(r"/\*.*?\*/", "", m.group(0)[m.group(0).index("(") + 1:-2]).split(",")
        want = [C.c_int64 if p.strip().startswith("int64_t n_graphs") else C.c_int if p.strip() == "int device" else C.c_void_p for p in params]
        assert _abi.DAG_ARGTYPES[name] == want, name
        assert all(("*" in p) == (t is C.c_void_p) for p, t in zip(params, want))
    api = T.api()
    assert list(inspect.signature(api.topology_sort).parameters) == ["g_voff", "rowptr", "col", "device"]
    assert list(inspect.signature(api.sssp_dag).parameters) == ["g_voff", "rowptr", "col", "w5", "src", "order", "device"]
    assert inspect.signature(api.sssp_dag).parameters["order"].default is False
    for name in _abi.DAG_ARGTYPES:
        assert name in api.EXPORTED and getattr(api.LIB, name).argtypes == _abi.DAG_ARGTYPES[name]
