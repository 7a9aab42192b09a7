"""GPU tier of k shortest walks on a resident graph batch (api.GraphBatch.k_shortest_walks over aasm_k_shortest_walks_device /
aasm_ksw_export_device), under poisoned working memory as tests/test_gpu_graphs_resident.py: every result, fetched with
torch_to_numpy and unpacked into the host layout (ksw_resident_cases.unpack), is word for word api.k_shortest_walks' for the same
graphs, sources, sinks, k and flags.  The one-wave scans over the graphs, the 64-lane tree kernels behind device-made offsets, the
pack kernels' bisections and the stream ordering exist only on the card.  Graphs stay under 400 vertices."""
import numpy as np
import pytest

import bf_cases as BC
import ksw_cases as KC
import ksw_cyclic_cases as CC
import ksw_resident_cases as KR
from alignasm_amd._abi import AASM_KSW_CYCLES, AASM_KSW_NEGATIVE, AASM_KSW_TREE, AASM_KSW_WALKS
from poison_testlib import BYTE_IDS, BYTES, cached, guarded, poisoned

pytestmark = pytest.mark.gpu

both_bytes = pytest.mark.parametrize("byte", BYTES, ids=BYTE_IDS)
MAX_K = 1 << 24
SCAN_TILE = 64                                                       # gr_wave_scans: graphs per step


def _kw(flags):
    return {"walks": bool(flags & AASM_KSW_WALKS), "tree": bool(flags & AASM_KSW_TREE), "cycles": bool(flags & AASM_KSW_CYCLES),
            "negative": bool(flags & AASM_KSW_NEGATIVE)}


def _sets():
    """mode -> batch: the CPU tier's case sets"""
    def make():
        small = lambda gs: [g for g in gs if g["n"] < 400]   # noqa: E731
        return {"dag": KC.make_batch(small(KC.golden_graphs()) + KC.random_graphs(20271, 24)),
                "cycles": KC.make_batch(small(CC.golden_graphs()) + CC.random_graphs(20273, 16) + [CC.ever_improving(), CC.sink_improves()]),
                "negative": KC.make_batch(small(BC.golden_graphs()))}
    return cached("ksw resident sets", make)


def _want(api, name, b, k, flags):
    """The host entry's answer, computed once per (batch, k, flags)."""
    return cached(("ksw resident want", name, k, flags),
                  lambda: api.k_shortest_walks(b["g_voff"], b["rowptr"], b["col"], b["w"], b["src"], b["sink"], k, **_kw(flags)))


def _make(api, b, how):
    w = np.asarray(b["w"], np.int64).reshape(-1, 5)
    if how == "upload":
        return api.GraphBatch.upload(b["g_voff"], b["rowptr"], b["col"], w5=w)
    import torch
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt).reshape(-1)).to(torch.device("cuda", 0))   # noqa: E731
    return api.GraphBatch.from_torch(t(b["g_voff"], np.int64), t(b["rowptr"], np.int64), t(b["col"], np.int32), w5=t(w, np.int64))


def _flat(o):
    """torch_to_numpy's dict with the [n, 5] arrays flat, as aasm_ksw_dev_out has them"""
    return {name: (a.reshape(-1) if name in ("dist5", "d5") else a) for name, a in o.items()}


def _got(api, gb, b, k, flags, **kw):
    o = api.torch_to_numpy(guarded(api, gb.k_shortest_walks, b["src"], b["sink"], k, **_kw(flags), **kw))
    return KR.unpack(_flat(o), len(b["src"]), k, flags)


@both_bytes
@pytest.mark.parametrize("how", ("upload", "from_torch"))
@pytest.mark.parametrize("mode", ("dag", "cycles", "negative"))
def test_resident_equals_the_host_entry(T, byte, how, mode):
    api = T.api()
    b, flags = _sets()[mode], KR.WT | KR.MODES[mode]
    want = {k: _want(api, mode, b, k, flags) for k in (1, 7, 100)}
    if mode == "cycles":
        assert want[100]["status"][-2] == KR.E_OVERFLOW and want[100]["status"][-1] == KR.E_INVAL and (want[100]["n_found"] == 100).any()
    if mode == "negative":
        assert (want[7]["status"] == KR.E_INVAL).sum() >= 3
    with poisoned(api, byte):
        gb = guarded(api, _make, api, b, how)
        try:
            for k in (100, 1, 7):
                assert KR.differ(_got(api, gb, b, k, flags), want[k]) == [], k
        finally:
            gb.close()


@both_bytes
@pytest.mark.parametrize("count", (300, 5000))
def test_tiny_batches(T, byte, count):
    """Graphs of 1 - 3 vertices, many with an empty share of every arena - unreachable sinks, source == sink, single vertices, and
    with cycles=True self-loops and two-cycles: 300, and 5000 = 78 steps of the one-wave scans' 64 graphs and a remainder of 8."""
    api = T.api()
    assert count % SCAN_TILE and count > 2 * SCAN_TILE
    for loops, flags in ((False, KR.WT), (True, KR.WT | AASM_KSW_CYCLES)):
        name = ("tiny", count, loops)
        b = cached(("ksw resident batch",) + name, lambda: KC.make_batch(KR.tiny_graphs(count, 20278, loops)))
        want = _want(api, name, b, 7, flags)
        assert (want["n_found"] == 0).any() and (want["n_found"] == 7).any() == loops
        with poisoned(api, byte):
            gb = guarded(api, _make, api, b, "from_torch" if loops else "upload")
            try:
                assert KR.differ(_got(api, gb, b, 7, flags), want) == []
            finally:
                gb.close()


@both_bytes
def test_k_at_its_maximum(T, byte):
    """The 300 tiny DAGs at k = 2^24: the result is as small as the walks found (the host entry cannot be asked: its dist5 alone
    would be 670 MB per graph), and equal to the host entry's at k = 64, which finds them all."""
    api = T.api()
    b = cached(("ksw resident batch", "tiny", 300, False), lambda: KC.make_batch(KR.tiny_graphs(300, 20278, False)))
    want = _want(api, ("tiny", 300, False), b, 64, KR.WT)
    assert want["n_found"].max() < 64
    with poisoned(api, byte):
        gb = guarded(api, _make, api, b, "upload")
        try:
            o = api.torch_to_numpy(guarded(api, gb.k_shortest_walks, b["src"], b["sink"], MAX_K, tree=True))
        finally:
            gb.close()
    assert o["dist5"].shape == (int(want["n_found"].sum()), 5) and len(o["walk_off"]) == want["n_found"].sum() + 1
    assert KR.differ(KR.unpack(_flat(o), 300, 64, KR.WT), want) == []


@both_bytes
def test_two_solves_on_one_handle(T, byte):
    """Different k and flags back to back: the second is right under poison - nothing is inherited -, and the first solve's sizes
    are refused afterwards."""
    api = T.api()
    b = _sets()["cycles"]
    f1, f2 = KR.WT | AASM_KSW_CYCLES, AASM_KSW_WALKS | AASM_KSW_CYCLES
    want1, want2 = _want(api, "cycles", b, 100, f1), _want(api, "cycles", b, 7, f2)
    with poisoned(api, byte):
        gb = guarded(api, _make, api, b, "upload")
        try:
            sz1 = guarded(api, gb.ksw_solve, b["src"], b["sink"], 100, **_kw(f1))
            assert KR.differ(_got(api, gb, b, 7, f2), want2) == []
            with pytest.raises(api.AlignasmError) as ei:
                gb.ksw_export(sz1)
            assert ei.value.code == KR.E_INVAL and "not those of the handle's latest k-walk solve" in str(ei.value)
            assert KR.differ(_got(api, gb, b, 100, f1), want1) == []
        finally:
            gb.close()


@both_bytes
def test_one_solve_exported_twice_on_two_streams(T, byte):
    import torch
    api = T.api()
    b, flags = _sets()["dag"], KR.WT
    want = _want(api, "dag", b, 7, flags)
    with poisoned(api, byte):
        gb = guarded(api, _make, api, b, "from_torch")
        try:
            s1, s2 = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
            sz = guarded(api, gb.ksw_solve, b["src"], b["sink"], 7, **_kw(flags), stream=s1)
            a, c = guarded(api, gb.ksw_export, sz, stream=s1), guarded(api, gb.ksw_export, sz, stream=s2)
            s1.synchronize(); s2.synchronize()
            a, c = api.torch_to_numpy(a), api.torch_to_numpy(c)
        finally:
            gb.close()
    assert sorted(a) == sorted(c) and all(np.array_equal(a[n], c[n]) for n in a)
    assert KR.differ(KR.unpack(_flat(a), len(b["src"]), 7, flags), want) == []


@both_bytes
def test_exported_tensors_survive_a_later_call(T, byte):
    """dag() on the handle takes the working memory (and poisons it); the tensors are the caller's."""
    api = T.api()
    b, flags = _sets()["dag"], KR.WT
    want = _want(api, "dag", b, 100, flags)
    with poisoned(api, byte):
        gb = guarded(api, _make, api, b, "upload")
        try:
            sz = guarded(api, gb.ksw_solve, b["src"], b["sink"], 100, **_kw(flags))
            t = guarded(api, gb.ksw_export, sz)
            guarded(api, gb.dag, b["src"])
            with pytest.raises(api.AlignasmError) as ei:
                gb.ksw_export(sz)
            assert ei.value.code == KR.E_INVAL
            o = api.torch_to_numpy(t)
        finally:
            gb.close()
    assert KR.differ(KR.unpack(_flat(o), len(b["src"]), 100, flags), want) == []


@both_bytes
def test_mixed_status_batches(T, byte):
    """A cycle among DAGs in DAG mode, a negative cycle among clean graphs with cycles + negative: the graph gets AASM_E_INVAL and
    no room, its neighbours are solved."""
    api = T.api()
    dags = KC.random_graphs(20274, 5)
    neg = BC.golden_graphs()
    bad, clean = [g for g in neg if g["want"] is None and g["n"] < 400][:2], [g for g in neg if g["want"] is not None and g["n"] < 400][:4]
    assert len(bad) == 2 and len(clean) == 4
    for name, gs, flags, at in (("cycle among dags", dags[:2] + [KC.cycle_graph()] + dags[2:] + [KC.cycle_graph()], KR.WT, (2, 6)),
                                ("negative cycle among clean", clean[:1] + bad[:1] + clean[1:] + bad[1:], KR.WT | KR.MODES["negative"], (1, 5))):
        b = cached(("ksw resident batch", name), lambda: KC.make_batch(gs))
        want = _want(api, name, b, 7, flags)
        assert [int(s) for s in want["status"][list(at)]] == [KR.E_INVAL] * 2 and (np.delete(want["status"], at) == 0).all() and want["n_found"].sum() > 0
        with poisoned(api, byte):
            gb = guarded(api, _make, api, b, "from_torch")
            try:
                assert KR.differ(_got(api, gb, b, 7, flags), want) == [], name
            finally:
                gb.close()
