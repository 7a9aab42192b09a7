"""GPU tier of the device-side export: DeviceResult.to_torch() (aasm_result_sizes + aasm_result_export, the pack kernels on the
MI355X) equals DeviceResult.fetch() (the host pack) array for array, under every selection / chain launch form, at full size,
across a later solve, across torch streams; the export's argument checks."""

import numpy as np
import pytest

from test_export_cpu import CASE_IDS, CASES

pytestmark = pytest.mark.gpu
KEYS = ("main_off", "alt_off", "all_path_off", "all_elem_off", "main", "alt", "all", "status")


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("the GPU tier needs torch to see the device")
    return torch


def _same(want, got, what=""):
    assert want["n_contigs"] == got["n_contigs"], what
    for k in KEYS:
        assert want[k].dtype == got[k].dtype and want[k].shape == got[k].shape, (what, k, want[k].shape, got[k].shape)
        assert want[k].tobytes() == got[k].tobytes(), (what, k)


def _exported(api, torch, res):
    d = res.to_torch()
    torch.cuda.current_stream(res.device).synchronize()
    return api.torch_to_numpy(d)


def _check(T, torch, hb, K, nsl=False, **hooks):
    api = T.api()
    db = api.DeviceBatch(hb)
    res = db.solve(max_paths=K, non_skip_linkable=nsl, **hooks)
    got = _exported(api, torch, res)
    want = res.fetch()
    _same(want, got, str(hooks))
    res.close(); db.close()
    return want


@pytest.mark.parametrize("form", ["default", "chain_all", "chain_none", "sequential"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_export_equals_fetch_small_shapes(T, torch, case, form):
    nc, nr, seed, K, dense, dup, shuf, heavy, nsl = case
    hooks = {"default": {}, "chain_all": {"chain": "all"}, "chain_none": {"chain": "none"}, "sequential": {"sequential_select": True}}[form]
    hb = T.synth(nc, nr, seed, dense=dense, dup_every=dup, shuffle=shuf, heavy_tail=heavy)
    _check(T, torch, hb, K, nsl, **hooks)


def test_export_with_empty_and_single_record_contigs(T, torch):
    """Contigs of no record and of one record between ordinary ones."""
    from alignasm_amd._abi import HostBatch
    hb = T.synth(6, 30, 41, dup_every=3)
    a = dict(hb.arrays)
    off = a["ctg_rec_off"]
    a["ctg_rec_off"] = np.concatenate([[0], np.repeat(off[1:], 2)]).astype(np.int64)   # an empty contig after each one
    mixed = HostBatch(a)
    want = _check(T, torch, mixed, 10000)
    assert want["n_contigs"] == 12 and (np.diff(want["main_off"])[1::2] == 0).all()
    _check(T, torch, T.synth(9, 1, 5), 10000)


@pytest.mark.parametrize("shape", ["c3_k4", "c3_k10000", "c3_dup3", "c5_share"])
def test_export_equals_fetch_full_size(T, torch, shape):
    api = T.api()
    n, r, seed, K, kw = {"c3_k4": (5000, 1000, 21, 4, {}), "c3_k10000": (5000, 1000, 21, 10000, {}),
                         "c3_dup3": (5000, 1000, 21, 4, {"dup_every": 3}), "c5_share": (1250, 1000, 31, 16, {"dense": True})}[shape]
    paf = api.Paf.synth(n, r, seed, no_cs=True, **kw)
    db = api.DeviceBatch(paf)
    res = db.solve(max_paths=K)
    got = _exported(api, torch, res)
    want = res.fetch()
    _same(want, got, shape)
    if shape == "c3_dup3":
        assert len(want["all"]) > 0
    res.close(); db.close(); paf.close()


def test_overflow_rerun_duplicate_heavy(T, torch):
    """Every record duplicated at K = 10 000: tie runs long enough that the .all pool's first guess may overflow and the pick is
    re-run at the exact size (there is no small-capacity hook); status and .all still equal the host pack."""
    for sel in (False, True):
        want = _check(T, torch, T.synth(64, 200, 13, dense=True, dup_every=1, shuffle=True), 10000, sequential_select=sel)
        assert len(want["all"]) > 0


def test_exported_tensors_survive_the_next_solve(T, torch):
    api = T.api()
    db_a = api.DeviceBatch(T.synth(40, 120, 3, dup_every=3))
    res_a = db_a.solve(max_paths=10000)
    want_a = res_a.fetch()
    d_a = res_a.to_torch()
    torch.cuda.current_stream(0).synchronize()
    first = api.torch_to_numpy(d_a)
    _same(want_a, first, "A")
    db_b = api.DeviceBatch(T.synth(60, 200, 4, dense=True))
    res_b = db_b.solve(max_paths=16)
    torch.cuda.synchronize()
    _same(want_a, api.torch_to_numpy(d_a), "A after B")
    with pytest.raises(api.AlignasmError) as ei:
        res_a.fetch()
    assert ei.value.code == -1
    with pytest.raises(api.AlignasmError) as ei:
        res_a.sizes()
    assert ei.value.code == -1
    _same(res_b.fetch(), _exported(api, torch, res_b), "B")
    for x in (res_a, res_b, db_a, db_b):
        x.close()


def test_solve_and_export_on_separate_torch_streams(T, torch):
    api = T.api()
    hb = T.synth(30, 150, 9, dup_every=3, shuffle=True)
    db = api.DeviceBatch(hb)
    s1, s2 = torch.cuda.Stream(0), torch.cuda.Stream(0)
    res = db.solve(max_paths=10000, stream=s1.cuda_stream)
    with torch.cuda.stream(s2):
        d = res.to_torch(stream=s2)
        # consumed on the export's stream, no synchronize in between
        main, alle = d["main"].clone(), d["all"] * 1
        eoff_sum, status = d["all_elem_off"].sum(), d["status"].clone()
    s2.synchronize()
    want = res.fetch()
    assert main.cpu().numpy().tobytes() == want["main"].tobytes()
    assert alle.cpu().numpy().tobytes() == want["all"].tobytes()
    assert int(eoff_sum.item()) == int(want["all_elem_off"].sum())
    assert status.cpu().numpy().tobytes() == want["status"].tobytes()
    res.close(); db.close()


def test_export_rejects_bad_arguments_and_writes_nothing(T, torch):
    from alignasm_amd._abi import DevOut, OutSizes
    api = T.api()
    db = api.DeviceBatch(T.synth(12, 100, 5, dup_every=3))
    res = db.solve(max_paths=10000)
    sz = res.sizes()
    assert sz["n_all_paths"] > 0 and sz["n_main"] > 0
    dev = torch.device("cuda", 0)
    c = sz["n_contigs"]
    bufs = [torch.full((n,), -5, dtype=torch.int64, device=dev) for n in (c + 1, c + 1, c + 1, sz["n_all_paths"] + 1)]
    bufs += [torch.full((n, 5), -5, dtype=torch.int64, device=dev) for n in (sz["n_main"], max(sz["n_alt"], 1), sz["n_all_elems"])]
    bufs.append(torch.full((c,), -5, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    ptrs = [b.data_ptr() for b in bufs]
    good = OutSizes(*(sz[n] for n, _ in OutSizes._fields_))
    host = np.zeros(5 * sz["n_main"] + 8, np.int64)
    stream = torch.cuda.current_stream(0).cuda_stream
    bad_sizes = OutSizes(*(sz[n] for n, _ in OutSizes._fields_))
    bad_sizes.n_main += 1
    assert res.export_raw(bad_sizes, DevOut(*ptrs), stream) == -1
    p = list(ptrs); p[4] = host.ctypes.data                            # main_elems in host memory
    assert res.export_raw(good, DevOut(*p), stream) == -1
    for i in range(8):                                               # each non-empty list NULL in turn
        p = list(ptrs); p[i] = None
        if i == 5 and sz["n_alt"] == 0:
            continue
        assert res.export_raw(good, DevOut(*p), stream) == -1, i
    p = list(ptrs); p[6] = ptrs[6] + 4                               # misaligned
    assert res.export_raw(good, DevOut(*p), stream) == -1
    torch.cuda.synchronize()
    for b in bufs:
        assert (b == -5).all()
    assert res.export_raw(good, DevOut(*ptrs), stream) == 0          # and the same arguments, corrected, go through
    torch.cuda.synchronize()
    want = res.fetch()
    assert bufs[4].cpu().numpy().tobytes() == want["main"].tobytes()
    res.close(); db.close()


def test_repeated_exports_in_flight_on_a_side_stream(T, torch):
    """to_torch twice on one result on a side stream, then sizes() again, with no synchronize in between: the second call must
    not rebuild the scratch the first export is still reading (sizes are computed once per result); both copies equal fetch."""
    api = T.api()
    paf = api.Paf.synth(5000, 1000, 21, no_cs=True, dup_every=3)   # big enough that the first export is still running
    db = api.DeviceBatch(paf)
    res = db.solve(max_paths=4)
    s2 = torch.cuda.Stream(0)
    with torch.cuda.stream(s2):
        d1 = res.to_torch(stream=s2)
        d2 = res.to_torch(stream=s2)
        sz = res.sizes()
    s2.synchronize()
    want = res.fetch()
    assert sz["n_all_paths"] == len(want["all_elem_off"]) - 1 and sz["n_all_elems"] == len(want["all"]) > 0
    _same(want, api.torch_to_numpy(d1), "first")
    _same(want, api.torch_to_numpy(d2), "second")
    res.close(); db.close(); paf.close()
