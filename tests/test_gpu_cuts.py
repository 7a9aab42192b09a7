"""GPU tier of the cut plans: aasm_cut_plans_device (kernel aasm_cut_plans on the MI355X) against the vectors recorded from the
reference's get_edited_paf_data and against the host codec on solver output, through DeviceBatch -> solve -> to_torch(cuts=batch);
the planned writer on plans fetched from the device; one full-size run; the entry's argument checks; plans across a later solve
and on a side stream."""
import numpy as np
import pytest

import cuts_testlib as X
from alignasm_amd import _abi
from test_cs_ref import _accepted_text, _file_level
from test_cuts_cpu import assert_fixture_was_covered, check_recorded
from test_export_cpu import CASE_IDS, CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("the GPU tier needs torch to see the device")
    return torch


def solved_on_device(T, torch, case=None, paf=None, K=None, nsl=False):
    """-> (paf, device batch, result, exported arrays as numpy, plans as numpy)."""
    api = T.api()
    if paf is None:
        nc, nr, seed, K, dense, dup, shuf, heavy, nsl = case
        paf = api.Paf.synth(nc, nr, seed, dense=dense, heavy_tail=heavy, dup_every=dup, shuffle=shuf)
    db = api.DeviceBatch(paf, cs_only=True)
    res = db.solve(max_paths=K, non_skip_linkable=nsl)
    d = res.to_torch(cuts=db)
    torch.cuda.current_stream(db.device).synchronize()
    return paf, db, res, api.torch_to_numpy(d), api.cuts_to_numpy(d)


def test_to_torch_without_cuts_is_unchanged(T, torch):
    api = T.api()
    db = api.DeviceBatch(T.synth(6, 60, 3, dup_every=3))
    res = db.solve(max_paths=10000)
    assert sorted(res.to_torch()) == sorted(["main_off", "alt_off", "all_path_off", "all_elem_off", "main", "alt", "all", "status", "n_contigs"])
    res.close(); db.close()


def test_device_kernel_equals_the_recorded_reference_vectors(T, torch):
    api = T.api()
    paf, rows, out, where = X.golden_case_batch(api, X.golden_cs(T), _file_level, _accepted_text)
    db = api.DeviceBatch(paf)
    plans = X.device_plans(api, db, out)
    assert_fixture_was_covered(check_recorded(rows, out, where, plans))
    db.close()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_device_kernel_equals_the_host_codec_on_solver_output(T, torch, case):
    paf, db, res, out, plans = solved_on_device(T, torch, case)
    want = res.fetch()
    for k in X.LISTS:
        assert out[k].tobytes() == want[k].tobytes()
    n = X.check_against_host(T, X.view_arrays(paf.view()), out, plans)
    assert n["elements"] == len(out["main"]) + len(out["alt"]) + len(out["all"]) and n["errors"] == 0
    if case[1] > 1:
        assert n["cut"] >= 0.25 * n["elements"], n
    if case[5] and case[3] > 1:
        assert len(out["all"]) > 0 and any(int(f) & 1 for f in plans["all"]["flags"])
    res.close(); db.close()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_planned_writer_with_device_plans_writes_the_same_bytes(T, torch, case, tmp_path):
    paf, db, res, out, plans = solved_on_device(T, torch, case)
    bo = res.fetch_raw()
    try:
        want = X.write_three(paf, bo, tmp_path, "walk")
        assert X.write_three(paf, bo, tmp_path, "plan", cuts=plans) == want and len(want[0]) > 0
    finally:
        T.api().free_out(bo)
    res.close(); db.close()


def test_planned_writer_reads_the_device_plans(T, torch, tmp_path):
    """The seeded faults of the CPU tier (a changed head_keep, every error flag, a stretch outside the tag, a plan of the wrong
    kind, wrong counts) on plans fetched from the device."""
    paf, db, res, out, plans = solved_on_device(T, torch, CASES[2])
    bo = res.fetch_raw()
    try:
        want = X.write_three(paf, bo, tmp_path, "f_walk")
        assert X.write_three(paf, bo, tmp_path, "f_plan", cuts=plans) == want
        X.seeded_writer_faults(T.api(), paf, bo, plans, want, tmp_path)
    finally:
        T.api().free_out(bo)
    res.close(); db.close()


@pytest.mark.parametrize("name", ["tiny", "dense"])
def test_planned_writer_with_device_plans_golden_files(T, torch, name, tmp_path):
    import os
    paf = T.api().Paf.read(os.path.join(T.GOLDEN, "files", name + ".paf"))
    paf, db, res, out, plans = solved_on_device(T, torch, paf=paf, K=10000)
    bo = res.fetch_raw()
    try:
        assert X.write_three(paf, bo, tmp_path, "plan", cuts=plans) == X.write_three(paf, bo, tmp_path, "walk")
    finally:
        T.api().free_out(bo)
    res.close(); db.close()


def test_full_size_run_equals_the_host_codec(T, torch):
    """C3 (5 000 contigs x 1 000 records, seed 21) at K = 4: every element's kind against its record, and a random sample plus
    every IRREGULAR or error-flagged element against the host codec."""
    api = T.api()
    paf = api.Paf.synth(5000, 1000, 21)
    paf, db, res, out, plans = solved_on_device(T, torch, paf=paf, K=4)
    va = X.view_arrays(paf.view())
    rec = X.record_of(out, va["ctg_rec_off"])
    rng = np.random.default_rng(5)
    which, n_cut = {}, 0
    for k in X.LISTS:
        f = plans[k]["flags"]
        uncut = (out[k]["qs"] == va["qry_str"][rec[k]]) & (out[k]["qe"] == va["qry_end"][rec[k]])
        assert np.array_equal((f & _abi.AASM_CUT_IS_CUT) == 0, uncut)
        assert (plans[k]["reserved"] == 0).all() and ((f & ~0xf3) == 0).all()
        n_cut += int((~uncut).sum())
        odd = np.flatnonzero(f & (_abi.AASM_CUT_IRREGULAR | _abi.AASM_CUT_ERRORS))
        pick = rng.choice(len(f), size=min(len(f), 4000), replace=False) if len(f) else np.zeros(0, np.int64)
        which[k] = sorted(set(odd.tolist()) | set(pick.tolist()))
    assert n_cut > 100000
    n = X.check_against_host(T, va, out, plans, which)
    assert n["errors"] == 0 and n["cut"] > 1000
    res.close(); db.close(); paf.close()


def test_cut_plans_reject_bad_arguments_and_write_nothing(T, torch):
    from alignasm_amd._abi import DevCuts, DevOut, OutSizes
    api = T.api()
    paf = api.Paf.synth(12, 100, 5, dup_every=3)
    db = api.DeviceBatch(paf, cs_only=True)
    res = db.solve(max_paths=10000)
    d = res.to_torch()
    sz = res.sizes()
    assert sz["n_all_elems"] > 0 and sz["n_main"] > 0 and sz["n_alt"] > 0
    dev = torch.device("cuda", 0)
    bufs = [torch.full((sz[n], 6), -5, dtype=torch.int64, device=dev) for n in ("n_main", "n_alt", "n_all_elems")]
    torch.cuda.synchronize()
    ptrs = [b.data_ptr() for b in bufs]
    good = OutSizes(*(sz[n] for n, _ in OutSizes._fields_))
    dev_out = DevOut(*(d[k].data_ptr() for k in ("main_off", "alt_off", "all_path_off", "all_elem_off", "main", "alt", "all", "status")))
    stream = torch.cuda.current_stream(0).cuda_stream
    host = np.zeros(6 * sz["n_main"] + 8, np.int64)
    calls = []
    p = list(ptrs); p[0] = host.ctypes.data                          # a destination in host memory
    calls.append((db.dev_view, good, dev_out, DevCuts(*p)))
    for i in range(3):                                               # each non-empty list NULL in turn
        p = list(ptrs); p[i] = None
        calls.append((db.dev_view, good, dev_out, DevCuts(*p)))
    p = list(ptrs); p[2] = ptrs[2] + 4                               # misaligned
    calls.append((db.dev_view, good, dev_out, DevCuts(*p)))
    o = DevOut(*(d[k].data_ptr() for k in ("main_off", "alt_off", "all_path_off", "all_elem_off", "main", "alt", "all", "status")))
    o.main_elems = None                                              # a source list NULL
    calls.append((db.dev_view, good, o, DevCuts(*ptrs)))
    wrong = OutSizes(*(sz[n] for n, _ in OutSizes._fields_))
    wrong.n_contigs += 1                                             # sizes of another batch
    calls.append((db.dev_view, wrong, dev_out, DevCuts(*ptrs)))
    no_cs = api.DeviceBatch(paf)                                     # uploaded with match ranges: no tags on the device
    assert not no_cs.dev_view.cs_text
    calls.append((no_cs.dev_view, good, dev_out, DevCuts(*ptrs)))
    for i, c in enumerate(calls):
        assert api.cut_plans_raw(*c, 0, stream) == -1, i
    torch.cuda.synchronize()
    for b in bufs:
        assert (b == -5).all()
    assert api.cut_plans_raw(db.dev_view, good, dev_out, DevCuts(*ptrs), 0, stream) == 0   # the same arguments, corrected, go through
    torch.cuda.synchronize()
    plans = api.cuts_to_numpy(dict(zip(("main_cut", "alt_cut", "all_cut"), bufs)))
    n = X.check_against_host(T, X.view_arrays(paf.view()), api.torch_to_numpy(d), plans)
    assert n["cut"] > 0
    for x in (res, db, no_cs):
        x.close()


def test_plans_survive_the_next_solve(T, torch):
    api = T.api()
    paf, db, res, out, plans = solved_on_device(T, torch, CASES[4])
    d = res.to_torch(cuts=db)
    torch.cuda.synchronize()
    other = api.DeviceBatch(T.synth(60, 200, 4, dense=True))
    res_b = other.solve(max_paths=16)
    torch.cuda.synchronize()
    again = api.cuts_to_numpy(d)
    for k in X.LISTS:
        assert again[k].tobytes() == plans[k].tobytes() and len(plans["main"]) > 0
    for x in (res, res_b, db, other):
        x.close()


def test_export_and_cut_on_a_side_stream_while_the_default_stream_is_busy(T, torch):
    api = T.api()
    paf, db, res, out, plans = solved_on_device(T, torch, CASES[7])
    a = torch.randn(4096, 4096, device="cuda:0")
    side = torch.cuda.Stream(0)
    for _ in range(40):                                              # the default stream has work queued for a while
        a = (a @ a).clamp_(-1, 1)
    with torch.cuda.stream(side):
        d = res.to_torch(stream=side, cuts=db)
        main_cut, all_cut, main = d["main_cut"].clone(), d["all_cut"] * 1, d["main"].clone()   # consumed on the side stream, nothing in between
    side.synchronize()
    assert main.cpu().numpy().tobytes() == out["main"].tobytes()
    assert main_cut.cpu().numpy().tobytes() == plans["main"].tobytes() and all_cut.cpu().numpy().tobytes() == plans["all"].tobytes()
    assert len(plans["all"]) > 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a).all())
    res.close(); db.close()
