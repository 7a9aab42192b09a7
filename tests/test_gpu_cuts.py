"""GPU tier of the cut plans: aasm_cut_plans_device (kernel aasm_cut_plans on the MI355X) against the vectors recorded from the
reference's get_edited_paf_data and against the host codec on solver output, through DeviceBatch -> solve -> to_torch(cuts=batch);
the planned writer on plans fetched from the device; one full-size run; the entry's argument checks; plans across a later solve
and on a side stream; hand-made lists at the chunk edges, more chunks than blocks (the grid-stride loop), elements outside their contig,
damaged tags and random clips."""
import numpy as np
import pytest

import cuts_testlib as X
from alignasm_amd import _abi
from test_cs_ref import _accepted_text, _file_level, _paf_line
from test_cuts_cpu import assert_edge_case, assert_fixture_was_covered, check_recorded, edge_file
from test_export_cpu import CASE_IDS, CASES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def emc():
    """The emulated kernel, what the device plans of damaged tags are compared with."""
    return X.build_emul()


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


# ---- the chunk loop, on hand-made lists ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edges(T, torch):
    paf, rows, pools = edge_file(T)
    db = T.api().DeviceBatch(paf)
    yield paf, rows, pools, db, X.view_arrays(paf.view())
    db.close()


@pytest.mark.parametrize("case", X.edge_cases(), ids=lambda c: "%d_%d_%d_%s" % c[:4])
def test_device_kernel_at_the_chunk_edges(T, torch, edges, case):
    """The emulation tier's cases (test_emulated_kernel_at_the_chunk_edges) with 256 lanes per block: the ballot compaction and
    the LDS atomic fill the list to exactly a chunk, one short of it and one into the next.  Every plan against the host codec."""
    paf, rows, pools, db, va = edges
    out = X.edge_lists(rows, pools, *case)
    assert_edge_case(T, va, out, X.device_plans(T.api(), db, out), case)


def test_device_kernel_flags_elements_outside_their_contig(T, torch, edges):
    """AASM_CUT_E_RECORD on the card: ctg_index -1 and ctg_index = the contig's record count (in the last contig: record
    n_records), first and last in a chunk and inside: flags exactly 0x80, every other word 0, the neighbours untouched."""
    paf, rows, pools, db, va = edges
    good, bad, where = X.record_fault_lists(rows, pools)
    assert X.record_of(bad, va["ctg_rec_off"])["main"][-1] == len(rows) == db.n_records
    X.check_record_faults(X.device_plans(T.api(), db, good), X.device_plans(T.api(), db, bad), where)


def test_more_chunks_than_blocks_take_the_grid_stride_loop(T, torch):
    """The recorded-vector batch with every contig's main, alt and .all elements tiled until the three lists hold more than
    4 400 chunks of 2 048 elements (the grid is capped at 4 096 blocks): blocks take a second chunk with the LDS list and the
    search bounds of the first, and for some of them (asserted below) the first chunk is of main or alt and the second of .all.
    The plans equal the un-tiled run's, gathered through the same index, byte for byte (on the device: the arrays hold
    0.9 GB)."""
    api = T.api()
    paf, rows, out, where = X.golden_case_batch(api, X.golden_cs(T), _file_level, _accepted_text)
    db = api.DeviceBatch(paf)
    small = X.device_plans(api, db, out)
    n_small = sum(len(out[k]) for k in X.LISTS)
    t = (4400 * X.CHUNK) // n_small + 1
    C = out["n_contigs"]
    idx = {}
    for k in ("main", "alt"):
        o = out[k + "_off"]
        idx[k] = np.concatenate([np.tile(np.arange(o[c], o[c + 1]), t) for c in range(C)])
    po, eo = out["all_path_off"], out["all_elem_off"]
    path_idx = np.concatenate([np.tile(np.arange(po[c], po[c + 1]), t) for c in range(C)])     # every contig's paths, t times
    lens = np.diff(eo)[path_idx]
    big_eo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx["all"] = (np.repeat(eo[path_idx] - big_eo[:-1], lens) + np.arange(big_eo[-1])).astype(np.int64)
    offs = {"main_off": out["main_off"] * t, "alt_off": out["alt_off"] * t, "all_path_off": po * t, "all_elem_off": big_eo}
    ch0 = np.cumsum([0] + [-(-len(idx[k]) // X.CHUNK) for k in X.LISTS])      # list l owns the chunks [ch0[l], ch0[l + 1])
    n_chunks, blocks = int(ch0[3]), 4096                                       # AASM_CUT_MAX_BLOCKS
    assert n_chunks > blocks + 256 and all(len(idx[k]) > 2 * X.CHUNK for k in X.LISTS)
    second = np.arange(blocks, n_chunks)                                       # block b's second chunk is chunk b + 4096
    l_first, l_second = np.searchsorted(ch0, second - blocks, "right") - 1, np.searchsorted(ch0, second, "right") - 1
    assert ((l_first < 2) & (l_second == 2)).any()                             # blocks go from main or alt on to .all, whose search starts at the paths
    dev = torch.device("cuda", db.device)
    el_small = {k: torch.from_numpy(np.ascontiguousarray(out[k]).view(np.int64).reshape(-1, 5)).to(dev) for k in X.LISTS}
    p_small = {k: torch.from_numpy(np.ascontiguousarray(small[k]).view(np.int64).reshape(-1, 6)).to(dev) for k in X.LISTS}
    ix = {k: torch.from_numpy(idx[k]).to(dev) for k in X.LISTS}
    el = {k: el_small[k][ix[k]].contiguous() for k in X.LISTS}
    t_off = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.int64)).to(dev) for k, v in offs.items()}
    plans = {k: torch.full((len(idx[k]), 6), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device=dev) for k in X.LISTS}
    sizes = _abi.OutSizes(C, len(idx["main"]), len(idx["alt"]), len(big_eo) - 1, len(idx["all"]))
    dev_out = _abi.DevOut(t_off["main_off"].data_ptr(), t_off["alt_off"].data_ptr(), t_off["all_path_off"].data_ptr(), t_off["all_elem_off"].data_ptr(),
                          el["main"].data_ptr(), el["alt"].data_ptr(), el["all"].data_ptr(), None)
    st = torch.cuda.current_stream(dev)
    rc = api.cut_plans_raw(db.dev_view, sizes, dev_out, _abi.DevCuts(*(plans[k].data_ptr() for k in X.LISTS)), db.device, st.cuda_stream)
    assert rc == 0, (rc, api.LIB.aasm_last_error())
    st.synchronize()
    for k in X.LISTS:
        assert bool(torch.equal(plans[k], p_small[k][ix[k]])), k
    db.close()


def test_device_kernel_equals_the_emulation_on_damaged_tags(T, torch, emc):
    """The damaged-tag corpus and clips of the sanitizer test, the rows the reader takes with device ranges (the others lack the
    'cs:Z:' prefix, a reader error): the device plans equal the emulated kernel's byte for byte."""
    api = T.api()
    rows, per = X.damaged_corpus()
    taken = []
    for i, r in enumerate(rows):
        try:
            api.Paf.parse(_paf_line(r, "d"), device_ranges=True).close()
            taken.append(i)
        except api.AlignasmError:
            pass
    assert len(taken) >= 800 and len(rows) - len(taken) >= 20
    paf = api.Paf.parse(b"".join(_paf_line(rows[i], "d%d" % i) for i in taken), device_ranges=True)
    assert paf.n_contigs == len(taken)
    out = X.elements([per[i] for i in taken])
    want = X.emul_plans(emc, paf.view(), out)
    db = api.DeviceBatch(paf)
    got = X.device_plans(api, db, out)
    db.close()
    assert got["main"].tobytes() == want["main"].tobytes() and len(want["main"]) == 10 * len(taken)
    f = want["main"]["flags"]
    assert (f & _abi.AASM_CUT_E_TAG != 0).sum() > 100 and (f & _abi.AASM_CUT_ERRORS == 0).sum() >= len(taken)


def test_device_kernel_equals_the_host_codec_on_random_clips(T, torch):
    """tests/cs_cases.py's random clips of 1 400 accepted rows (ends on matched bases, anywhere, inconsistent reference spans)
    against the host codec."""
    api = T.api()
    rows, per = X.random_clip_corpus(T)
    paf = api.Paf.parse(b"".join(_paf_line(r, "r%d" % i) for i, r in enumerate(rows)), device_ranges=True)
    assert paf.n_contigs == len(rows)
    out = X.elements(per)
    db = api.DeviceBatch(paf)
    n = X.check_against_host(T, X.view_arrays(paf.view()), out, X.device_plans(api, db, out))
    db.close()
    assert n["cut"] > 1500 and n["errors"] > 100 and n["irregular"] > 0, n
