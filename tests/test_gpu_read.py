"""GPU tier of the device reader: aasm_paf_parse_device (kernels aasm_read_* on the MI355X) on every case of tests/read_cases.py
against the host reader, the I/O oracle and an uploaded batch, the large and long-row ones again with capped grids; the pipe path of
aasm_paf_read_device; the error contract; parse_device -> solve -> fetch -> cut plans ->
written files end to end; `alignasm --device-reader`; device memory after a read."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import cuts_testlib as XC
import read_cases as RC
import read_testlib as X
from alignasm_amd import _abi
from test_golden import SUFFIXES, _variants
from test_read_cpu import _case_ids, check_case

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("the GPU tier needs torch to see the device")
    return torch


@pytest.fixture(scope="module")
def synth_text(T):
    return T.api().Paf.synth(200, 50, 11, dup_every=9, shuffle=True).to_text()


@pytest.fixture(scope="module")
def cases(synth_text):
    return RC.valid_cases(synth_text)


# ---- 1. every valid case ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _case_ids())
def test_device_reader_equals_host_reader_oracle_and_upload(T, cases, name):
    api = T.api()
    fetch = X.hip_fetcher(api)
    case = next(c for c in cases if c["name"] == name)
    host = api.Paf.parse(case["text"], device_ranges=True)
    up = api.DeviceBatch(host)                                       # what aasm_upload_batch gives for the host-read container
    want_dev = X.view_arrays(up.dev_view, fetch)
    modes = [0] + ([_abi.AASM_READ_H_WEAK_HASH] if case["weak"] else [])
    if RC.few_blocks(case):                                          # 3 blocks per grid: the grid-stride loops, wave operations inside
        modes += [f | _abi.AASM_READ_H_FEW_BLOCKS for f in modes]
    for flags in modes:
        before = api.debug_counter("read_host_fallbacks")
        paf, db = api.Paf.parse_device(case["text"], _flags=flags)
        assert api.debug_counter("read_host_fallbacks") == before   # conditions, not measurements: the device did the work ...
        assert api.debug_counter("read_slow_rows") == case["slow"]  # ... and the host patched exactly the rows that need strtoll
        got_dev = X.view_arrays(db.dev_view, fetch)
        check_case(T, api, case, paf.to_text(), X.view_arrays(paf.view()), got_dev)
        assert X.diff_views(want_dev, got_dev) == []
        db.close(); paf.close()
    up.close()


def test_case_list_is_complete(cases):
    assert sorted(_case_ids()) == sorted(c["name"] for c in cases)
    few = [c["name"] for c in cases if RC.few_blocks(c)]
    assert {"synth_file", "refs_more_than_64", "long_one_row_per_tile", "long_1mib_only", "ref_names_5000_differ_in_last_byte"} <= set(few)


def test_device_reader_halves(T, cases):
    """paf = NULL gives the batch alone, up = dev_view = NULL the container alone."""
    api = T.api()
    fetch = X.hip_fetcher(api)
    text = next(c for c in cases if c["name"] == "slow_numbers")["text"]
    paf, db = api.Paf.parse_device(text)
    up, view, h = C.c_void_p(), _abi.BatchIn(), C.c_void_p()
    assert api.LIB.aasm_paf_parse_device(text, len(text), 0, 0, None, C.byref(up), C.byref(view)) == 0
    assert X.diff_views(X.view_arrays(db.dev_view, fetch), X.view_arrays(view, fetch)) == []
    api.LIB.aasm_upload_free(up)
    assert api.LIB.aasm_paf_parse_device(text, len(text), 0, 0, C.byref(h), None, None) == 0
    only = api.Paf(h)
    assert only.to_text() == paf.to_text()


@pytest.mark.parametrize("which", ["tiny", "long_1mib_between"])
def test_read_device_from_a_pipe(T, cases, which, tmp_path):
    """aasm_paf_read_device on what is no regular file: read into memory, then the same as parse_device on those bytes."""
    api = T.api()
    fetch = X.hip_fetcher(api)
    text = open(os.path.join(G, "files", "tiny.paf"), "rb").read() if which == "tiny" else next(c for c in cases if c["name"] == which)["text"]
    fifo = str(tmp_path / "in.paf")
    os.mkfifo(fifo)

    def write():
        with open(fifo, "wb") as f:
            f.write(text)
    writer = threading.Thread(target=write, daemon=True)
    writer.start()
    paf, db = api.Paf.read_device(fifo)                              # (opens the pipe first of all, which lets the writer go)
    writer.join(10)
    assert not writer.is_alive()
    want_paf, want_db = api.Paf.parse_device(text)
    assert X.diff_views(X.view_arrays(want_paf.view()), X.view_arrays(paf.view())) == [] and paf.to_text() == want_paf.to_text()
    assert X.diff_views(X.view_arrays(want_db.dev_view, fetch), X.view_arrays(db.dev_view, fetch)) == []
    assert X.diff_views(X.host_read(api, text)[1], X.view_arrays(db.dev_view, fetch)) == []
    db.close(); want_db.close()


# ---- 2. errors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _ in RC.error_cases()])
def test_device_reader_reports_the_host_readers_error(T, name):
    api = T.api()
    text = dict(RC.error_cases())[name]
    code, msg = X.host_error(api, text)
    before = api.debug_counter("read_host_fallbacks")
    with pytest.raises(api.AlignasmError) as ei:
        api.Paf.parse_device(text)
    assert ei.value.code == code == _abi.AASM_E_PARSE and str(ei.value).split(": ", 1)[1] == msg
    assert api.debug_counter("read_host_fallbacks") == before + 1


def test_malformed_tag_alone_fails_in_the_solve(T):
    api = T.api()
    text = RC.bad_tag_only()
    paf, db = api.Paf.parse_device(text)
    assert paf.to_text() == api.Paf.parse(text, device_ranges=True).to_text()
    with pytest.raises(api.AlignasmError) as got:
        db.solve(max_paths=4)
    up = api.DeviceBatch(api.Paf.parse(text, device_ranges=True))
    with pytest.raises(api.AlignasmError) as want:
        up.solve(max_paths=4)
    assert got.value.code == want.value.code == _abi.AASM_E_PARSE and str(got.value) == str(want.value)
    db.close(); up.close()


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------
def _texts(synth_text):
    return {"synth": synth_text, "tiny": open(os.path.join(G, "files", "tiny.paf"), "rb").read(), "dense": open(os.path.join(G, "files", "dense.paf"), "rb").read()}


@pytest.mark.parametrize("which", ["synth", "tiny", "dense"])
def test_parse_device_solve_fetch_cut_plans(T, torch, synth_text, which, tmp_path):
    api = T.api()
    text = _texts(synth_text)[which]
    paf, db = api.Paf.parse_device(text)
    host = api.Paf.parse(text, device_ranges=True)
    up = api.DeviceBatch(host)
    for K in (4, 16):
        res, ref = db.solve(max_paths=K), None
        got = res.fetch()
        d = res.to_torch(cuts=db)
        torch.cuda.current_stream(db.device).synchronize()
        plans = api.cuts_to_numpy(d)
        res.close()
        ref = up.solve(max_paths=K)
        want = ref.fetch()
        d = ref.to_torch(cuts=up)
        torch.cuda.current_stream(up.device).synchronize()
        want_plans = api.cuts_to_numpy(d)
        ref.close()
        for k in T.OUT_KEYS:
            assert got[k].tobytes() == want[k].tobytes(), (K, k)
        for k in XC.LISTS:
            assert plans[k].tobytes() == want_plans[k].tobytes(), (K, k)
    db.close(); up.close()


@pytest.mark.parametrize("name", ["tiny", "dense"])
def test_written_outputs_equal_the_golden_files(T, name, tmp_path):
    api = T.api()
    paf, db = api.Paf.read_device(os.path.join(G, "files", name + ".paf"))
    res = db.solve(max_paths=10000)
    bo = res.fetch_raw()
    try:
        got = XC.write_three(paf, bo, tmp_path, "dev")
    finally:
        api.free_out(bo)
    res.close(); db.close()
    sub = "" if name == "tiny" else "dense"
    assert got == [open(os.path.join(G, "files", sub, name + s), "rb").read() for s in SUFFIXES]


# ---- 4. the command line ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [v for v in _variants() if v[0] in ("", "alt", "dense_k4")], ids=lambda v: v[0] or "default")
def test_cli_device_reader_writes_the_same_files(T, tmp_path, variant):
    sub, inp, alt, flags, _K, _nsl, _base = variant
    exe = os.path.join(T.ROOT, "alignasm_amd", "alignasm")
    for name in (inp, alt):
        if name:
            (tmp_path / name).write_bytes(open(os.path.join(G, "files", name), "rb").read())
    flags = [str(tmp_path / f) if f.endswith(".paf") else f for f in flags]
    stem, runs = inp[:-4], []
    for extra in ([], ["--device-reader"]):
        r = subprocess.run([exe, str(tmp_path / inp)] + flags + extra, capture_output=True, text=True)
        files = []
        for suffix in SUFFIXES:
            files.append((tmp_path / (stem + suffix)).read_bytes())
            (tmp_path / (stem + suffix)).unlink()
        runs.append((r.returncode, r.stdout, r.stderr, files))
    assert runs[0] == runs[1] and runs[0][0] == 0
    assert runs[1][3] == [open(os.path.join(G, "files", sub, stem + s), "rb").read() for s in SUFFIXES]


def test_cli_device_reader_streaming_shape_and_bad_files(T, tmp_path):
    """A file above the range path's thresholds (solved in place instead), a bad row, a malformed tag, the usage error."""
    api = T.api()
    exe = os.path.join(T.ROOT, "alignasm_amd", "alignasm")
    src = tmp_path / "s.paf"
    api.Paf.synth(120, 600, 3, dup_every=7).save(str(src))
    few = tmp_path / "few.paf"
    few.write_bytes(dict(RC.error_cases())["later_kind_first"])
    tag = tmp_path / "tag.paf"
    tag.write_bytes(RC.bad_tag_only())
    for path, code in ((src, 0), (few, 1), (tag, 1)):
        runs = []
        for extra in ([], ["--device-reader"]):
            r = subprocess.run([exe, str(path), "--max-paths", "16"] + extra, capture_output=True, text=True)
            files = []
            for suffix in SUFFIXES:
                p = tmp_path / (path.name[:-4] + suffix)
                files.append(p.read_bytes() if p.exists() else None)
                if p.exists():
                    p.unlink()
            runs.append((r.returncode, r.stdout, r.stderr, files))
        assert runs[0] == runs[1] and runs[0][0] == code, (path.name, runs[0][:3], runs[1][:3])
        assert (runs[0][3][0] is not None) == (code == 0)
    assert "Missing cs:Z tag" in subprocess.run([exe, str(few), "--device-reader"], capture_output=True, text=True).stderr
    r = subprocess.run([exe, str(src), "--device-reader", "--host-ranges"], capture_output=True, text=True)
    assert r.returncode == 1 and "Usage" in r.stderr and not (tmp_path / "s.aln.paf").exists()


# ---- 5. memory ----------------------------------------------------------------------------------------------------------------
def test_a_warm_read_leaves_no_device_memory_behind(T, torch, synth_text):
    api = T.api()
    paf, db = api.Paf.parse_device(synth_text)                       # (warm: the context, the scan's scratch words)
    db.close()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    mallocs = api.debug_counter("device_mallocs")
    paf, db = api.Paf.parse_device(synth_text)
    held = free0 - torch.cuda.mem_get_info(0)[0]
    assert held >= len(synth_text) // 2                              # the batch is resident: the tags are most of the text
    assert held < 3 * len(synth_text) + (64 << 20)                   # ... and the raw text and the row scratch are gone
    db.close()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] == free0
    assert api.debug_counter("device_mallocs") == mallocs            # (the arena was not touched)
