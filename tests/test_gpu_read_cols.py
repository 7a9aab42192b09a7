"""GPU tier of the device reader's resident row columns and the route without a container: aasm_paf_parse_device_rows (kernels
aasm_read_names / aasm_read_row_ids behind the reader's own) on every case of tests/read_cases.py and tests/read_cols_cases.py against
aasm_paf_upload_rows on the host reader's container; again with poisoned working memory; text that is already on the device;
parse -> solve -> plans -> aasm_writer_append_device(paf = NULL) against the golden files and the host writers; the command line
with --device-reader --device-writer."""
import ctypes as C
import os
import subprocess

import pytest

import cuts_testlib as XC
import read_cases as RC
import read_cols_cases as NC
import read_cols_testlib as XR
import read_testlib as X
import text_fuzz as F
from alignasm_amd import _abi
from test_golden import SUFFIXES, _variants
from test_read_cpu import _case_ids

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEVICE_TEXT_CASES = ("synth_file", "slow_numbers", "slow_rows_64", "slow_rows_65", "slow_rows_300", "slow_row_last_no_newline", "names_straddle_tile_edges",
                     "long_1mib_between")


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
    return RC.valid_cases(synth_text) + NC.name_cases()


@pytest.fixture(scope="module")
def yardstick(T, cases):
    """name -> (view arrays, column arrays) of the host-read container, uploaded and fetched back; made once per case."""
    api = T.api()
    fetch = X.hip_fetcher(api)
    made = {}

    def get(name):
        if name not in made:
            host = api.Paf.parse(next(c for c in cases if c["name"] == name)["text"], device_ranges=True)
            up = api.DeviceBatch(host)
            made[name] = (X.view_arrays(up.dev_view, fetch), XR.uploaded_cols(api, host, fetch))
            up.close(); host.close()
        return made[name]
    return get


def _modes(case):
    modes = [0] + ([_abi.AASM_READ_H_WEAK_HASH] if case["weak"] else [])
    if case.get("few") or RC.few_blocks(case):
        modes += [f | _abi.AASM_READ_H_FEW_BLOCKS for f in modes]
    return modes


def _check_batch(api, fetch, db, want):
    want_view, want_cols = want
    assert X.diff_views(want_view, X.view_arrays(db.dev_view, fetch)) == []
    got = XR.cols_arrays(db.row_cols(), db.n_contigs, db.n_records, fetch)
    assert XR.diff_cols(want_cols, got) == []


def _read_all_modes(api, fetch, case, want):
    for flags in _modes(case):
        fallbacks, containers = api.debug_counter("read_host_fallbacks"), api.debug_counter("read_containers")
        paf, db = api.Paf.parse_device(case["text"], _flags=flags, container=False)
        assert paf is None
        assert api.debug_counter("read_host_fallbacks") == fallbacks    # conditions, not measurements: the device did the work,
        assert api.debug_counter("read_slow_rows") == case["slow"]      # the host patched exactly the rows that need strtoll,
        assert api.debug_counter("read_containers") == containers       # and no container was built
        _check_batch(api, fetch, db, want)
        db.close()


# ---- 1 / 2. every valid case and the name shapes --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _case_ids() + NC.case_ids())
def test_resident_columns_equal_the_uploaded_containers(T, cases, yardstick, name):
    api = T.api()
    _read_all_modes(api, X.hip_fetcher(api), next(c for c in cases if c["name"] == name), yardstick(name))


def test_a_container_beside_the_columns_counts(T, cases, yardstick):
    """paf != NULL through the rows entry: the container of aasm_paf_parse_device, the same columns, read_containers + 1."""
    api = T.api()
    fetch = X.hip_fetcher(api)
    text = next(c for c in cases if c["name"] == "slow_numbers")["text"]
    before = api.debug_counter("read_containers")
    h, up, view, cols = C.c_void_p(), C.c_void_p(), _abi.BatchIn(), _abi.RowCols()
    assert api.LIB.aasm_paf_parse_device_rows(text, len(text), 0, 0, C.byref(h), C.byref(up), C.byref(view), C.byref(cols)) == 0
    paf = api.Paf(h)
    assert api.debug_counter("read_containers") == before + 1
    assert paf.to_text() == api.Paf.parse(text, device_ranges=True).to_text()
    want_view, want_cols = yardstick("slow_numbers")
    assert X.diff_views(want_view, X.view_arrays(view, fetch)) == []
    assert XR.diff_cols(want_cols, XR.cols_arrays(cols, int(view.n_contigs), int(view.n_records), fetch)) == []
    api.LIB.aasm_upload_free(up)


# ---- 3. poison: the names block is fresh memory, a byte the kernel skips shows ---------------------------------------------------
@pytest.mark.parametrize("byte", [0xA5, 0xFF])
@pytest.mark.parametrize("name", ["synth_file"] + NC.case_ids())
def test_resident_columns_with_poisoned_memory(T, cases, yardstick, name, byte):
    api = T.api()
    want = yardstick(name)
    prev = api.debug_poison(byte)
    try:
        _read_all_modes(api, X.hip_fetcher(api), next(c for c in cases if c["name"] == name), want)
    finally:
        api.debug_poison(prev)


# ---- 4. text that is already on the device -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DEVICE_TEXT_CASES)
def test_device_text_gives_the_same_batch(T, torch, cases, yardstick, name):
    api = T.api()
    fetch = X.hip_fetcher(api)
    case = next(c for c in cases if c["name"] == name)
    t = torch.frombuffer(bytearray(case["text"]), dtype=torch.uint8).cuda()
    fallbacks, containers = api.debug_counter("read_host_fallbacks"), api.debug_counter("read_containers")
    db = api.DeviceBatch.from_device_text(t)
    assert api.debug_counter("read_host_fallbacks") == fallbacks and api.debug_counter("read_containers") == containers
    assert api.debug_counter("read_slow_rows") == case["slow"]
    _check_batch(api, fetch, db, yardstick(name))
    assert bytes(t.cpu().numpy()) == case["text"]                    # the text is the caller's: unchanged
    db.close()


def test_device_text_refusals(T, torch, cases):
    api = T.api()
    text = next(c for c in cases if c["name"] == "slow_numbers")["text"]
    t = torch.frombuffer(bytearray(b"\n" + text), dtype=torch.uint8).cuda()
    with pytest.raises(api.AlignasmError) as ei:
        api.DeviceBatch.from_device_text(t[1:])                      # a slice from byte 1: not 16-byte aligned
    assert ei.value.code == _abi.AASM_E_INVAL
    h, up, view, cols = C.c_void_p(), C.c_void_p(), _abi.BatchIn(), _abi.RowCols()
    f = api.LIB.aasm_paf_parse_device_rows
    out = (C.byref(up), C.byref(view), C.byref(cols))
    assert f(C.c_void_p(t.data_ptr()), t.numel(), _abi.AASM_READ_TEXT_ON_DEVICE, 0, C.byref(h), *out) == _abi.AASM_E_INVAL   # with a container
    assert f(text, len(text), _abi.AASM_READ_TEXT_ON_DEVICE, 0, None, *out) == _abi.AASM_E_INVAL                            # host memory
    assert not h and not up
    with pytest.raises(api.AlignasmError) as ei:
        api.DeviceBatch.from_device_text(t[16:16])                   # no bytes: the host reader's verdict on an empty text
    assert ei.value.code == _abi.AASM_E_PARSE and str(ei.value).split(": ", 1)[1] == X.host_error(api, b"")[1]


def test_errors_are_the_host_readers_and_leave_nothing_behind(T, torch, synth_text):
    api = T.api()
    _, db = api.Paf.parse_device(synth_text, container=False)        # (warm: the context, the scan's scratch words)
    db.close()
    tensors = {n: torch.frombuffer(bytearray(x if x else b"\0"), dtype=torch.uint8).cuda()[:len(x)] for n, x in RC.error_cases()}
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    mallocs = api.debug_counter("device_mallocs")
    for name, text in RC.error_cases():
        code, msg = X.host_error(api, text)
        for form in ("device text", "host text"):
            before = api.debug_counter("read_host_fallbacks")
            with pytest.raises(api.AlignasmError) as ei:
                if form == "device text":
                    api.DeviceBatch.from_device_text(tensors[name])
                else:
                    api.Paf.parse_device(text, container=False)
            assert ei.value.code == code == _abi.AASM_E_PARSE and str(ei.value).split(": ", 1)[1] == msg, (name, form)
            assert api.debug_counter("read_host_fallbacks") == before + 1
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info(0)[0] == free0
    assert api.debug_counter("device_mallocs") == mallocs            # (the arena was not touched)


# ---- 5. files ------------------------------------------------------------------------------------------------------------------
def _bare_files(api, torch, text, K, nsl, d, stem, piece=0, device_text=False):
    """text -> reader without a container -> solve -> export and plans -> device writer without a container: the three files' bytes."""
    containers = api.debug_counter("read_containers")
    if device_text:
        db = api.DeviceBatch.from_device_text(torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda())
    else:
        _, db = api.Paf.parse_device(text, container=False)
    res = db.solve(max_paths=K, non_skip_linkable=nsl)
    try:
        paths = [str(d / (stem + s)) for s in SUFFIXES]
        db.write_outputs(res.to_torch(cuts=db), *paths, piece_bytes=piece)
        assert api.debug_counter("read_containers") == containers
        return [open(p, "rb").read() for p in paths]
    finally:
        res.close(); db.close()


def _host_files(api, text, K, nsl, d, stem):
    paf = api.Paf.parse(text)
    bo = api.solve_batch_raw(paf.view(), _abi.make_opts(K, nsl, 0, False, False))
    try:
        return XC.write_three(paf, bo, d, stem)
    finally:
        api.free_out(bo)


@pytest.mark.parametrize("variant", [v for v in _variants() if v[2] is None], ids=lambda v: v[0] or "default")
def test_golden_files_without_a_container(T, torch, tmp_path, variant):
    sub, inp, _alt, _flags, K, nsl, _base = variant
    api = T.api()
    text = open(os.path.join(G, "files", inp), "rb").read()
    want = [open(os.path.join(G, "files", sub, inp[:-4] + s), "rb").read() for s in SUFFIXES]
    assert _bare_files(api, torch, text, K, nsl, tmp_path, "a") == want
    assert _bare_files(api, torch, text, K, nsl, tmp_path, "b", piece=1500, device_text=True) == want


def test_synthetic_and_fuzz_files_without_a_container(T, torch, synth_text, tmp_path):
    api = T.api()
    for i, text in enumerate([synth_text] + [F.shaped_text(k) for k in range(6)]):
        K, nsl = (16, False) if i == 0 else F.RUNS[i % 2]
        want = _host_files(api, text, K, nsl, tmp_path, "h%d" % i)
        assert len(want[0]) > 0
        assert _bare_files(api, torch, text, K, nsl, tmp_path, "d%d" % i) == want, i
        if i < 2:                                                    # several pieces per list
            assert _bare_files(api, torch, text, K, nsl, tmp_path, "p%d" % i, piece=1500) == want, i
        if i > 0:
            exp = F.expected(T, text, K, nsl)
            assert exp.kind == "ok" and list(exp.files) == want, i


def test_rejected_results_write_nothing(T, torch, tmp_path):
    """A run the oracle rejects: the append without a container raises rows_flagged_error's code class and message and leaves no
    file; with the container the reference's message comes as before.  A malformed tag fails in the solve."""
    api = T.api()
    i = next(i for i in range(8) if F.expected(T, F.unshaped_text(i), *F.RUNS[i % 2]).kind == "err")
    K, nsl = F.RUNS[i % 2]
    exp = F.expected(T, F.unshaped_text(i), K, nsl)
    _, db = api.Paf.parse_device(F.unshaped_text(i), container=False)
    res = db.solve(max_paths=K, non_skip_linkable=nsl)
    with pytest.raises(api.AlignasmError) as got:
        db.write_outputs(res, *[str(tmp_path / ("d" + s)) for s in SUFFIXES])
    assert got.value.code == _abi.AASM_E_PARSE
    with pytest.raises(api.AlignasmError) as rows:                   # (the message api.rows_flagged_error builds)
        res.to_torch(cuts=db, rows=True)
    assert (rows.value.code, str(rows.value)) == (got.value.code, str(got.value)) and "output elements cannot be formatted; the first: list" in str(got.value)
    assert os.listdir(tmp_path) == []
    res.close(); db.close()
    paf, db = api.Paf.parse_device(F.unshaped_text(i))
    res = db.solve(max_paths=K, non_skip_linkable=nsl)
    with pytest.raises(api.AlignasmError) as want:
        paf.write_outputs_device(db, res, *[str(tmp_path / ("c" + s)) for s in SUFFIXES])
    assert want.value.code == _abi.AASM_E_PARSE and exp.message in str(want.value)
    assert os.listdir(tmp_path) == []
    res.close(); db.close()
    # a malformed tag: read fine, refused by the solve, with the message of the batch uploaded from the container
    text = RC.bad_tag_only()
    _, db = api.Paf.parse_device(text, container=False)
    with pytest.raises(api.AlignasmError) as got:
        db.solve(max_paths=4)
    up = api.DeviceBatch(api.Paf.parse(text, device_ranges=True))
    with pytest.raises(api.AlignasmError) as want:
        up.solve(max_paths=4)
    assert got.value.code == want.value.code == _abi.AASM_E_PARSE and str(got.value) == str(want.value)
    db.close(); up.close()


# ---- 6. the command line -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [v for v in _variants() if v[0] in ("", "dense", "dense_nsl", "dense_k4", "alt")], ids=lambda v: v[0] or "default")
def test_cli_both_flags_write_the_golden_files(T, tmp_path, variant):
    sub, inp, alt, flags, _K, _nsl, _base = variant
    exe = os.path.join(T.ROOT, "alignasm_amd", "alignasm")
    for name in (inp, alt):
        if name:
            (tmp_path / name).write_bytes(open(os.path.join(G, "files", name), "rb").read())
    flags = [str(tmp_path / f) if f.endswith(".paf") else f for f in flags]
    r = subprocess.run([exe, str(tmp_path / inp)] + flags + ["--device-reader", "--device-writer", "--timing"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    plain = subprocess.run([exe, str(tmp_path / inp)] + flags, capture_output=True, text=True)
    timing = [ln for ln in r.stderr.split("\n") if ln.startswith("alignasm timing:")]
    assert len(timing) == 1 and timing[0].endswith(" container %d" % (1 if alt else 0)) and " total_s " in timing[0]
    assert [ln for ln in r.stderr.split("\n") if not ln.startswith("alignasm timing:")] == plain.stderr.split("\n")
    stem = inp[:-4]
    for s in SUFFIXES:
        assert (tmp_path / (stem + s)).read_bytes() == open(os.path.join(G, "files", sub, stem + s), "rb").read(), s
    assert r.stdout == plain.stdout and plain.returncode == 0


def test_cli_both_flags_bad_files_are_reported_as_without_them(T, tmp_path):
    exe = os.path.join(T.ROOT, "alignasm_amd", "alignasm")
    (tmp_path / "tag.paf").write_bytes(RC.bad_tag_only())
    (tmp_path / "few.paf").write_bytes(dict(RC.error_cases())["later_kind_first"])
    (tmp_path / "cut.paf").write_bytes(next(F.unshaped_text(i) for i in range(8) if F.expected(T, F.unshaped_text(i), 10000, False).kind == "err"))
    for name in ("tag", "few", "cut"):
        runs = []
        for extra in ([], ["--device-reader", "--device-writer"]):
            r = subprocess.run([exe, str(tmp_path / (name + ".paf"))] + extra, capture_output=True, text=True)
            runs.append((r.returncode, r.stdout, r.stderr))
            assert [s for s in SUFFIXES if (tmp_path / (name + s)).exists()] == [], (name, extra)
        assert runs[0] == runs[1] and runs[0][0] != 0, (name, runs)
