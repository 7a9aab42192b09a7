"""CPU tier of the device reader's resident row columns (aasm_paf_parse_device_rows / aasm_paf_read_device_rows): the C-ABI
surface, the reader's driver and kernel bodies under AASM_READ_ROW_COLS (1-lane host emulation, tests/host_emul/read_cols_emul.cpp) on
every case of tests/read_cases.py and tests/read_cols_cases.py against rows_host_cols of the host reader's container, host text
and "device" text, free and capped grids; every case text under a host address sanitizer."""
import ctypes as C
import os
import re
import subprocess

import pytest

import read_cases as RC
import read_cols_cases as NC
import read_cols_testlib as XR
import read_testlib as X
import rows_testlib as XW
from alignasm_amd import _abi
from test_read_cpu import _case_ids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "alignasm_amd.h")
NEW_FUNCS = ("aasm_paf_parse_device_rows", "aasm_paf_read_device_rows")


@pytest.fixture(scope="module")
def emrc():
    return XR.build_emul(san=True)


@pytest.fixture(scope="module")
def rows_lib():
    return XW.build_emul()


@pytest.fixture(scope="module")
def cases(T):
    return RC.valid_cases(T.api().Paf.synth(200, 50, 11, dup_every=9, shuffle=True).to_text()) + NC.name_cases()


# ---- 1. the surface ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_rows_reader():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    tail = (r"\s*int\s+flags\s*,\s*int\s+device\s*,\s*aasm_paf\s*\*\*\s*paf\s*,\s*aasm_upload\s*\*\*\s*up\s*,\s*aasm_batch_in\s*\*\s*dev_view\s*,"
            r"\s*(struct\s+)?aasm_row_cols\s*\*\s*dev_cols\s*\)")
    assert re.search(r"int\s+aasm_paf_parse_device_rows\s*\(\s*const\s+char\s*\*\s*text\s*,\s*int64_t\s+len\s*," + tail, src)
    assert re.search(r"int\s+aasm_paf_read_device_rows\s*\(\s*const\s+char\s*\*\s*path\s*," + tail, src)
    assert re.search(r"#define\s+AASM_READ_ROW_COLS\s+2\b", src) and _abi.AASM_READ_ROW_COLS == 2
    assert re.search(r"#define\s+AASM_READ_TEXT_ON_DEVICE\s+4\b", src) and _abi.AASM_READ_TEXT_ON_DEVICE == 4
    assert re.search(r"#define\s+AASM_ABI_VERSION\s+3\b", src)


def test_library_exports_the_rows_reader(T):
    api = T.api()
    for n in NEW_FUNCS:
        assert n in api.EXPORTED and hasattr(api.LIB, n)
    assert api.LIB.aasm_abi_version() == 3
    assert api.debug_counter("read_containers") >= 0


def test_bad_arguments(T, tmp_path):
    api = T.api()
    h, up, view, cols = C.c_void_p(), C.c_void_p(), _abi.BatchIn(), _abi.RowCols()
    text = RC.row()
    f = api.LIB.aasm_paf_parse_device_rows
    I = _abi.AASM_E_INVAL
    assert f(None, 0, 0, 0, None, C.byref(up), C.byref(view), C.byref(cols)) == I
    assert f(text, -1, 0, 0, None, C.byref(up), C.byref(view), C.byref(cols)) == I
    assert f(text, len(text), 0, 0, None, C.byref(up), C.byref(view), None) == I                  # the columns are what the entry is for
    assert f(text, len(text), 0, 0, C.byref(h), None, None, C.byref(cols)) == I
    # device text only without a container: refused before anything touches a device
    assert f(text, len(text), _abi.AASM_READ_TEXT_ON_DEVICE, 0, C.byref(h), C.byref(up), C.byref(view), C.byref(cols)) == I
    g = api.LIB.aasm_paf_read_device_rows
    assert g(None, 0, 0, None, C.byref(up), C.byref(view), C.byref(cols)) == I
    assert g(os.fsencode(tmp_path / "none.paf"), 0, 0, None, C.byref(up), C.byref(view), C.byref(cols)) == _abi.AASM_E_IO
    assert not h and not up
    if api.device_count() == 0:                                      # the loud failure, no fallback (guarded as tests/test_abi.py does)
        with pytest.raises(api.AlignasmError) as ei:
            api.Paf.parse_device(text, container=False)
        assert ei.value.code == _abi.AASM_E_NODEVICE


# ---- 2. the kernel bodies in the 1-lane emulation ---------------------------------------------------------------------------
def test_name_cases_are_what_they_claim(cases):
    by = {c["name"]: c["text"] for c in cases}
    assert sorted(NC.case_ids()) == sorted(c["name"] for c in NC.name_cases())
    assert set(range(1, 41)) | {63, 64, 65, 127, 128, 129} == set(NC.LENGTHS)
    first = [ln.split(b"\t") for ln in by["contig_names_every_length"].split(b"\n") if ln]
    assert [len(f[0]) for f in first[::2]] == NC.LENGTHS and len({f[0] for f in first}) == len(NC.LENGTHS)
    refs = [ln.split(b"\t")[5] for ln in by["ref_names_every_length"].split(b"\n") if ln]
    assert sorted({len(r) for r in refs}) == sorted(NC.LENGTHS) and len(set(refs)) == len(NC.LENGTHS)
    assert by["one_row_contigs_2000"].count(b"\n") == 2000
    last = by["last_row_new_names_no_newline"]
    assert not last.endswith(b"\n") and last.endswith(b"\tcs:Z:") and len(last.rsplit(b"\n", 1)[1].split(b"\t")[5]) == 129


@pytest.mark.parametrize("name", _case_ids() + NC.case_ids())
def test_emulated_columns_equal_the_host_containers(T, emrc, rows_lib, cases, name):
    lib, _ = emrc
    api = T.api()
    case = next(c for c in cases if c["name"] == name)
    host, want_view, _ = X.host_read(api, case["text"])
    want = XR.host_cols(rows_lib, host)
    assert want["ctg_name_off"][0] == 0 and want["chr_name_off"][0] == want["ctg_name_off"][-1]
    for flags in (0, _abi.AASM_READ_H_WEAK_HASH) if case["weak"] else (0,):
        for max_blocks in (0, 3):                                    # 3: fewer blocks than names and rows, the grid-stride loops
            for device_text in (False, True):
                before = lib.emrc_counter(1)
                rc, msg, view, cols = XR.emul_parse(lib, case["text"], flags, max_blocks, device_text)
                assert rc == 0, msg
                assert lib.emrc_counter(1) == before and lib.emrc_counter(0) == case["slow"]
                assert X.diff_views(want_view, view) == [], (flags, max_blocks, device_text)
                assert XR.diff_cols(want, cols) == [], (flags, max_blocks, device_text)


@pytest.mark.parametrize("name", [n for n, _ in RC.error_cases()])
def test_emulated_rows_reader_reports_the_host_readers_error(T, emrc, name):
    lib, _ = emrc
    api = T.api()
    text = dict(RC.error_cases())[name]
    code, msg = X.host_error(api, text)
    for device_text in (False, True):
        before = lib.emrc_counter(1)
        rc, got, view, cols = XR.emul_parse(lib, text, device_text=device_text)
        assert (rc, got) == (code, msg) and view is None and cols is None
        assert lib.emrc_counter(1) == before + 1


# ---- 3. under a host address sanitizer: loads stay inside [0, len), stores inside the exact arrays, nothing leaks ------------
def test_every_case_text_under_the_address_sanitizer(T, emrc, cases, tmp_path):
    _, san = emrc
    paths, want = [], []
    for c in cases:
        p = tmp_path / (c["name"] + ".paf")
        p.write_bytes(c["text"])
        paths.append(str(p))
        host = X.host_read(T.api(), c["text"])[0]
        v = host.view()
        # rows, reference names, bytes of names: from the container's own text
        rows = [ln.split(b"\t") for ln in host.to_text().split(b"\n") if ln]
        ctg, seen = [], []
        for f in rows:
            if not ctg or ctg[-1] != f[0]:
                ctg.append(f[0])
            if f[5] not in seen:
                seen.append(f[5])
        assert len(ctg) == int(v.n_contigs)
        want += ["%s 0 %d %d %d" % (p, len(rows), len(seen), sum(map(len, ctg)) + sum(map(len, seen)))] * 4
    bad = tmp_path / "bad.paf"
    bad.write_bytes(dict(RC.error_cases())["fault_in_last_row_no_newline"])
    r = subprocess.run([san] + paths + [str(bad)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split("\n")[:-1] == want + ["%s %d -1 -1 -1" % (bad, _abi.AASM_E_PARSE)] * 4
