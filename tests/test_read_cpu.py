"""CPU tier of the device reader (aasm_paf_parse_device / aasm_paf_read_device): the C-ABI surface and the ctypes signatures, the
kernel bodies and their driver (1-lane host emulation, tests/host_emul/read_emul.cpp) on every case of tests/read_cases.py against the
I/O oracle and the host reader, the error contract, and the framing cases under a host address sanitizer."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import read_cases as RC
import read_testlib as X
from alignasm_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "alignasm_amd.h")
NEW_FUNCS = ("aasm_paf_parse_device", "aasm_paf_read_device")


@pytest.fixture(scope="module")
def emr():
    return X.build_emul(san=True)


@pytest.fixture(scope="module")
def cases(T):
    return RC.valid_cases(T.api().Paf.synth(200, 50, 11, dup_every=9, shuffle=True).to_text())


# ---- 1. the surface ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_device_reader():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    tail = r"\s*int\s+flags\s*,\s*int\s+device\s*,\s*aasm_paf\s*\*\*\s*paf\s*,\s*aasm_upload\s*\*\*\s*up\s*,\s*aasm_batch_in\s*\*\s*dev_view\s*\)"
    assert re.search(r"int\s+aasm_paf_parse_device\s*\(\s*const\s+char\s*\*\s*text\s*,\s*int64_t\s+len\s*," + tail, src)
    assert re.search(r"int\s+aasm_paf_read_device\s*\(\s*const\s+char\s*\*\s*path\s*," + tail, src)
    assert re.search(r"#define\s+AASM_READ_H_WEAK_HASH\s+0x100\b", src) and _abi.AASM_READ_H_WEAK_HASH == 0x100
    assert re.search(r"#define\s+AASM_READ_H_FEW_BLOCKS\s+0x200\b", src) and _abi.AASM_READ_H_FEW_BLOCKS == 0x200
    assert re.search(r"#define\s+AASM_READ_DEVICE_RANGES\s+1\b", src) and _abi.AASM_READ_DEVICE_RANGES == 1
    assert re.search(r"#define\s+AASM_ABI_VERSION\s+3\b", src)


def test_library_exports_the_device_reader(T):
    api = T.api()
    for n in NEW_FUNCS:
        assert n in api.EXPORTED and hasattr(api.LIB, n)
    assert api.LIB.aasm_abi_version() == 3
    seven = [C.c_char_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert api.LIB.aasm_paf_parse_device.argtypes == seven and api.LIB.aasm_paf_read_device.argtypes == [C.c_char_p] + seven[2:]
    assert api.debug_counter("read_slow_rows") >= 0 and api.debug_counter("read_host_fallbacks") >= 0
    assert api.debug_counter("no_such_counter") == -1


def test_bad_arguments_and_no_device(T, tmp_path):
    api = T.api()
    h, up, view = C.c_void_p(), C.c_void_p(), _abi.BatchIn()
    text = RC.row()
    f = api.LIB.aasm_paf_parse_device
    assert f(None, 0, 0, 0, C.byref(h), C.byref(up), C.byref(view)) == _abi.AASM_E_INVAL
    assert f(text, -1, 0, 0, C.byref(h), C.byref(up), C.byref(view)) == _abi.AASM_E_INVAL
    assert f(text, len(text), 0, 0, C.byref(h), C.byref(up), None) == _abi.AASM_E_INVAL           # up without dev_view
    assert f(text, len(text), 0, 0, C.byref(h), None, C.byref(view)) == _abi.AASM_E_INVAL
    assert f(text, len(text), 0, 0, None, None, None) == _abi.AASM_E_INVAL                        # nothing asked for
    assert api.LIB.aasm_paf_read_device(None, 0, 0, C.byref(h), C.byref(up), C.byref(view)) == _abi.AASM_E_INVAL
    assert api.LIB.aasm_paf_read_device(os.fsencode(tmp_path / "none.paf"), 0, 0, C.byref(h), C.byref(up), C.byref(view)) == _abi.AASM_E_IO
    assert not h and not up
    if api.device_count() == 0:                                      # the loud failure, no fallback (guarded as tests/test_abi.py does)
        with pytest.raises(api.AlignasmError) as ei:
            api.Paf.parse_device(text)
        assert ei.value.code == _abi.AASM_E_NODEVICE
        (tmp_path / "one.paf").write_bytes(text)
        with pytest.raises(api.AlignasmError) as ei:
            api.Paf.read_device(tmp_path / "one.paf")
        assert ei.value.code == _abi.AASM_E_NODEVICE


# ---- 2. the kernel bodies in the 1-lane emulation ---------------------------------------------------------------------------
def test_case_list_is_what_the_kernels_assume(emr, cases):
    lib, _ = emr
    assert lib.emr_tile() == RC.TILE
    by = {c["name"]: c["text"] for c in cases}
    assert by["newline_last_byte_of_tile"][RC.TILE - 1:RC.TILE] == b"\n" and by["newline_first_byte_of_tile"][RC.TILE:RC.TILE + 1] == b"\n"
    assert by["crlf_split_by_tile_edge"][RC.TILE - 1:RC.TILE + 1] == b"\r\n" and by["crlf_ends_tile"][RC.TILE - 2:RC.TILE] == b"\r\n"
    assert by["row_start_on_second_edge"][2 * RC.TILE - 1:2 * RC.TILE] == b"\n"
    assert 200_000 < len(by["synth_file"]) and len(by["synth_file"]) // RC.TILE >= 12
    wide = by["contig_spans_three_tiles"]
    assert wide.rindex(b"wide\t") - wide.index(b"wide\t") > 2 * RC.TILE
    for extra in (1, 7, 8, 9, 15, 16, 17):
        assert len(by["len_tile_plus_%d" % extra]) == RC.TILE + extra == len(by["len_tile_plus_%d_open" % extra])
    edges = by["names_straddle_tile_edges"]
    assert edges[RC.TILE - 21:RC.TILE + 21] == b"\n" + b"Q" * 39 + b"q\t" and edges[2 * RC.TILE - 21:2 * RC.TILE + 21] == b"\t" + b"R" * 39 + b"r\t"
    per_tile = by["long_one_row_per_tile"]
    assert [per_tile[:20 * RC.TILE].count(b"\n", t * RC.TILE, (t + 1) * RC.TILE) for t in range(20)] == [1] * 20
    assert all(per_tile[(t + 1) * RC.TILE - 1] == 10 for t in range(20))
    big = by["long_1mib_only"]
    assert big.count(b"\n") == 1 and len(big) > 64 * RC.TILE
    for name, tiles in (("slow_rows_64", 3), ("slow_rows_65", 3), ("slow_rows_300", 2)):        # the slow rows lie in several tiles
        starts = [m.start() for m in re.finditer(rb"\t[+ ][0-9]+\t|\t1[0-9]{18}\t", by[name])]
        assert len(starts) == int(name.rsplit("_", 1)[1]) and len({s // RC.TILE for s in starts}) >= tiles


def _case_ids():
    return [c["name"] for c in RC.valid_cases(RC.fill(400))]


def check_case(T, api, case, got_paf_text, got_container, got_view):
    """A reader's container (its view's arrays and to_text()) and batch view against the host reader and, where it models the
    text, the I/O oracle."""
    _, want, want_text = X.host_read(api, case["text"])
    assert X.diff_views(want, got_container) == []
    assert got_paf_text == want_text
    if got_view is not None:
        assert X.diff_views(want, got_view) == []
    if case["oracle"]:
        X.check_against_oracle(T, case["text"], got_container, got_paf_text)


@pytest.mark.parametrize("name", _case_ids())
def test_emulated_reader_equals_oracle_and_host_reader(T, emr, cases, name):
    lib, _ = emr
    api = T.api()
    case = next(c for c in cases if c["name"] == name)
    for flags in (0, _abi.AASM_READ_H_WEAK_HASH) if case["weak"] else (0,):
        for max_blocks in (0, 3):                                    # 3: fewer blocks than tiles and rows, the grid-stride loops
            before = lib.emr_counter(1)
            rc, msg, paf, view = X.emul_parse(lib, case["text"], flags, max_blocks)
            assert rc == 0, msg
            assert lib.emr_counter(1) == before and lib.emr_counter(0) == case["slow"]
            check_case(T, api, case, paf.to_text(), X.view_arrays(paf.view()), view)


def test_emulated_reader_halves(T, emr, cases):
    """paf alone and the batch alone give what both together give."""
    lib, _ = emr
    case = next(c for c in cases if c["name"] == "slow_numbers")
    _, _, paf, view = X.emul_parse(lib, case["text"])
    rc, _, paf1, none = X.emul_parse(lib, case["text"], want_view=False)
    assert rc == 0 and none is None and paf1.to_text() == paf.to_text()
    rc, _, none, view1 = X.emul_parse(lib, case["text"], want_paf=False)
    assert rc == 0 and none is None and X.diff_views(view, view1) == []


def test_emulated_container_writes_the_host_readers_files(T, emr, cases, tmp_path):
    """row_index and cord_type (the xi tags) and the names: the writers' three files from the emulated container."""
    lib, _ = emr
    api = T.api()
    text = next(c for c in cases if c["name"] == "synth_file")["text"]
    host = api.Paf.parse(text, device_ranges=True)
    sol = _abi.BatchOut()
    ranged = api.Paf.parse(text)                                     # (match ranges for the oracle's solve)
    hv = ranged.view()
    assert T.oracle().oracle_solve_batch(C.byref(hv), C.byref(_abi.Opts(4, 0, 0, 0, 0)), 2, C.byref(sol)) == 0
    rc, msg, paf, _ = X.emul_parse(lib, text, want_view=False)
    assert rc == 0, msg
    a = [str(tmp_path / n) for n in ("a.paf", "a.alt.paf", "a.all.paf")]
    b = [str(tmp_path / n) for n in ("b.paf", "b.alt.paf", "b.all.paf")]
    host.write_outputs(sol, *a)
    paf.write_outputs(sol, *b)
    T.oracle().oracle_free_out(C.byref(sol))
    for x, y in zip(a, b):
        assert os.path.getsize(x) > 0 and open(x, "rb").read() == open(y, "rb").read()


# ---- 3. errors --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _ in RC.error_cases()])
def test_emulated_reader_reports_the_host_readers_error(T, emr, name):
    lib, _ = emr
    api = T.api()
    text = dict(RC.error_cases())[name]
    code, msg = X.host_error(api, text)
    assert code == _abi.AASM_E_PARSE
    before = lib.emr_counter(1)
    rc, got, paf, view = X.emul_parse(lib, text)
    assert (rc, got) == (code, msg) and paf is None and view is None
    assert lib.emr_counter(1) == before + 1                          # the device found the fault itself and asked the host why


def test_error_messages_name_the_first_bad_row(T):
    """What the case list claims about the host reader's messages (they are the contract)."""
    api = T.api()
    e = dict(RC.error_cases())
    assert "Missing cs:Z tag" in X.host_error(api, e["later_kind_first"])[1]
    assert "non-numeric" in X.host_error(api, e["number_before_columns"])[1]
    assert "fewer than 12 columns" in X.host_error(api, e["columns_before_number"])[1]
    assert "Unsupported operation" in X.host_error(api, e["bad_tag_before_column_fault"])[1]
    assert X.host_error(api, e["empty_text"])[1] == "empty PAF"


def test_malformed_tag_alone_is_left_to_the_solve(T, emr):
    lib, _ = emr
    api = T.api()
    text = RC.bad_tag_only()
    rc, msg, paf, view = X.emul_parse(lib, text)
    assert rc == 0, msg
    _, want, want_text = X.host_read(api, text)
    assert X.diff_views(want, view) == [] and paf.to_text() == want_text


# ---- 4. under a host address sanitizer: reads stay inside [0, len) ----------------------------------------------------------
def test_framing_cases_under_the_address_sanitizer(T, emr, cases, tmp_path):
    _, san = emr
    framing = cases[:[c["name"] for c in cases].index("synth_file")]
    framing += [c for c in cases if c["name"] in ("bare_cs", "slow_row_last_no_newline", "contig_spans_three_tiles", "refs_more_than_64")]
    framing += [c for c in cases if c["name"].startswith("long_") or c["name"] in ("names_straddle_tile_edges", "empty_query_name", "slow_rows_65")]
    assert len(framing) >= 53
    paths, want = [], []
    for c in framing:
        p = tmp_path / (c["name"] + ".paf")
        p.write_bytes(c["text"])
        paths.append(str(p))
        n = X.host_read(T.api(), c["text"])[1]["n_records"]
        want += ["%s 0 %d" % (p, n)] * 2
    bad = tmp_path / "bad.paf"
    bad.write_bytes(dict(RC.error_cases())["fault_in_last_row_no_newline"])
    r = subprocess.run([san] + paths + [str(bad)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split("\n")[:-1] == want + ["%s %d -1" % (bad, _abi.AASM_E_PARSE)] * 2
