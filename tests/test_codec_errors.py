"""PAF reader errors: which row is named and with what message, for every kind of bad row, wherever
it sits in a multi-chunk file, at every host thread count, with host or device match ranges; the
--alt reader's own messages; number spellings both readers accept alike."""
import ctypes as C

import numpy as np
import pytest

from alignasm_amd._abi import AASM_E_PARSE

THREADS = (1, 3, 16)


@pytest.fixture(scope="module")
def lines(T):
    text = T.api().Paf.synth(30, 100, 13).to_text()
    assert len(text) > (1 << 20)                       # several reader chunks
    return text.split(b"\n")[:-1]


def _cs_fault(prefix):
    def bad(f):
        f[-1] = b"cs:Z:" + prefix + f[-1][5:]
        return f
    return bad


def _num_fault(f):
    f[7] = f[7] + b"x"
    return f


# kind -> (how the row is broken, message for row n with query name q, reported in device-ranges mode too)
FAULTS = {
    "columns": (lambda f: f[:11], lambda n, q: "PAF row %d has fewer than 12 columns" % n, True),
    "number": (_num_fault, lambda n, q: "PAF row %d: non-numeric field" % n, True),
    "no_cs": (lambda f: f[:13], lambda n, q: "Missing cs:Z tag in PAF record for query '%s'" % q, True),
    "number_no_cs": (lambda f: _num_fault(f[:13]), lambda n, q: "PAF row %d: non-numeric field" % n, True),
    "cs_length": (_cs_fault(b":0"), lambda n, q: "Invalid :length operation in cs tag (row %d)" % n, False),
    "cs_subst": (_cs_fault(b"*a"), lambda n, q: "Invalid substitution operation in cs tag (row %d)" % n, False),
    "cs_indel": (_cs_fault(b"+"), lambda n, q: "Empty indel operation in cs tag (row %d)" % n, False),
    "cs_op": (_cs_fault(b"?"), lambda n, q: "Unsupported operation in short-form cs tag (row %d)" % n, False),
    "cs_consume": (_cs_fault(b":9999999"), lambda n, q: "cs tag consumption does not match PAF coordinates (row %d)" % n, False),
}


def _broken(lines, faults):
    """lines with row i replaced by FAULTS[kind] applied to it, for every (i, kind) in faults."""
    out = list(lines)
    for i, kind in faults:
        out[i] = b"\t".join(FAULTS[kind][0](lines[i].split(b"\t")))
    return b"\n".join(out) + b"\n"


def _cut_row(text, t, T):
    """First row of reader chunk t of T (chunks start at the first line start at or after len * t / T)."""
    b = len(text) * t // T
    return text.count(b"\n", 0, b - 1 + text[b - 1:].index(b"\n") + 1)


def _positions(lines, kind):
    """Rows to break: the first, one in the middle of the first chunk of 3, the first row past the cut of 3 and of 16
    chunks (found on the broken text itself, whose length moves the cuts)."""
    plain = b"\n".join(lines) + b"\n"
    rows = [0, _cut_row(plain, 1, 6)]
    for t, T in ((1, 3), (1, 16)):
        i = _cut_row(plain, t, T)
        for _ in range(4):
            j = _cut_row(_broken(lines, [(i, kind)]), t, T)
            if j == i:
                break
            i = j
        rows.append(i)
    return rows


def _parse(api, text, device_ranges):
    return api.Paf.parse(text, device_ranges=device_ranges)


def _expect_error(api, text, device_ranges, msg):
    with pytest.raises(api.AlignasmError) as e:
        _parse(api, text, device_ranges)
    assert e.value.code == AASM_E_PARSE
    assert str(e.value) == "alignasm_amd error %d: %s" % (AASM_E_PARSE, msg)


@pytest.mark.parametrize("kind", list(FAULTS))
def test_reader_reports_each_bad_row_kind_anywhere(T, lines, kind):
    api = T.api()
    old = api.set_host_threads(1)
    try:
        for row in _positions(lines, kind):
            text = _broken(lines, [(row, kind)])
            msg = FAULTS[kind][1](row, lines[row].split(b"\t")[0].decode())
            for n in THREADS:
                api.set_host_threads(n)
                _expect_error(api, text, False, msg)
                if FAULTS[kind][2]:
                    _expect_error(api, text, True, msg)
                else:                                  # the host does not read the tags: the GPU reports them
                    assert _parse(api, text, True).n_contigs == 30
    finally:
        api.set_host_threads(old)


PAIRS = [("cs_consume", "columns"), ("columns", "cs_op"), ("number", "no_cs"), ("no_cs", "number"), ("cs_subst", "cs_length"),
         ("cs_indel", "number_no_cs")]


@pytest.mark.parametrize("first,second", PAIRS)
def test_reader_reports_the_earlier_of_two_bad_rows(T, lines, first, second):
    """Two bad rows in different chunks: the one earlier in the file is named.  With device ranges a bad cs tag counts
    only when the file has another error after it: the serial reader's precedence."""
    api = T.api()
    plain = b"\n".join(lines) + b"\n"
    a, b = _cut_row(plain, 1, 6), _cut_row(plain, 2, 3) + 5
    text = _broken(lines, [(a, first), (b, second)])
    q = lambda i: lines[i].split(b"\t")[0].decode()
    old = api.set_host_threads(1)
    try:
        for n in THREADS:
            api.set_host_threads(n)
            _expect_error(api, text, False, FAULTS[first][1](a, q(a)))
            if FAULTS[second][2]:
                _expect_error(api, text, True, FAULTS[first][1](a, q(a)))
            elif FAULTS[first][2]:
                _expect_error(api, text, True, FAULTS[first][1](a, q(a)))
            else:
                assert _parse(api, text, True).n_contigs == 30
    finally:
        api.set_host_threads(old)


def test_reader_empty_inputs(T):
    api = T.api()
    for text in (b"", b"\n", b"\r\n\n\r\n"):
        for dev in (False, True):
            _expect_error(api, text, dev, "empty PAF")


def test_reader_rejects_a_line_longer_than_int32(T):
    api = T.api()
    head = T.api().Paf.synth(2, 5, 3).to_text()
    n = len(head) + (1 << 31) + 1
    buf = bytearray(b"x") * n
    buf[:len(head)] = head
    buf[-1:] = b"\n"
    h = C.c_void_p()
    rc = api.LIB.aasm_paf_parse_mem_opts((C.c_char * n).from_buffer(buf), C.c_int64(n), 0, C.byref(h))
    assert rc == AASM_E_PARSE
    assert api.LIB.aasm_last_error() == b"PAF row 10 is longer than 2147483647 bytes"


def _alt_rows(T):
    api = T.api()
    main = api.Paf.synth(3, 6, 17)
    names = [ln.split(b"\t")[0] for ln in main.to_text().split(b"\n")[:-1]]
    src = api.Paf.synth(2, 5, 4).to_text().split(b"\n")[:-1]
    rows = []
    for i, line in enumerate(src):
        f = line.split(b"\t")
        f[0] = names[0 if i < 5 else -1] + b":101-%d" % (100 + int(f[1]))
        rows.append(f)
    return main.to_text(), rows


ALT_FAULTS = {
    "columns": (lambda f: f[:11], "alt PAF row %d has fewer than 12 columns"),
    "piece_no_colon": (lambda f: [f[0].replace(b":", b"_")] + f[1:], "Invalid input string format"),
    "piece_number": (lambda f: [f[0].split(b":")[0] + b":x1-9"] + f[1:], "Error parsing number"),
    "piece_before_number": (lambda f: [f[0].replace(b":", b"_")] + _num_fault(f)[1:], "Invalid input string format"),
    "number": (_num_fault, "alt PAF row %d: non-numeric field"),
    "no_cs": (lambda f: f[:13], "Missing cs:Z tag in alternative PAF record for query '%s'"),
    "number_no_cs": (lambda f: _num_fault(f[:13]), "alt PAF row %d: non-numeric field"),
    "cs_subst": (_cs_fault(b"*a"), "Invalid substitution operation in cs tag (alt row %d)"),
    "cs_consume": (_cs_fault(b":9999999"), "cs tag consumption does not match PAF coordinates (alt row %d)"),
}


@pytest.mark.parametrize("kind", list(ALT_FAULTS))
def test_alt_reader_reports_bad_rows(T, kind):
    api = T.api()
    main_text, rows = _alt_rows(T)
    for i in (0, 6):
        bad = [list(f) for f in rows]
        bad[i] = ALT_FAULTS[kind][0](list(rows[i]))
        text = b"\n".join(b"\t".join(f) for f in bad) + b"\n"
        msg = ALT_FAULTS[kind][1]
        msg = msg % bad[i][0].decode() if "%s" in msg else msg % i if "%d" in msg else msg
        for dev in (False, True):
            paf = api.Paf.parse(main_text, device_ranges=dev)
            with pytest.raises(api.AlignasmError) as e:
                paf.merge_alt(text)
            assert e.value.code == AASM_E_PARSE
            assert str(e.value) == "alignasm_amd error %d: %s" % (AASM_E_PARSE, msg)


def _respell(f):
    """The same numbers written as strtoll also reads them: a '+' sign, leading zeros, 19 digits."""
    f = list(f)
    f[1] = b"+" + f[1]
    f[2] = b"00" + f[2]
    f[6] = f[6].rjust(19, b"0")
    f[9] = b"+0" + f[9]
    f[11] = f[11].rjust(20, b"0")
    return f


def test_number_spellings_read_alike_by_both_readers(T):
    api = T.api()
    main_text, rows = _alt_rows(T)
    main_rows = [ln.split(b"\t") for ln in main_text.split(b"\n")[:-1]]
    join = lambda rs: b"\n".join(b"\t".join(f) for f in rs) + b"\n"
    arrays = lambda p: {k: v.copy() for k, v in p.batch().arrays.items()}
    for dev in (False, True):
        want = arrays(api.Paf.parse(main_text, device_ranges=dev))
        got = arrays(api.Paf.parse(join([_respell(f) for f in main_rows]), device_ranges=dev))
        for k in want:
            assert np.array_equal(want[k], got[k]), (dev, k)
        plain, spelled = api.Paf.parse(main_text, device_ranges=dev), api.Paf.parse(main_text, device_ranges=dev)
        plain.merge_alt(join(rows))
        spelled.merge_alt(join([_respell(f) for f in rows]))
        want, got = arrays(plain), arrays(spelled)
        for k in want:
            assert np.array_equal(want[k], got[k]), (dev, k)
    # beyond int64: strtoll's saturation
    big = list(main_rows[0])
    big[1] = b"9" * 20
    assert api.Paf.parse(join([big])).batch().arrays["qry_total"][0] == (1 << 63) - 1
