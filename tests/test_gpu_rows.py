"""GPU tier of the device rows: aasm_rows_sizes_device / aasm_rows_format_device (kernels aasm_rows_len, aasm_rows_fill on the MI355X),
to_torch(rows=True), aasm_writer_append_device and the command line's --device-writer.  The hand-made cases of the CPU tier run here
with all the lanes of the fill's cooperative copy (every buffer between guard bytes); expected bytes come from the oracle's files, the
host writers on the same result, or the row layout restated in tests/rows_testlib.py."""
import os
import subprocess

import numpy as np
import pytest

import cuts_testlib as X
import rows_testlib as W
import text_fuzz as F
from alignasm_amd import _abi
from test_export_cpu import CASE_IDS, CASES

pytestmark = pytest.mark.gpu
SUFFIXES = (".aln.paf", ".aln.alt.paf", ".aln.all.paf")


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("the GPU tier needs torch to see the device")
    return torch


@pytest.fixture(scope="module")
def emc():
    return X.build_emul()


def hand_cases():
    return [("alignment", W.alignment_case, 0), ("long_rows", W.long_case, 0), ("one_row", lambda: W.sized_case(1, 0, 3), 0),
            ("chunk_minus_1", lambda: W.sized_case(W.CHUNK - 1, 0, W.CHUNK), 0), ("chunk", lambda: W.sized_case(W.CHUNK, 1, W.CHUNK + 1), 0),
            ("chunk_plus_1", lambda: W.sized_case(W.CHUNK + 1, W.CHUNK - 1, 1), 0), ("two_chunks_plus_1", lambda: W.sized_case(2 * W.CHUNK + 1, 0, 2 * W.CHUNK + 1), 0),
            ("many_chunks_few_blocks", lambda: W.sized_case(9 * W.CHUNK + 5, 4 * W.CHUNK + 1, 17 * W.CHUNK + 3), _abi.AASM_ROWS_H_FEW_BLOCKS),
            ("length_chunks", lambda: W.sized_case(2 * W.LEN_CHUNK + 1, W.LEN_CHUNK, W.LEN_CHUNK + 1), 0)]


@pytest.mark.parametrize("name,make,flags", hand_cases(), ids=[c[0] for c in hand_cases()])
def test_hand_made_lists(T, torch, name, make, flags):
    """Rows at every start offset mod 16 with stretches of 0 .. 33 bytes, a 1 MiB tag and a 70 000-operation tag (uncut and cut),
    lists of 1, chunk - 1, chunk, chunk + 1, 2 chunk + 1 rows with an empty alt list, more chunks than blocks (the hook), lists
    longer than the length pass's chunk: the bytes are the restated layout's, the offsets their prefix sums."""
    case = make()
    dc = W.DeviceCase(case)
    texts = dc.texts(T.api(), flags)
    assert texts == W.joined_py(case)
    W.check_offsets(dc.offsets(), texts)


def test_all_numbering_and_digits(T, torch):
    from test_rows_cpu import I32_EDGES, I64_EDGES
    rec = {"cs": W.TAG, "fwd": True, "qs": 100, "qe": 134}
    contigs = [("first", [rec]), ("none", [rec]), ("many", [rec, dict(rec, fwd=False)]), ("none2", [rec]), ("last", [rec])]
    per = [{"all": [[(100, 134, 7, 41, 0)], [], [(100, 134, 7, 41, 0)] * 2]}, {}, {"all": [[(100, 134, 7, 41, p % 2)] * (1 + p % 3) for p in range(101)]}, {},
           {"all": [[], [(100, 134, 7, 41, 0)]]}]
    n64 = len(I64_EDGES)
    for i in range(n64):
        v = lambda k: I64_EDGES[(i + k) % n64]   # noqa: E731
        contigs.append(("d%d" % i, [{"cs": W.TAG, "fwd": i % 2 == 0, "qs": v(1), "qe": v(2), "qtot": v(0), "rtot": v(3), "mat": I32_EDGES[i % 9], "aln": I32_EDGES[(i + 1) % 9],
                                     "mq": (0, 9, 10, 99, 100, 255)[i % 6], "row_index": (0, 2 ** 31 - 1)[i % 2], "cord": (i // 2) % 2}]))
        per.append({"main": [(v(1), v(2), v(4), v(5), 0)]})
    case = W.hand_case(contigs, ["chrA"], per)
    assert W.DeviceCase(case).texts(T.api()) == W.joined_py(case)


def test_ranges(T, torch):
    """Every split point of a 40-row list: the two ranges concatenate to the whole and touch no byte outside their own; bad
    ranges, a bad list and an info that is not the sizes call's are refused."""
    api, case = T.api(), W.sized_case(40, 40, 40)
    dc = W.DeviceCase(case)
    texts = dc.texts(api)
    assert texts == W.joined_py(case)
    for e in range(41):
        a, b = dc.format(api, 2, 0, e), dc.format(api, 2, e, 40)
        assert a[0] == 0 and b[0] == 0 and a[1] + b[1] == texts[2], e
    assert dc.format(api, 0, 17, 17) == (0, b"")
    for lst, e0, e1 in ((0, 3, 2), (1, 0, 41), (2, -1, 4), (3, 0, 1)):
        assert dc.format(api, lst, e0, e1)[0] == _abi.AASM_E_INVAL
    dc.info.bytes[1] += 1
    assert dc.format(api, 1, 0, 40)[0] == _abi.AASM_E_INVAL
    dc.info.bytes[1] -= 1
    host = np.zeros(1 << 16, np.uint8)                                # host memory for the text
    assert api.rows_format_raw(dc.view, dc.cols, dc.sz, dc.dev_out, dc.cuts, dc.ro, dc.info, 0, 0, 40, host.ctypes.data, 0, 0, 0) == _abi.AASM_E_INVAL
    ro = _abi.DevRows(dc.ro.main_off + 4, dc.ro.alt_off, dc.ro.all_off)   # a misaligned offsets array
    assert api.rows_sizes_raw(dc.view, dc.cols, dc.sz, dc.dev_out, dc.cuts, ro, _abi.RowsInfo(), 0, 0, 0) == _abi.AASM_E_INVAL


def test_offsets_above_2_31(T, torch):
    import read_cases as RC
    big = "cs:Z:" + RC.long_tag(1 << 20).decode()
    case = W.hand_case([("huge", [{"cs": big, "fwd": True, "qs": 0, "qe": 10 ** 7}])], ["chrL"], [{"main": [(0, 10 ** 7, 1, 2, 0)] * 2100}])
    dc = W.DeviceCase(case)
    row = W.py_row("huge", 1000, 0, 10 ** 7, True, "chrL", 5000, 1, 2, 7, 9, 60, False, 0, 0, big)
    assert dc.sizes(T.api()) == 0 and dc.info.n_flagged == 0 and dc.info.bytes[0] == 2100 * len(row) > 2 ** 31
    assert np.array_equal(dc.offsets()["main"], np.arange(2101, dtype=np.int64) * len(row))
    assert dc.format(T.api(), 0, 2098, 2100) == (0, row + row)


def test_faults_are_flagged_and_never_formatted(T, torch):
    """A record fault, a plan of the wrong kind and a stretch outside the tag at chunk edges of all three lists: counted, the
    first in file order named, length 0, and the format call refuses."""
    api, n = T.api(), W.LEN_CHUNK + W.CHUNK + 1
    case = W.sized_case(n, n, n)
    case.out["all"]["ctg_index"][n - 1] = 3                           # the last element of .all: record count
    case.out["alt"]["ctg_index"][W.CHUNK] = -1
    cut = np.flatnonzero((case.plans["main"]["flags"] & 1) != 0)
    i = int(cut[np.abs(cut - (W.LEN_CHUNK - 1)).argmin()])
    case.plans["main"]["keep_hi"][i] = len(W.TAG) + 1
    j = int(cut[0])
    case.plans["alt"][j + 3 * W.CHUNK] = np.zeros(1, _abi.CUT_DT)[0] if (j + 3 * W.CHUNK) % 3 == 2 else case.plans["alt"][j + 3 * W.CHUNK]
    dc = W.DeviceCase(case)
    assert dc.sizes(api) == 0
    flagged = 3 + (1 if (j + 3 * W.CHUNK) % 3 == 2 else 0)
    assert (dc.info.n_flagged, dc.info.bad_list, dc.info.bad_elem, dc.info.bad_flags) == (flagged, 0, i, _abi.AASM_ROWS_E_STRETCH)
    off = dc.offsets()
    assert off["main"][i + 1] == off["main"][i] and off["alt"][W.CHUNK + 1] == off["alt"][W.CHUNK] and off["all"][n] == off["all"][n - 1]
    for l in range(3):
        assert dc.format(api, l, 0, n)[0] == _abi.AASM_E_INVAL


def fuzz_on_device(T, torch, text, K, nsl, rows=True):
    api = T.api()
    paf = api.Paf.parse(text, device_ranges=True)
    db = api.DeviceBatch(paf)
    res = db.solve(max_paths=K, non_skip_linkable=nsl)
    return api, paf, db, res


def test_text_fuzz_to_torch_rows(T, torch):
    """Shaped texts 0 - 7 (irregular plans among them) and the unshaped texts 0 - 7 through solve -> export -> plans -> rows on the
    device: the oracle's files, or AlignasmError(AASM_E_PARSE) naming the oracle's first rejected element."""
    n = {"ok": 0, "err": 0, "irregular": 0}
    for kind, text_of in (("shaped", F.shaped_text), ("unshaped", F.unshaped_text)):
        for i in range(8):
            K, nsl = F.RUNS[i % 2]
            exp = F.expected(T, text_of(i), K, nsl)
            api, paf, db, res = fuzz_on_device(T, torch, text_of(i), K, nsl)
            n[exp.kind] += 1
            if exp.kind == "ok":
                d = res.to_torch(cuts=db, rows=True)
                torch.cuda.current_stream(db.device).synchronize()
                got = [d[k + "_text"].cpu().numpy().tobytes() for k in W.LISTS]
                assert got == list(exp.files), (kind, i)
                W.check_offsets({k: d[k + "_row_off"].cpu().numpy() for k in W.LISTS}, got)
                n["irregular"] += sum(int(((p["flags"] & _abi.AASM_CUT_IRREGULAR) != 0).sum()) for p in api.cuts_to_numpy(d).values())
            else:
                l, j, v = next((l, j, v) for l, k in enumerate(W.LISTS) for j, v in enumerate(exp.verdict[k]) if v)
                with pytest.raises(api.AlignasmError) as e:
                    res.to_torch(cuts=db, rows=True)
                assert e.value.code == _abi.AASM_E_PARSE and "list %s, element %d, flags 0x%x" % (W.LISTS[l], j, v) in str(e.value), (kind, i)
            res.close(); db.close()
    assert n["ok"] >= 8 and n["err"] >= 2 and n["irregular"] >= 1, n


def irregular_cases():
    from test_rows_cpu import irregular_cases as cpu
    return [c + (0,) for c in cpu()] + [("nine_chunks_few_blocks", cpu()[-1][1], _abi.AASM_ROWS_H_FEW_BLOCKS)]


@pytest.mark.parametrize("name,make,flags", irregular_cases(), ids=[c[0] for c in irregular_cases()])
def test_irregular_hand_cases(T, torch, emc, name, make, flags):
    """The CPU tier's hand-made irregular rows with all the lanes of the fill: every chunk of a list irregular (tags rendered in
    place at every offset and length mod 8, runs of 1 .. 19 digits), irregular rows at chunk, list and path edges beside uncut and
    regular ones with a chunk that holds none, 70 000-unit and 1 MiB irregular tags beside short rows, 9 irregular chunks on the
    full grid and on 3 blocks.  The plans are the emulated cut-plan kernel's, checked against the oracle and uploaded; the rows
    are the I/O oracle's."""
    from test_rows_cpu import check_irregular_inputs
    case = W.consistent_plans(emc, make())
    check_irregular_inputs(name.replace("_few_blocks", ""), case)
    dc = W.DeviceCase(case)
    texts = dc.texts(T.api(), flags)
    assert texts == W.joined_py(case)
    W.check_offsets(dc.offsets(), texts)


def test_irregular_ranges(T, torch, emc):
    """40-row lists with every third row irregular, the first and the last among them: every split point gives the whole, every
    irregular row formatted alone is that row, and no range touches a byte outside its own (the 64 guard bytes)."""
    from test_rows_cpu import ranges_case
    api, case = T.api(), W.consistent_plans(emc, ranges_case())
    dc = W.DeviceCase(case)
    texts = dc.texts(api)
    assert texts == W.joined_py(case)
    rows = case.py_rows()
    assert case.irregular["main"][0] and case.irregular["main"][39]
    for l, k in enumerate(W.LISTS):
        for e in range(41):
            a, b = dc.format(api, l, 0, e), dc.format(api, l, e, 40)
            assert a[0] == 0 and b[0] == 0 and a[1] + b[1] == texts[l], (l, e)
        for i in np.flatnonzero(case.irregular[k]):
            assert dc.format(api, l, int(i), int(i) + 1) == (0, rows[k][int(i)]), (k, i)


REFUSAL = b"aasm_rows_format_device: info is not what aasm_rows_sizes_device returned for these row_off arrays"


def test_the_64_most_recent_sizes_calls(T, torch):
    """The library remembers the 64 most recent sizes calls of a device (include/alignasm_amd.h): after 65 calls on distinct
    row_off arrays the first info is refused, the other 64 format; sizing the first again makes it valid; a sizes call on the same
    arrays with another result replaces the earlier one, whose info is refused from then on."""
    api = T.api()
    case = W.sized_case(1, 0, 0)
    row = W.joined_py(case)[0]
    dcs = [W.DeviceCase(case) for _ in range(65)]
    for dc in dcs:
        assert dc.sizes(api) == 0 and dc.info.n_flagged == 0 and dc.info.bytes[0] == len(row)
    assert dcs[0].format(api, 0, 0, 1)[0] == _abi.AASM_E_INVAL and api.LIB.aasm_last_error() == REFUSAL
    for dc in dcs[1:]:
        assert dc.format(api, 0, 0, 1) == (0, row)
    assert dcs[0].sizes(api) == 0 and dcs[0].format(api, 0, 0, 1) == (0, row)
    # the same arrays sized with another result (a row of another length)
    other = W.hand_case([("another_name", [{"cs": W.TAG, "fwd": True, "qs": 100, "qe": 134}])], ["chrA"], [{"main": [(100, 134, 7, 41, 0)]}])
    row2 = W.joined_py(other)[0]
    assert len(row2) != len(row)
    dc2 = W.DeviceCase(other)
    dc2.off, dc2.ro = dcs[0].off, dcs[0].ro
    assert dc2.sizes(api) == 0 and dc2.info.bytes[0] == len(row2)
    assert dcs[0].format(api, 0, 0, 1)[0] == _abi.AASM_E_INVAL and api.LIB.aasm_last_error() == REFUSAL
    assert dc2.format(api, 0, 0, 1) == (0, row2)


def test_a_non_default_stream(T, torch, emc):
    """Sizes and format on a torch.cuda.Stream(): the buffer's 0xEE fill is enqueued on that stream right before the format call
    with no synchronize in between, so a kernel that ran on another stream shows as wrong bytes.  The same stream through
    to_torch(stream=..., rows=True)."""
    api, st = T.api(), torch.cuda.Stream()
    case = W.consistent_plans(emc, W.irregular_mixed_case())
    want = W.joined_py(case)
    dc = W.DeviceCase(case)
    torch.cuda.synchronize()                                         # (the uploads ran on the default stream)
    assert dc.sizes(api, stream=st.cuda_stream) == 0 and dc.info.n_flagged == 0
    for l, k in enumerate(W.LISTS):
        assert dc.format(api, l, 0, case.n[k], on=st) == (0, want[l])
        assert dc.format(api, l, W.CHUNK - 1, 2 * W.CHUNK, on=st) == (0, b"".join(case.py_rows({k: range(W.CHUNK - 1, 2 * W.CHUNK)})[k].values()))
    text = F.joined([F.shaped_text(i) for i in range(3)])
    exp = F.expected(T, text, *F.RUNS[0])
    assert exp.kind == "ok"
    api, paf, db, res = fuzz_on_device(T, torch, text, *F.RUNS[0])
    d = res.to_torch(stream=st, cuts=db, rows=True)
    with torch.cuda.stream(st):
        got = [d[k + "_text"].cpu().numpy().tobytes() for k in W.LISTS]
    assert got == list(exp.files)
    res.close(); db.close()


def host_files(T, paf, res, d, stem, cuts=None):
    bo = res.fetch_raw()
    try:
        return X.write_three(paf, bo, d, stem, cuts=cuts)
    finally:
        T.api().free_out(bo)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_device_writer_equals_the_host_writer(T, torch, case, tmp_path):
    """Solver output of the export cases: aasm_writer_append_device writes the walking writer's bytes, in default pieces and in
    pieces of a few rows (a piece per row where a row is longer)."""
    api = T.api()
    nc, nr, seed, K, dense, dup, shuf, heavy, nsl = case
    paf = api.Paf.synth(nc, nr, seed, dense=dense, heavy_tail=heavy, dup_every=dup, shuffle=shuf)
    db = api.DeviceBatch(paf, cs_only=True)
    res = db.solve(max_paths=K, non_skip_linkable=nsl)
    want = host_files(T, paf, res, tmp_path, "walk")
    for piece in (0, 1500):
        paths = [str(tmp_path / ("dev%d%s" % (piece, s))) for s in SUFFIXES]
        paf.write_outputs_device(db, res, *paths, piece_bytes=piece)
        assert [open(p, "rb").read() for p in paths] == want, piece
    assert len(want[0]) > 0
    res.close(); db.close()


def test_device_writer_after_alt_merge(T, torch, tmp_path):
    """The -a case: the merged container's A_ rows and row_index."""
    api = T.api()
    g = os.path.join(T.GOLDEN, "files")
    paf = api.Paf.parse(open(os.path.join(g, "tiny.paf"), "rb").read(), device_ranges=True)
    paf.merge_alt(open(os.path.join(g, "tiny_alt.paf"), "rb").read(), 0.5)
    db = api.DeviceBatch(paf)
    res = db.solve(max_paths=10000)
    paths = [str(tmp_path / ("d" + s)) for s in SUFFIXES]
    paf.write_outputs_device(db, res, *paths)
    got = [open(p, "rb").read() for p in paths]
    assert got == [open(os.path.join(g, "alt", "tiny" + s), "rb").read() for s in SUFFIXES] and b"xi:Z:A_" in got[0] + got[1] + got[2]
    res.close(); db.close()


def test_device_writer_rejects_as_the_planned_writer_does(T, torch, tmp_path):
    """A run the oracle rejects: nothing is written, and code and message are those of aasm_writer_append_cuts on the same inputs."""
    n = 0
    for i in range(8):
        K, nsl = F.RUNS[i % 2]
        exp = F.expected(T, F.unshaped_text(i), K, nsl)
        if exp.kind != "err":
            continue
        api, paf, db, res = fuzz_on_device(T, torch, F.unshaped_text(i), K, nsl)
        d = res.to_torch(cuts=db)
        with pytest.raises(api.AlignasmError) as want:
            host_files(T, paf, res, tmp_path, "plan", cuts=api.cuts_to_numpy(d))
        with pytest.raises(api.AlignasmError) as got:
            paf.write_outputs_device(db, d, *[str(tmp_path / ("d" + s)) for s in SUFFIXES])
        assert (got.value.code, str(got.value)) == (want.value.code, str(want.value)) and exp.message in str(got.value)
        assert os.listdir(tmp_path) == []
        res.close(); db.close()
        n += 1
    assert n >= 2


def test_row_cols_needs_a_container(T, torch):
    api = T.api()
    db = api.DeviceBatch(T.synth(3, 20, 5))
    with pytest.raises(api.AlignasmError) as e:
        db.row_cols()
    assert e.value.code == _abi.AASM_E_INVAL
    db.close()


@pytest.mark.parametrize("flags", (["--device-writer"], ["--device-writer", "--device-reader"]), ids=("writer", "reader_writer"))
def test_cli_device_writer_files_match_golden(T, torch, tmp_path, flags):
    g = os.path.join(T.GOLDEN, "files")
    exe = os.path.join(T.ROOT, "alignasm_amd", "alignasm")
    for sub, inp, extra in (("", "tiny.paf", []), ("dense", "dense.paf", []), ("alt", "tiny.paf", ["-a", "tiny_alt.paf"])):
        for name in (inp, "tiny_alt.paf"):
            (tmp_path / name).write_bytes(open(os.path.join(g, name), "rb").read())
        extra = [str(tmp_path / f) if f.endswith(".paf") else f for f in extra]
        r = subprocess.run([exe, str(tmp_path / inp)] + extra + flags + ["--timing"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert "Write output PAF file" in r.stdout and "alignasm timing:" in r.stderr
        for s in SUFFIXES:
            assert (tmp_path / (inp[:-4] + s)).read_bytes() == open(os.path.join(g, sub, inp[:-4] + s), "rb").read(), (sub, s)
            (tmp_path / (inp[:-4] + s)).unlink()


def test_cli_device_writer_rejected_file_is_reported_as_without_the_flag(T, torch, tmp_path):
    text = next(F.unshaped_text(i) for i in range(8) if F.expected(T, F.unshaped_text(i), 10000, False).kind == "err")
    (tmp_path / "bad.paf").write_bytes(text)
    exe = os.path.join(T.ROOT, "alignasm_amd", "alignasm")
    runs = [subprocess.run([exe, str(tmp_path / "bad.paf")] + f, capture_output=True, text=True) for f in ([], ["--device-writer"])]
    assert runs[0].returncode == runs[1].returncode != 0 and runs[0].stderr == runs[1].stderr
    assert sorted(os.listdir(tmp_path)) == ["bad.paf"]
