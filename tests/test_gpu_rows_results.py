"""GPU tier of the device rows on results of real size: solver output of several fill chunks with irregular plans in it through
to_torch(rows=True) and aasm_writer_append_device in pieces of every kind, the 2 700-contig texts, and a list made for the piece
cutter's sampled offsets.  Expected bytes are the oracle side's (tests/text_fuzz.py, expected()) or the host writer's files."""
import os

import pytest

import rows_testlib as W
import text_fuzz as F
from alignasm_amd import _abi
from test_gpu_rows import SUFFIXES, fuzz_on_device, host_files

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("the GPU tier needs torch to see the device")
    return torch


@pytest.fixture(scope="module")
def emw():
    return W.build_emul()


def count_pieces(emw, off, limit):
    """What the piece cutter makes of these offsets, by its host build, checked against its contract (W.check_pieces)."""
    pieces, calls = W.emul_cut_pieces(emw, off, limit)
    return W.check_pieces(off, limit, pieces, calls)


def rows_and_writer(T, torch, text, K, nsl, d_path, pieces):
    """text -> solve -> to_torch(rows=True) and write_outputs_device per piece size, all equal to the oracle's files
    -> (api, result dict as numpy offsets, plans)."""
    exp = F.expected(T, text, K, nsl)
    assert exp.kind == "ok"
    api, paf, db, res = fuzz_on_device(T, torch, text, K, nsl)
    d = res.to_torch(cuts=db, rows=True)
    torch.cuda.current_stream(db.device).synchronize()
    got = [d[k + "_text"].cpu().numpy().tobytes() for k in W.LISTS]
    assert got == list(exp.files)
    off = {k: d[k + "_row_off"].cpu().numpy() for k in W.LISTS}
    W.check_offsets(off, got)
    for p in pieces(off):
        paths = [os.path.join(str(d_path), "p%d%s" % (p, s)) for s in SUFFIXES]
        paf.write_outputs_device(db, d, *paths, piece_bytes=p)
        assert [open(f, "rb").read() for f in paths] == list(exp.files), p
    plans = api.cuts_to_numpy(d)
    res.close(); db.close()
    return exp, off, plans


@pytest.mark.parametrize("first", (0, 10))
def test_joined_texts(T, torch, tmp_path, first):
    """Ten shaped texts as one file, both runs: the rows of to_torch(rows=True) and the device writer's files in default pieces,
    pieces of 4096 bytes and a piece per row are the oracle's files; main holds irregular rows in three fill chunks or more
    (counted on the device's plans, checked against the I/O oracle)."""
    text = F.joined([F.shaped_text(i) for i in range(first, first + 10)])
    for K, nsl in F.RUNS:
        exp, off, plans = rows_and_writer(T, torch, text, K, nsl, tmp_path, lambda off: (0, 4096, 1))
        irr = W.oracle_checked_irregular(T, exp, plans)
        chunks = set(i // W.CHUNK for i in irr["main"])
        assert len(plans["main"]) > 2 * W.CHUNK and len(chunks) >= 3, (len(plans["main"]), irr["main"])


def test_joined_text_the_oracle_rejects(T, torch, tmp_path):
    """Unshaped texts joined, some the oracle rejects: to_torch(rows=True) raises naming the oracle's first rejected element, the
    device writer raises with the oracle's message, and no file is left behind."""
    bad = [i for i in range(24) if F.expected(T, F.unshaped_text(i), 10000, False).kind == "err"][:3]   # (the oracle's choice)
    text = F.joined([F.unshaped_text(i) for i in [0, 1] + bad])
    exp = F.expected(T, text, 10000, False)
    assert exp.kind == "err"
    api, paf, db, res = fuzz_on_device(T, torch, text, 10000, False)
    l, j, v = next((l, j, v) for l, k in enumerate(W.LISTS) for j, v in enumerate(exp.verdict[k]) if v)
    with pytest.raises(api.AlignasmError) as e:
        res.to_torch(cuts=db, rows=True)
    assert e.value.code == _abi.AASM_E_PARSE and "list %s, element %d, flags 0x%x" % (W.LISTS[l], j, v) in str(e.value)
    for p in (0, 4096, 1):
        with pytest.raises(api.AlignasmError) as e:
            paf.write_outputs_device(db, res, *[str(tmp_path / ("d" + s)) for s in SUFFIXES], piece_bytes=p)
        assert e.value.code == _abi.AASM_E_PARSE and exp.message in str(e.value), p
        assert os.listdir(tmp_path) == []
    res.close(); db.close()


@pytest.mark.parametrize("case", [(7, 0, 10000, False), (8, 1, 3, True)], ids=["seed7_style0_k10000", "seed8_style1_k3_nsl"])
def test_many_contigs_texts(T, torch, emw, tmp_path, case):
    """The 2 700-contig texts of test_gpu_text_fuzz.py (12 064 and 7 418 main rows) through to_torch(rows=True) and the device
    writer, in default pieces and in pieces of one and a half blocks of 1024 rows: several pieces, all cut at sampled offsets.
    expected() on these texts takes 2.2 and 2.5 CPU seconds (4.7 together, beside 2.1 and 2.7 for making the texts): less than
    test_many_contigs_texts spends, which makes the same two calls and three solves and writers on top, so both texts stay."""
    seed, style, K, nsl = case
    limit = {}

    def pieces(off):
        limit["v"] = int(off["main"][W.SAMPLE]) * 3 // 2
        return (0, limit["v"])
    exp, off, plans = rows_and_writer(T, torch, F.many_contigs_text(seed, style), K, nsl, tmp_path, pieces)
    assert exp.sol["n_contigs"] == 2700 and len(off["main"]) - 1 > 7 * W.SAMPLE
    by_samples, by_rows = count_pieces(emw, off["main"], limit["v"])
    assert by_samples > 1 and by_rows == 0, (by_samples, by_rows)


def test_pieces_at_samples_and_at_rows(T, torch, emw, tmp_path):
    """2 049 single-record contigs, one main row each, row 1 500 with a tag of 300 KB: the device writer in pieces of 1 byte, of
    the first block's bytes (the `<=`), one less, one and a half blocks and the default equals the host writer byte for byte.
    With a block's bytes the first block is one piece, the second is cut by rows (the long row alone) and the last row is a
    piece: both kinds of cut in one run (counted by the cutter's host build on the result's offsets, against its contract)."""
    api = T.api()
    rows = []
    for c in range(2049):
        n = 60000 if c == 1500 else 1 + c % 7
        tag, q = "cs:Z:" + ":1*ac" * n + ":%d" % (3 + c % 50), 2 * n + 3 + c % 50
        rows.append("\t".join(["s%d" % c, str(q + 20), "5", str(5 + q), "+-"[c % 2], "chrA", "9000000", str(100 + c), str(100 + c + q), str(q - n), str(q), "60", "tp:A:P", tag]))
    text = ("\n".join(rows) + "\n").encode()
    paf = api.Paf.parse(text, device_ranges=True)
    db = api.DeviceBatch(paf)
    res = db.solve(max_paths=10000)
    want = host_files(T, paf, res, tmp_path, "walk")
    d = res.to_torch(cuts=db, rows=True)
    torch.cuda.current_stream(db.device).synchronize()
    off = d["main_row_off"].cpu().numpy()
    assert len(off) - 1 == 2049 and [d[k + "_text"].cpu().numpy().tobytes() for k in W.LISTS] == want
    block = int(off[W.SAMPLE])
    assert int(off[1501] - off[1500]) > 300000 > block
    for p in (1, block, block - 1, block * 3 // 2, 0):
        paths = [str(tmp_path / ("dev%d%s" % (p, s))) for s in SUFFIXES]
        paf.write_outputs_device(db, d, *paths, piece_bytes=p)
        assert [open(f, "rb").read() for f in paths] == want, p
    assert count_pieces(emw, off, block) == (2, 3)                   # block 0 and the last row; the rows before the long one, it, those behind
    assert count_pieces(emw, off, block - 1) == (1, 5)               # block 0 falls into rows [0, 1023) and row 1023
    res.close(); db.close()
