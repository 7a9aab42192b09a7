"""CPU tier of the device rows (alignasm_amd/csrc/aasm_rows.h) on the 1-lane emulation (tests/host_emul/rows_emul.cpp): row lengths,
offsets, digits, the irregular walk, ranges and the error contract.  One lane cannot see a fault between the lanes of the fill's
cooperative copy; tests/test_gpu_rows.py runs the same cases on the card.  Expected bytes come from the oracle's files, the
committed golden files, or the row layout restated in tests/rows_testlib.py - never from the code under test."""
import ctypes as C
import os

import numpy as np
import pytest

import cuts_testlib as X
import rows_testlib as W
import text_fuzz as F
from alignasm_amd import _abi
from alignasm_amd._abi import AASM_CUT_IS_CUT, CUT_DT

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def emw():
    return W.build_emul(san=True)


@pytest.fixture(scope="module")
def emc():
    return X.build_emul()


def _variants():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(G, "make_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.FILE_VARIANTS


def golden_case(T, emw, emc, variant):
    """A golden file variant as a case: oracle solve on the host container, emulated plans on the cs-form container -> (case, files)."""
    sub, inp, alt, _flags, K, nsl, base = variant
    api = T.api()
    text = open(os.path.join(G, "files", inp), "rb").read()
    alt_text = open(os.path.join(G, "files", alt), "rb").read() if alt else None
    want = [open(os.path.join(G, "files", sub, inp[:-4] + s), "rb").read() for s in (".aln.paf", ".aln.alt.paf", ".aln.all.paf")]
    host, dev = api.Paf.parse(text), api.Paf.parse(text, device_ranges=True)
    if alt_text:
        host.merge_alt(alt_text, base); dev.merge_alt(alt_text, base)
    view, out = host.view(), _abi.BatchOut()
    assert T.oracle().oracle_solve_batch(C.byref(view), C.byref(_abi.Opts(K, 1 if nsl else 0, 0, 0, 0)), 1, C.byref(out)) == 0
    sol = _abi.unpack_out(out)
    T.oracle().oracle_free_out(C.byref(out))
    return W.paf_case(emw[0], dev, sol, X.emul_plans(emc, dev.view(), sol)), want


@pytest.mark.parametrize("variant", _variants(), ids=lambda v: v[0] or "default")
def test_golden_files(T, emw, emc, variant):
    """tiny, dense (default K, K = 4, non_skip_linkable) and the two -a cases (A_ rows, merged row_index): oracle solve -> emulated
    plans -> emulated rows equal the committed files byte for byte, all three lists."""
    case, want = golden_case(T, emw, emc, variant)
    info, off, texts = W.emul_texts(emw[0], case)
    assert texts == want
    W.check_offsets(off, texts)
    if variant[2]:
        assert b"xi:Z:A_" in texts[0] + texts[1] + texts[2]


def fuzz_case(T, emw, emc, text, K, nsl):
    exp = F.expected(T, text, K, nsl)
    dev = T.api().Paf.parse(text, device_ranges=True)
    return exp, W.paf_case(emw[0], dev, exp.sol, X.emul_plans(emc, dev.view(), exp.sol))


def test_text_fuzz_accepted(T, emw, emc):
    """Shaped texts 0 - 29, both runs of each: the three files equal the oracle's, irregular plans included."""
    irregular = 0
    for i in range(30):
        for K, nsl in F.RUNS:
            exp, case = fuzz_case(T, emw, emc, F.shaped_text(i), K, nsl)
            assert exp.kind == "ok"
            info, off, texts = W.emul_texts(emw[0], case, max_blocks=(3 if i % 5 == 0 else 0))
            assert texts == list(exp.files), (i, K)
            W.check_offsets(off, texts)
            irregular += sum(int(((case.plans[k]["flags"] & _abi.AASM_CUT_IRREGULAR) != 0).sum()) for k in W.LISTS)
    assert irregular >= 1, "no irregular row was rendered"


def test_text_fuzz_rejected(T, emw, emc):
    """Unshaped texts 0 - 23: a run the oracle rejects has flagged elements, the first of them the first non-zero entry of the
    oracle's verdict in file order, and the format call refuses; a run it accepts equals its files.  At least a quarter of the
    runs are of either kind (counted on the oracle alone)."""
    n = {"ok": 0, "err": 0}
    for i in range(24):
        for K, nsl in F.RUNS:
            exp, case = fuzz_case(T, emw, emc, F.unshaped_text(i), K, nsl)
            n[exp.kind] += 1
            if exp.kind == "ok":
                assert W.emul_texts(emw[0], case)[2] == list(exp.files), (i, K)
                continue
            rc, info, off = W.emul_sizes(emw[0], case)
            first = next((l, j, v) for l, k in enumerate(W.LISTS) for j, v in enumerate(exp.verdict[k]) if v)
            assert rc == 0 and info.n_flagged == sum(1 for k in W.LISTS for v in exp.verdict[k] if v) > 0
            assert (info.bad_list, info.bad_elem, info.bad_flags) == first, (i, K)
            for l, k in enumerate(W.LISTS):
                assert W.emul_format(emw[0], case, info, off, l, 0, case.n[k])[0] == _abi.AASM_E_INVAL
    assert n["ok"] >= 12 and n["err"] >= 12, n


I64_EDGES = [0] + [v for k in range(1, 19) for v in (10 ** k - 1, 10 ** k)] + [1 << 40, -1, -10, -(1 << 40)]
I32_EDGES = [0, 1, -1, 999999999, -999999999, 1000000000, -1000000000, 2 ** 31 - 1, -2 ** 31]


def test_digit_edges(emw):
    """Every printed int64 field through 0, 9, 10, ... 10^18, 2^40 and negatives; the int32 fields through their edges from the
    record (uncut) and from the plan (cut); map_qul, row_index, both strands, both tp and both xi kinds."""
    contigs, per, plans = [], [], []
    mqs, n64, n32 = (0, 9, 10, 99, 100, 255), len(I64_EDGES), len(I32_EDGES)
    for i in range(n64):
        v = lambda k: I64_EDGES[(i + k) % n64]   # noqa: E731
        w = lambda k: I32_EDGES[(i + k) % n32]   # noqa: E731
        qe = v(2) if v(2) != v(1) else v(2) + 5                     # (qe + 1 is printed: 10^k - 1 prints 10^k)
        rec = {"cs": W.TAG, "fwd": i % 2 == 0, "qs": v(1), "qe": qe, "qtot": v(0), "rtot": v(3), "chr": i % 2, "mat": w(0), "aln": w(1), "mq": mqs[i % 6],
               "row_index": (0, 2 ** 31 - 1)[i % 2], "cord": (i // 2) % 2}
        contigs.append(("d%d" % i, [rec]))
        # main: the uncut element (the record's own mat / aln); alt: a cut one with the plan's counts, head and tail
        per.append({"main": [(v(1), qe, v(4), v(5), 0)], "alt": [(v(1) + 1, qe, v(5), v(4), 0)]})
        plans.append(W.cut_plan(7, 15, abs(v(6)), abs(v(7)), w(2), w(3)))
    case = W.hand_case(contigs, ["chrA", "b"], per, {"main": np.zeros(n64, CUT_DT), "alt": np.array(plans, CUT_DT), "all": np.zeros(0, CUT_DT)})
    info, off, texts = W.emul_texts(emw[0], case)
    assert texts == W.joined_py(case)
    W.check_offsets(off, texts)
    both = texts[0] + texts[1]
    for needle in (b"\t+\t", b"\t-\t", b"tp:A:P", b"tp:A:S", b"xi:Z:P_0\t", b"xi:Z:A_2147483647\t", b"\t-2147483648\t", b"\t1000000000000000000\t", b"\t-1099511627776\t", b"\t255\t"):
        assert needle in both, needle


def test_all_numbering(emw):
    """.all names: a contig with 101 paths (.1 .9 .10 .99 .100 .101), contigs without paths between contigs with paths, an empty path."""
    rec = {"cs": W.TAG, "fwd": True, "qs": 100, "qe": 134}
    contigs = [("first", [rec]), ("none", [rec]), ("many", [rec, dict(rec, fwd=False)]), ("none2", [rec]), ("last", [rec])]
    el = (100, 134, 7, 41, 0)
    per = [{"all": [[el], [], [el, el]]}, {}, {"all": [[(100, 134, 7, 41, p % 2)] * (1 + p % 3) for p in range(101)]}, {}, {"all": [[], [el]]}]
    case = W.hand_case(contigs, ["chrA"], per)
    info, off, texts = W.emul_texts(emw[0], case)
    assert texts == W.joined_py(case)
    for suffix in (1, 9, 10, 99, 100, 101):
        assert b"many.%d\t" % suffix in texts[2]
    assert b"first.3\t" in texts[2] and b"first.2\t" not in texts[2] and b"last.2\t" in texts[2] and b"last.1\t" not in texts[2]


def test_alignment(emw):
    case = W.alignment_case()
    info, off, texts = W.emul_texts(emw[0], case)
    assert texts == W.joined_py(case)
    assert set(int(o) % 16 for o in off["main"][:-1]) == set(range(16))


def test_long_rows(emw):
    case = W.long_case()
    info, off, texts = W.emul_texts(emw[0], case)
    assert texts == W.joined_py(case)
    assert info.bytes[0] > (1 << 20) + (1 << 19)


@pytest.mark.parametrize("n", (1, W.CHUNK - 1, W.CHUNK, W.CHUNK + 1, 2 * W.CHUNK + 1))
def test_list_sizes(emw, n):
    """Lists of 1, chunk - 1, chunk, chunk + 1 and 2 chunk + 1 rows, an empty alt list, contigs without elements at chunk edges;
    the largest also with every grid capped at 3 blocks and with all three lists long."""
    case = W.sized_case(n, 0, (n + 7) % (2 * W.CHUNK + 2))
    want = W.joined_py(case)
    assert W.emul_texts(emw[0], case)[2] == want and want[1] == b""
    if n == 2 * W.CHUNK + 1:
        big = W.sized_case(4 * W.CHUNK + 5, 3 * W.CHUNK + 1, 5 * W.CHUNK + 3)
        assert W.emul_texts(emw[0], big, max_blocks=3)[2] == W.joined_py(big)


def test_ranges(emw):
    """A 40-row list at every split point: format[0, e) + format[e, n) is the whole; the empty range writes nothing."""
    case = W.sized_case(40, 40, 40)
    info, off, texts = W.emul_texts(emw[0], case)
    assert texts == W.joined_py(case)
    for l in range(3):
        for e in range(41):
            a, b = W.emul_format(emw[0], case, info, off, l, 0, e), W.emul_format(emw[0], case, info, off, l, e, 40)
            assert a[0] == 0 and b[0] == 0 and a[1] + b[1] == texts[l], (l, e)
        assert W.emul_format(emw[0], case, info, off, l, 17, 17) == (0, b"")
        for e0, e1 in ((3, 2), (0, 41), (-1, 4)):
            assert W.emul_format(emw[0], case, info, off, l, e0, e1)[0] == _abi.AASM_E_INVAL
    assert W.emul_format(emw[0], case, info, off, 3, 0, 1)[0] == _abi.AASM_E_INVAL
    other = _abi.RowsInfo.from_buffer_copy(info)
    other.bytes[0] += 1                                              # not what the sizes call returned
    assert W.emul_format(emw[0], case, other, off, 0, 0, 40)[0] == _abi.AASM_E_INVAL


def test_offsets_above_2_31(emw):
    """2 100 uncut elements that all name the one 1 MiB-tag record: bytes[0] > 2^31 and row_off are the prefix sums, without the
    memory - only the last two rows are formatted, into a buffer of their 2 MiB."""
    import read_cases as RC
    big = "cs:Z:" + RC.long_tag(1 << 20).decode()
    case = W.hand_case([("huge", [{"cs": big, "fwd": True, "qs": 0, "qe": 10 ** 7}])], ["chrL"], [{"main": [(0, 10 ** 7, 1, 2, 0)] * 2100}])
    rc, info, off = W.emul_sizes(emw[0], case)
    row = W.py_row("huge", 1000, 0, 10 ** 7, True, "chrL", 5000, 1, 2, 7, 9, 60, False, 0, 0, big)
    assert rc == 0 and info.n_flagged == 0 and info.bytes[0] == 2100 * len(row) > 2 ** 31
    assert np.array_equal(off["main"], np.arange(2101, dtype=np.int64) * len(row))
    assert 2 * len(row) < (2 << 20) + 512                            # (the buffer: two rows, 2 MiB and the rows' few columns)
    assert W.emul_format(emw[0], case, info, off, 0, 2098, 2100) == (0, row + row)


def fault_cases():
    """(name, flags, mutate(case, list, i)): record and plan faults an element can carry."""
    def plan(**f):
        def m(case, k, i):
            for name, v in f.items():
                case.plans[k][name][i] = v
        return m

    def ctg_index(v):
        def m(case, k, i):
            case.out[k]["ctg_index"][i] = v
        return m
    return [("ctg_index_neg", 0x80, ctg_index(-1)), ("ctg_index_count", 0x80, ctg_index(3)),
            ("cut_on_uncut", 0x100, "uncut_says_cut"), ("uncut_on_cut", 0x100, "cut_says_uncut"),
            ("keep_hi_beyond", 0x200, plan(keep_hi=len(W.TAG) + 1)), ("keep_lo_4", 0x200, plan(keep_lo=4)), ("negative_head", 0x200, plan(head_keep=-1)),
            ("plan_edit_error", 0x40, plan(flags=AASM_CUT_IS_CUT | 0x40))]


@pytest.mark.parametrize("name,flag,mutate", fault_cases(), ids=[f[0] for f in fault_cases()])
def test_record_and_plan_faults(emw, name, flag, mutate):
    """Each fault as the first and as the last element of a chunk (of the fill's and of the length pass's): flagged, named as the
    first one in file order, its neighbours' lengths untouched, and never formatted."""
    n = W.LEN_CHUNK + W.CHUNK + 1
    good = W.sized_case(n, n, n)
    rc, info0, off0 = W.emul_sizes(emw[0], good)
    assert rc == 0 and info0.n_flagged == 0
    len0 = {k: np.diff(off0[k]) for k in W.LISTS}
    for where in (0, W.CHUNK - 1, W.CHUNK, W.LEN_CHUNK - 1, W.LEN_CHUNK, n - 1):
        for l, k in enumerate(W.LISTS):
            case = W.sized_case(n, n, n)
            cut = (case.plans[k]["flags"] & AASM_CUT_IS_CUT) != 0
            i = where
            if mutate == "uncut_says_cut":
                i = where if not cut[where] else (where + 1 if where + 1 < n else where - 1)
                case.plans[k]["flags"][i] = AASM_CUT_IS_CUT
            elif mutate == "cut_says_uncut":
                i = int(np.flatnonzero(cut)[np.abs(np.flatnonzero(cut) - where).argmin()])
                case.plans[k][i] = np.zeros(1, CUT_DT)[0]
            elif flag in (0x200, 0x40):                             # (a stretch fault needs a cut, regular plan)
                i = int(np.flatnonzero(cut)[np.abs(np.flatnonzero(cut) - where).argmin()])
                mutate(case, k, i)
            else:
                mutate(case, k, i)
            rc, info, off = W.emul_sizes(emw[0], case)
            assert rc == 0 and info.n_flagged == 1 and (info.bad_list, info.bad_elem, info.bad_flags) == (l, i, flag), (name, k, where, info.bad_list, info.bad_elem, hex(info.bad_flags))
            want = {kk: len0[kk].copy() for kk in W.LISTS}
            want[k][i] = 0
            assert all(np.array_equal(np.diff(off[kk]), want[kk]) for kk in W.LISTS)
            assert W.emul_format(emw[0], case, info, off, l, 0, n)[0] == _abi.AASM_E_INVAL
            clean = _abi.RowsInfo.from_buffer_copy(info)             # a caller that hides the count: the chunk with the fault is not written
            clean.n_flagged = 0
            rc, t = W.emul_format(emw[0], case, clean, off, l, 0, n)
            lo, hi = int(off[k][i - i % W.CHUNK]), int(off[k][min(n, i - i % W.CHUNK + W.CHUNK)])
            assert rc == 0 and t[lo:hi] == b"\xee" * (hi - lo)


# ---- irregular rows placed by hand (tests/rows_testlib.py: consistent cases; expected bytes are the I/O oracle's) --------------------
def irregular_cases():
    return [("alignment", W.irregular_alignment_case), ("mixed", W.irregular_mixed_case), ("long", W.long_irregular_case),
            ("nine_chunks", lambda: W.irregular_alignment_case(9 * W.CHUNK))]


@pytest.mark.parametrize("name,make", irregular_cases(), ids=[c[0] for c in irregular_cases()])
def test_irregular_hand_cases(emw, emc, name, make):
    """Irregular rows in every chunk of a list, at chunk, list and path edges beside uncut and regular rows, long ones beside short
    ones, 9 chunks on 3 blocks: the emulated cut-plan kernel's plans agree with the oracle and the builder (flags, counts), and the
    rows are the oracle's, at the full grid and at 3 blocks."""
    case = W.consistent_plans(emc, make())
    want = W.joined_py(case)
    for mb in (0, 3):
        info, off, texts = W.emul_texts(emw[0], case, max_blocks=mb)
        assert texts == want, mb
        W.check_offsets(off, texts)
    check_irregular_inputs(name, case)


def check_irregular_inputs(name, case):
    """What a hand case must hold, from its inputs and the oracle's rows alone (both tiers)."""
    irr = {k: np.flatnonzero(case.irregular[k]) for k in W.LISTS}
    rows = case.py_rows({k: [int(i) for i in irr[k]] for k in W.LISTS})
    if name in ("alignment", "nine_chunks"):
        n = case.n["main"]
        assert len(irr["main"]) == n and set(irr["main"] // W.CHUNK) == set(range((n + W.CHUNK - 1) // W.CHUNK))
        whole = case.py_rows()["main"]                               # (every row is irregular: the offsets are the text's)
        at, lens, digits = W.irregular_stats([whole[i] for i in range(n)])
        assert at == set(range(8)) and lens == set(range(8)) and digits == set(range(1, 20)), (at, lens, digits)
        assert set(bool(f) for f in case.va["aln_fwd"]) == {True, False} and set(len(case.name_of(c)) for c in range(n)) == set(range(1, 18))
    elif name == "mixed":
        for k in W.LISTS:
            s = set(int(i) for i in irr[k])
            assert {0, W.CHUNK - 1, W.CHUNK, 2 * W.CHUNK - 1, W.MIXED_N - 1} <= s and not any(i // W.CHUNK == 2 for i in s)
            assert set(i // W.CHUNK for i in s) == {0, 1, 3}
            kinds = W.mixed_kinds()[k]
            beside = set(kinds[j] for i in (0, W.CHUNK - 1, W.CHUNK, 2 * W.CHUNK - 1, W.MIXED_N - 1) for j in (i - 1, i + 1) if 0 <= j < W.MIXED_N)
            assert beside == {"U", "R", "I"}
        names = [rows["all"][int(i)].split(b"\t")[0] for i in irr["all"]]
        for suffix in (b"k0.1", b"k0.10", b"k0.100"):
            assert names.count(suffix) == 2, suffix                  # both rows of the path
    elif name == "long":
        for k, i, units in (("main", 2, 70000), ("alt", 1, 70000), ("all", 0, 70000), ("main", 4, (1 << 20) // len(W.LONG_UNIT))):
            e = case.out[k][i]
            r = int(case.va["ctg_rec_off"][case.owners()[k][i][0]]) + int(e["ctg_index"])
            assert len(case.oracle_cut(k, i)[0]) == len(case.tag_of(r)) - units, (k, i)
        assert len(case.tag_of(4)) > (1 << 20)


def ranges_case():
    """40 rows per list, every third one irregular (the first and the last among them), the others uncut and regular in turn."""
    kinds = "".join("I" if i % 3 == 0 else "UR"[i % 2] for i in range(40))
    return W.kinds_case({"main": kinds, "alt": kinds[::-1], "all": kinds})


def test_irregular_ranges(emw, emc):
    """Every split point of 40-row lists with irregular rows: the two ranges concatenate to the whole; every irregular row formatted
    alone is that row; the guard bytes around every range stay untouched (emul_format)."""
    case = W.consistent_plans(emc, ranges_case())
    info, off, texts = W.emul_texts(emw[0], case)
    assert texts == W.joined_py(case)
    rows = case.py_rows()
    for l, k in enumerate(W.LISTS):
        for e in range(41):
            a, b = W.emul_format(emw[0], case, info, off, l, 0, e), W.emul_format(emw[0], case, info, off, l, e, 40)
            assert a[0] == 0 and b[0] == 0 and a[1] + b[1] == texts[l], (l, e)
        for i in np.flatnonzero(case.irregular[k]):
            assert W.emul_format(emw[0], case, info, off, l, int(i), int(i) + 1) == (0, rows[k][int(i)]), (k, i)
    assert case.irregular["main"][0] and case.irregular["main"][39] and case.irregular["main"].sum() == 14


# ---- results of real size (the text fuzz's joined texts) -----------------------------------------------------------------------------
@pytest.mark.parametrize("first", (0, 10))
def test_joined_texts(T, emw, emc, first):
    """Ten shaped texts as one file, both runs: main has three fill chunks or more and irregular rows in three of them or more
    (counted on plans checked against the oracle); the emulated rows are the oracle's files, at the full grid and at 3 blocks."""
    text = F.joined([F.shaped_text(i) for i in range(first, first + 10)])
    for K, nsl in F.RUNS:
        exp, case = fuzz_case(T, emw, emc, text, K, nsl)
        assert exp.kind == "ok"
        irr = W.oracle_checked_irregular(T, exp, case.plans)
        assert case.n["main"] > 2 * W.CHUNK and len(set(i // W.CHUNK for i in irr["main"])) >= 3, (case.n, irr["main"])
        for mb in (0, 3):
            info, off, texts = W.emul_texts(emw[0], case, max_blocks=mb)
            assert texts == list(exp.files), (K, mb)
        W.check_offsets(off, texts)


# ---- the device writer's pieces (rows_cut_pieces, aasm_rows.h) ---------------------------------------------------------------------
def piece_offsets(n, shape):
    """Offsets of n rows: "uniform" (37 bytes each), "random" (seeded, 1 - 400 bytes), ("giant", g): 37 bytes and row g of 10^6."""
    if shape == "uniform":
        lens = np.full(n, 37, np.int64)
    elif shape == "random":
        lens = np.random.default_rng(1024 + n).integers(1, 401, n).astype(np.int64)
    else:
        lens = np.full(n, 37, np.int64)
        lens[shape[1]] = 10 ** 6
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


PIECE_N = (0, 1, 1023, 1024, 1025, 2047, 2048, 2049, 3 * 1024 + 5)


def test_cut_pieces_contract(emw):
    """rows_cut_pieces over host arrays: the pieces cover the list in order without gap or overlap, start and end at the rows'
    offsets, hold at most `limit` bytes or one row; a limit of the whole text gives one piece; where every block of 1024 rows fits,
    every piece starts at a sample; the rows' own offsets are fetched only for blocks that do not fit, once each.  Both branches
    produce several pieces, alone and mixed, also where n is a multiple of 1024 and where the limit is a block's bytes."""
    lib = emw[0]
    seen = {"samples_only": 0, "rows_only": 0, "mixed": 0, "limit_is_block": 0, "long_row_in_block": 0}
    for n in PIECE_N:
        shapes = ["uniform", "random"] + [("giant", g) for g in sorted(set(g for g in (0, 1023, 1024, n - 1) if 0 <= g < n))]
        for shape in shapes:
            off = piece_offsets(n, shape)
            total, lens = int(off[-1]), np.diff(off)
            block = int(off[min(n, W.SAMPLE)])
            limits = {1, total, total - 1, block, block - 1, block + 1, block + block // 2}
            if n:
                limits |= {int(lens.min()), int(lens.max()), int(lens.max()) - 1}
            for limit in sorted(v for v in limits if v >= 1):
                pieces, calls = W.emul_cut_pieces(lib, off, limit)
                by_samples, by_rows = W.check_pieces(off, limit, pieces, calls)
                seen["samples_only"] += by_samples > 1 and by_rows == 0
                seen["rows_only"] += by_rows > 1 and by_samples == 0
                seen["mixed"] += by_samples >= 1 and by_rows >= 1
                seen["limit_is_block"] += limit == block and n > W.SAMPLE
                seen["long_row_in_block"] += n > 1 and int(lens.max()) > limit >= int(lens.min())
    assert all(v > 0 for v in seen.values()), seen


def test_sanitizer_program(T, emw, emc, tmp_path):
    """rows_emul_san (host address + undefined sanitizers; every tag in a block that ends with it, every list's text in a block of
    exactly its bytes) on the shaped corpus, the alignment case, the long rows and the hand-made irregular rows (all of three
    chunks, the long tags): exit 0 and the expected bytes."""
    lib, san = emw
    for i in range(0, 30, 3):
        K, nsl = F.RUNS[i % 2]
        exp, case = fuzz_case(T, emw, emc, F.shaped_text(i), K, nsl)
        assert W.run_san(san, case, tmp_path, "shaped%d" % i) == b"".join(exp.files), i
    for name, case in (("align", W.alignment_case()), ("long", W.long_case()), ("sized", W.sized_case(2 * W.CHUNK + 1, 5, W.CHUNK + 3)),
                       ("irregular_align", W.consistent_plans(emc, W.irregular_alignment_case())), ("irregular_long", W.consistent_plans(emc, W.long_irregular_case()))):
        assert W.run_san(san, case, tmp_path, name) == b"".join(W.joined_py(case)), name


def test_cli_refuses_device_writer_with_host_ranges_or_several_gpus(T, tmp_path):
    """--device-writer needs the tags on one device: a usage error (exit 1, nothing read) with --host-ranges and with --gpus 2."""
    import subprocess
    exe = os.path.join(T.ROOT, "alignasm_amd", "alignasm")
    for extra, text in ((["--host-ranges"], "--device-writer: not with --host-ranges"), (["--gpus", "2"], "--device-writer: not with --gpus above 1")):
        r = subprocess.run([exe, str(tmp_path / "none.paf"), "--device-writer"] + extra, capture_output=True, text=True)
        assert r.returncode == 1 and text in r.stderr and "Usage: alignasm" in r.stderr, (extra, r.stderr)
    assert "--device-writer" in subprocess.run([exe, "--help"], capture_output=True, text=True).stdout


def test_the_entries_exist_and_the_structs_have_the_header_layout(T):
    """What fails first without the feature: the C-ABI entries, the emulation sources and the ctypes layouts."""
    api = T.api()
    for name in ("aasm_paf_upload_rows", "aasm_rows_sizes_device", "aasm_rows_format_device", "aasm_writer_append_device"):
        assert hasattr(api.LIB, name) and name in api.EXPORTED
    assert C.sizeof(_abi.RowCols) == 72 and C.sizeof(_abi.DevRows) == 24 and C.sizeof(_abi.RowsInfo) == 48
    assert api.LIB.aasm_abi_version() == 3
    null = C.c_void_p()
    assert api.LIB.aasm_rows_sizes_device(null, null, null, null, null, null, 0, 0, null, null) == _abi.AASM_E_INVAL
    assert api.LIB.aasm_writer_append_device(null, null, null, null, null, null, null, C.c_int64(0), C.c_int64(0), 0) == _abi.AASM_E_INVAL
