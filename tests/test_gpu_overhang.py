"""GPU tier: records that run to or past the query's end (tests/overhang_cases.py) through every form that only runs on the card.

Such a record's edge into dest weighs (qry_total - qry_end - 1) * 2 <= 0, so walk score sums are negative - for whole contigs
(`zero`, the --alt merge's shape), for some contigs of a batch (`mixed`, `median`), or for the first part of one contig's K
walks (`centre`).  K8's sorted-runs queue (kb_enum_lsm) orders unsigned words and keeps sums biased by QE_SUM_BIAS for that
reason; the 1-lane emulation of the CPU tier runs the d-ary heap in its place, so its flush, run merges, cut, front refill and
far-tier threshold meet these sums here only, as do the 64-bit lane moves, the chain class, the several-waves heaps and two
contigs per wave.  Every comparison is exact.  Each test first asserts, on the oracle alone (O.profile), that its inputs hold
what they are meant to hold."""
import re

import numpy as np
import pytest

import overhang_cases as O
import text_fuzz as F
import wide_cases as W
from poison_testlib import BYTE_IDS, BYTES, guarded, poisoned
from test_fuzz import make_batch
from test_gpu_enum import check_queue_forms

pytestmark = pytest.mark.gpu
S, D = False, True
WIDE_L = 10 ** 8


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("the GPU tier needs torch to see the device")
    return torch


def _make(T, shape, mode):
    nc, nr, seed, K, dense, dup = shape
    base = T.synth(nc, nr, seed, dense=dense, dup_every=dup)
    return O.centre(base, K) if mode == "centre" else O.overhang(base, mode, seed)


def _check_profile(hb, K, mode, where, share=4):
    """The cell's inputs on the oracle alone -> the profile rows (printed: found, negative, min, max per contig).  centre: at
    least 1 / share of each contig's walks on each side of zero (share = 0: at least one walk)."""
    rows = O.profile(hb, K)
    print("profile %s: %s" % (where, rows), flush=True)
    if mode == "zero":
        assert all(found >= 1 and neg == found for found, neg, _, _ in rows), rows
    if mode == "centre":
        assert len(hb.skipped) <= 1, hb.skipped
        for c, (found, neg, _, _) in enumerate(rows):
            need = max(1, found // share) if share else 1
            if c not in hb.skipped:
                assert found >= 4 and neg >= need and found - neg >= need, (c, rows[c])
    return rows


# ---- a. K8's queue forms on negative and crossing sums ---------------------------------------------------------------------------
#         (contigs, records, seed, K, dense, dup_every), modes
QUEUE_SHAPES = [((6, 30, 4, 10000, S, 0), ("zero", "mixed", "centre")),   # wide spread of sums: the far tier's threshold moves several times; one contig's queue runs empty before K
                ((3, 1000, 21, 10000, S, 0), ("zero", "centre")),
                ((2, 400, 31, 10000, D, 0), ("median", "centre")),         # median: one contig all negative and one all positive in one batch
                ((4, 600, 9, 64, S, 0), ("zero", "centre")),               # K at one front
                ((4, 600, 9, 70, S, 0), ("zero", "centre")),               # ... and just past it
                ((1, 3000, 8, 30000, S, 0), ("zero",)),                    # lmax = 9
                ((3, 300, 5, 2500, S, 3), ("centre",))]                    # ties that straddle zero
QUEUE_CELLS = [(shape, mode) for shape, modes in QUEUE_SHAPES for mode in modes]


def _cell_id(cell):
    (nc, nr, seed, K, dense, dup), mode = cell
    return "c%dx%d_s%d_k%d_%s%s_%s" % (nc, nr, seed, K, "D" if dense else "S", "_dup%d" % dup if dup else "", mode)


@pytest.mark.parametrize("cell", QUEUE_CELLS, ids=_cell_id)
def test_queue_forms_on_negative_and_crossing_sums(T, cell):
    """runs / runs40 / heap agree on kfound, every popped distance, every pop's insertion index, every push's (node,
    predecessor) and the outputs; runs equals the oracle in every intermediate and in the outputs."""
    shape, mode = cell
    K = shape[3]
    hb = _make(T, shape, mode)
    rows = _check_profile(hb, K, mode, _cell_id(cell))
    if shape[:3] == (2, 400, 31) and mode == "median":
        assert rows[0][1] == rows[0][0] and rows[1][1] == 0, rows
    if shape[:3] == (6, 30, 4):
        assert any(found < K for found, _, _, _ in rows) and max(hi - lo for _, _, lo, hi in rows) > 50000, rows
    if mode == "mixed":
        assert any(neg == found for found, neg, _, _ in rows) and any(neg < found for found, neg, _, _ in rows), rows
    check_queue_forms(T, hb, K, expect=O.expect(hb, K))
    O.forget()


# ---- b. mixed batches at K around the front's capacity -----------------------------------------------------------------------------
def test_queue_forms_agree_on_mixed_overhang_batches_and_many_k(T):
    """test_gpu_enum.test_queue_forms_agree_on_mixed_batches_and_many_k's three batches with qry_total = 0 on half of each contig's
    records: all-negative contigs beside contigs with non-negative walks in every batch (profile at K = 130: sums only grow with
    the rank, so a non-negative walk there is one at any larger K)."""
    api = T.api()
    n_checked = 0
    for seed, nc, nr, dense, dup, heavy in ((1, 40, 300, False, 0, True), (3, 16, 220, True, 0, False), (4, 30, 120, True, 2, True)):
        hb = O.overhang(T.synth(nc, nr, seed, dense=dense, dup_every=dup, heavy_tail=heavy), "mixed", seed)
        rows = O.profile(hb, 130)
        O.forget()
        assert any(found and neg == found for found, neg, _, _ in rows) and any(neg < found for found, neg, _, _ in rows), rows
        db = api.DeviceBatch(hb)
        for K in (22, 65, 130, 2500):
            got = {}
            for form in ("heap", "runs", "runs40"):
                res = db.solve(max_paths=K, keep_debug=True, enum_heap=(form == "heap"), enum_small=(form == "runs40"))
                got[form] = (res.debug("kfound", np.int32)[:nc].copy(), res.debug("kd", T.DIST_DT)[:nc * K].copy(), res.debug("klast", np.int32)[:nc * K].copy())
                res.close()
            for other in ("runs", "runs40"):
                a, b = got["heap"], got[other]
                assert np.array_equal(a[0], b[0]), (seed, K, other)
                for c in range(nc):
                    n = int(a[0][c])
                    assert np.array_equal(a[1][c * K:c * K + n], b[1][c * K:c * K + n]) and np.array_equal(a[2][c * K:c * K + n], b[2][c * K:c * K + n]), (seed, K, other, c)
                    n_checked += 1
        db.close()
    assert n_checked == 2 * 4 * (40 + 16 + 30)


# ---- c. launch forms (tests/test_gpu_parity.py's) ----------------------------------------------------------------------------------
FORMS = [dict(chain=c, chain_own_queue=q) for c in ("auto", "all", "none", "half") for q in (False, True)] + [
    dict(graph_launches=True), dict(graph_launches=True, chain="none"),
    dict(heap_waves="all"), dict(heap_waves="none"), dict(heap_waves="all", heap_block_waves=4), dict(heap_waves="all", heap_block_waves=8),
    dict(heap_waves="all", heap_block_waves=16), dict(heap_input_order=True), dict(heap_waves="all", heap_input_order=True),
    dict(sequential_select=True), dict(grid_order=True)] + [dict(chain=c, test_small_root_ring=True) for c in ("none", "half", "all")]
FUZZ_SETTINGS = ((10000, False), (3, True))                          # test_fuzz._run's
#               name, maker(T), mode, settings
LAUNCH_BATCHES = [("fuzz%d_%s" % (style, mode), (lambda T, style=style, mode=mode: O.overhang(make_batch(200 + style, 6, 30, WIDE_L, style), mode, style)), mode, FUZZ_SETTINGS)
                  for style in (0, 1, 2) for mode in ("mixed", "median")] + [
    ("ht12x700_zero", lambda T: O.overhang(T.synth(12, 700, 3, heavy_tail=True), "zero"), "zero", ((130, False),)),
    ("dense16x220_centre", lambda T: O.centre(T.synth(16, 220, 3, dense=True), 130), "centre", ((130, False),))]


@pytest.mark.parametrize("batch", LAUNCH_BATCHES, ids=lambda b: b[0])
def test_launch_forms_on_overhang_batches(T, batch):
    """Outputs and every intermediate against the oracle in each launch form.  (The out-of-memory range split of the same
    batches: tests/test_gpu_split_overhang.py.)"""
    name, make, mode, settings = batch
    api = T.api()
    hb = make(T)
    db = api.DeviceBatch(hb)
    n_neg = n_walks = 0
    for K, nsl in settings:
        rows = O.profile(hb, K, nsl) if nsl else _check_profile(hb, K, mode, "%s K=%d" % (name, K), share=0)   # (dense: long ties at 0, so walks on both sides, not a quarter)
        n_neg += sum(r[1] for r in rows); n_walks += sum(r[0] for r in rows)
        want = T.oracle_solve(hb, K, nsl)
        for hooks in FORMS:
            res = db.solve(max_paths=K, non_skip_linkable=nsl, keep_debug=True, **hooks)
            try:
                assert T.diff_outputs(want, res.fetch()) == [], (name, K, nsl, hooks)
                bad = T.diff_intermediates(hb, res.debug, K, nsl, expect=O.expect(hb, K, nsl))
                assert bad == [], (name, K, nsl, hooks, bad[:6])
            finally:
                res.close()
    db.close()
    O.forget()
    assert 0 < n_neg and (n_neg < n_walks or mode == "zero"), (name, n_neg, n_walks)


# ---- d. two contigs per wave ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style", [0, 1, 2])
def test_many_small_overhang_contigs(T, style):
    """2 700 contigs (the sweeps run two contigs per wave, 32 lanes each) with qry_total = 0 on half of each contig's records."""
    api = T.api()
    hb = O.overhang(make_batch(7, 2700, 14, WIDE_L, style), "mixed", 7)
    qt, qe = hb.arrays["qry_total"], hb.arrays["qry_end"]
    assert 0.3 * len(qt) < int((qe >= qt - 1).sum()) < 0.7 * len(qt)                       # dest edges <= 0
    for K, nsl in FUZZ_SETTINGS:
        want = T.oracle_solve(hb, K, nsl)
        got = api.solve_batch(hb, max_paths=K, non_skip_linkable=nsl)
        assert T.diff_outputs(want, got) == [], (style, K, nsl)


# ---- e. wide coordinates ---------------------------------------------------------------------------------------------------------------
WIDE_NAMES = ("crafted_top", "crafted+top", "syn+top", "fz0+top", "wf39_s0_y0", "wf39_s0_y1", "wf39_s0_y2")


@pytest.fixture(scope="module")
def wide_corpus(T):
    return dict(W.corpus(T))


@pytest.mark.parametrize("name", WIDE_NAMES)
def test_queue_forms_on_wide_overhang(T, wide_corpus, name):
    """wide_cases' contigs with query coordinates up to 2^40 - 1 and qry_total = 0: dest weights near -2^41 (-2^40 for the fuzz at
    L = 2^39), every sum far inside (-2^62, 2^62)."""
    hb = O.overhang(wide_corpus[name], "zero")
    off = hb.arrays["ctg_rec_off"]
    hb = hb.subset([c for c in range(hb.n_contigs) if off[c + 1] - off[c] > 1])       # (a contig of one record has no graph)
    K = 10000
    wmin = min(int(O.debug(hb, c, K)["csr_w_qry"].min()) for c in range(hb.n_contigs))
    rows = O.profile(hb, K)
    assert wmin < -(1 << (39 if name.startswith("wf39") else 40)) and all(-(1 << 62) < lo and hi < (1 << 62) for _, _, lo, hi in rows), (wmin, rows)
    assert sum(neg for _, neg, _, _ in rows) > 0
    check_queue_forms(T, hb, K, expect=O.expect(hb, K))
    O.forget()


# ---- f. poison -------------------------------------------------------------------------------------------------------------------------
POISON_CELLS = [cell for cell in QUEUE_CELLS if cell[0][:3] == (6, 30, 4) or cell[0][:4] == (4, 600, 9, 70)]


@pytest.mark.parametrize("byte", BYTES, ids=BYTE_IDS)
@pytest.mark.parametrize("cell", POISON_CELLS, ids=_cell_id)
def test_queue_forms_on_poisoned_memory(T, cell, byte):
    """(a)'s cells with working memory filled with 0xA5 / 0xFF before every solve: a queue slot, run or threshold read before it
    is written shows as a different answer."""
    shape, mode = cell
    api = T.api()
    hb = _make(T, shape, mode)
    _check_profile(hb, shape[3], mode, _cell_id(cell))
    with poisoned(api, byte):
        guarded(api, check_queue_forms, T, hb, shape[3], expect=O.expect(hb, shape[3]))
    O.forget()


# ---- g. downstream of the solve ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def overhang_paf_text(T):
    text = O.overhang_text(T.api().Paf.synth(40, 60, 11, dup_every=9).to_text(), "mixed")
    rows = [ln.split(b"\t") for ln in text.split(b"\n") if ln]
    n_over = sum(int(f[3]) > int(f[1]) for f in rows)
    assert 0.3 * len(rows) < n_over < 0.7 * len(rows)                # rows with qry_end beyond qry_total
    return text


def test_overhang_text_through_every_route(T, torch, tmp_path, overhang_paf_text):
    """Host ranges, K0 on the card, the device reader with export into caller buffers and cut plans: solutions equal the solver
    oracle, plans equal the host codec on every element, every route's three files equal oracle/paf_io_oracle.py's bytes (the
    host route's among them)."""
    from test_gpu_text_fuzz import routes
    for K, nsl in F.RUNS:
        exp, _ = routes(T, torch, overhang_paf_text, K, nsl, {}, tmp_path, "ov%d" % K)
        assert exp.kind == "ok"
    rows = O.profile(T.io_oracle_batch(exp.st), F.RUNS[0][0], F.RUNS[0][1])
    O.forget()
    assert any(found and neg == found for found, neg, _, _ in rows) and any(neg < found for found, neg, _, _ in rows), rows


def test_overhang_text_rows_formatted_and_written_on_the_device(T, torch, tmp_path, overhang_paf_text):
    """to_torch(rows=True) (aasm_rows_format_device) and the device writer in default pieces, pieces of 4096 bytes and a piece per
    row: the I/O oracle's files."""
    from test_gpu_rows_results import rows_and_writer
    for K, nsl in F.RUNS:
        rows_and_writer(T, torch, overhang_paf_text, K, nsl, tmp_path, lambda off: (0, 4096, 1))


def test_overhang_text_on_the_command_line(T, tmp_path, overhang_paf_text):
    """`alignasm` over the four flag sets of tests/test_cli_routes.py: exit code, stdout, stderr and the three files identical,
    and the files the I/O oracle's."""
    from test_cli_routes import R, W as DW, _run
    from test_golden import SUFFIXES
    exp = F.expected(T, overhang_paf_text, 10000, False)
    assert exp.kind == "ok"
    path = tmp_path / "ov.paf"
    path.write_bytes(overhang_paf_text)
    outs = [tmp_path / ("ov" + s) for s in SUFFIXES]
    runs = []
    for extra in ([], [R], [DW], [R, DW]):
        code, out, err = _run(T, [path] + extra)
        files = [p.read_bytes() if p.exists() else None for p in outs]
        for p in outs:
            if p.exists():
                p.unlink()
        runs.append((code, out, err, files))
    assert runs[1] == runs[0] and runs[2] == runs[0] and runs[3] == runs[0], [r[:3] for r in runs]
    assert runs[0][0] == 0 and runs[0][2] == "" and runs[0][3] == list(exp.files)
    assert re.fullmatch(r"File read complete\nAnalyze PAF \d+ data in parallel\nWrite output PAF file\n", runs[0][1])
