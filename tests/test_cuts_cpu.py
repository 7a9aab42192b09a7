"""CPU tier of the cut plans (aasm_cut_plans_device / aasm_writer_append_cuts): the C-ABI surface and the ctypes mirrors, the
kernel body (1-lane host emulation, tests/host_emul/cuts_emul.cpp) against vectors recorded from the reference's get_edited_paf_data and
against the host codec on solver output, the planned writer byte for byte against the walking one, and damaged tags under a host
address sanitizer."""
import ctypes as C
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import cs_cases as G
import cuts_testlib as X
from alignasm_amd import _abi
from test_cs_ref import _accepted_text, _file_level, _paf_line
from test_export_cpu import CASE_IDS, CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "alignasm_amd.h")
NEW_FUNCS = ("aasm_cut_plans_device", "aasm_writer_append_cuts")


@pytest.fixture(scope="module")
def emc():
    return X.build_emul(san=True)


# ---- 0. the build of the emulation: once per process, the sanitizer program only where asked ----------------------------------
def test_build_emul_builds_once_and_no_program_unasked(T, emc, monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("build_emul started a process for a target this process has built: %r" % (args,))
    with monkeypatch.context() as m:                                 # the fixture built library and program: no second make
        m.setattr(T.subprocess, "run", refuse)
        assert X.build_emul() is emc[0] and X.build_emul(san=True) == emc and T.build_emul("cuts") is emc[0]
    assert os.path.dirname(emc[1]) == T._emul["dir"] and os.path.basename(emc[1]) == "cuts_emul_san"
    # a process that never asks for a program builds none: a cache of its own, as a fresh process has it
    monkeypatch.setattr(T, "_emul", {})
    lib = T.build_emul("cuts")
    try:
        assert lib is not emc[0] and T._emul["dir"] != os.path.dirname(emc[1])
        assert sorted(os.listdir(T._emul["dir"])) == ["libaasm_emul_cuts.so"]
        monkeypatch.setattr(T.subprocess, "run", refuse)
        assert T.build_emul("cuts") is lib
    finally:
        shutil.rmtree(T._emul["dir"])


# ---- 1. the surface ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_cut_plans():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"int\s+aasm_cut_plans_device\s*\(\s*const\s+aasm_batch_in\s*\*\s*dev_in\s*,\s*const\s+aasm_out_sizes\s*\*\s*sz\s*,\s*const\s+aasm_dev_out\s*\*\s*dev_out\s*,"
                     r"\s*const\s+aasm_dev_cuts\s*\*\s*dst\s*,\s*int\s+device\s*,\s*void\s*\*\s*stream\s*\)", src)
    assert re.search(r"int\s+aasm_writer_append_cuts\s*\(\s*aasm_writer\s*\*\s*w\s*,\s*const\s+aasm_paf\s*\*\s*paf\s*,\s*const\s+aasm_batch_out\s*\*\s*out\s*,"
                     r"\s*const\s+aasm_cuts\s*\*\s*cuts\s*,\s*int64_t\s+contig0\s*\)", src)
    for st in ("aasm_cut_plan", "aasm_dev_cuts", "aasm_cuts"):
        assert re.search(r"typedef\s+struct\s+%s\s*\{" % st, src)
    for name, v in (("IS_CUT", 0x1), ("IRREGULAR", 0x2), ("E_TAG", 0x10), ("E_INS_CLIP", 0x20), ("E_EDIT", 0x40), ("E_RECORD", 0x80)):
        assert re.search(r"#define\s+AASM_CUT_%s\s+0x%x\b" % (name, v), src, flags=re.I)
        assert getattr(_abi, "AASM_CUT_" + name) == v
    assert re.search(r"#define\s+AASM_ABI_VERSION\s+3\b", src)


def test_library_exports_the_cut_plans(T):
    api = T.api()
    for n in NEW_FUNCS:
        assert n in api.EXPORTED
        assert hasattr(api.LIB, n)
    assert api.LIB.aasm_abi_version() == 3


def test_ctypes_mirrors_have_the_header_sizes(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx is not None                                           # (the emulation below needs it anyway)
    mirrors = {"aasm_cut_plan": _abi.CutPlan, "aasm_dev_cuts": _abi.DevCuts, "aasm_cuts": _abi.Cuts}
    lines = ['#include <cstdio>', '#include <cstddef>', '#include "alignasm_amd.h"', "int main() {"]
    for st, cls in mirrors.items():
        lines.append(f'  std::printf("%zu\\n", sizeof({st}));')
        lines += [f'  std::printf("%zu\\n", offsetof({st}, {n}));' for n, _ in cls._fields_]
    lines.append("  return 0; }")
    (tmp_path / "probe.cpp").write_text("\n".join(lines) + "\n")
    subprocess.run([cxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), "probe.cpp", "-o", "probe"], cwd=tmp_path, check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for cls in mirrors.values():
        want.append(C.sizeof(cls))
        want += [getattr(cls, n).offset for n, _ in cls._fields_]
    assert got == want
    assert C.sizeof(_abi.CutPlan) == 48 and _abi.CUT_DT.itemsize == 48
    assert [(n, _abi.CUT_DT.fields[n][1]) for n in _abi.CUT_DT.names] == [(n, getattr(_abi.CutPlan, n).offset) for n, _ in _abi.CutPlan._fields_]


# ---- 2. the kernel against the reference's get_edited_paf_data ----------------------------------------------------------------
def check_recorded(rows, out, where, plans):
    """Plans of the hand-made elements against the recorded clips; returns the counts the fixture is known to hold."""
    n = {"cut": {(s, sh): 0 for s in (True, False) for sh in ("low", "high", "both")}, "err": 0, "uncut": 0, "irregular": 0}
    for k in X.LISTS:
        assert len(where[k]) == len(plans[k]) == len(out[k])
        for (i, j), p in zip(where[k], plans[k]):
            case, cl = rows[i], rows[i]["clips"][j]
            f = int(p["flags"])
            assert int(p["reserved"]) == 0
            if "err" in cl:
                n["err"] += 1
                assert f == (_abi.AASM_CUT_IS_CUT | X.ERR_FLAG[cl["err"][1]]), (case["cs"][:80], cl, f)
                assert p.tobytes()[:40] == b"\0" * 40
                continue
            assert not f & _abi.AASM_CUT_ERRORS, (case["cs"][:80], cl, f)
            assert bool(f & _abi.AASM_CUT_IS_CUT) == cl["cut"], (case["cs"][:80], cl, f)
            if not cl["cut"]:
                n["uncut"] += 1
                assert p.tobytes() == b"\0" * 48                     # the zero plan
                continue
            a, b = cl["clip"][:2]
            n["cut"][(case["fwd"], "both" if a > case["qs"] and b < case["qe"] else "low" if a > case["qs"] else "high")] += 1
            assert (int(p["mat_num"]), int(p["aln_len"])) == (cl["mat"], cl["aln"]), (case["cs"][:80], cl, p)
            if f & _abi.AASM_CUT_IRREGULAR:
                n["irregular"] += 1
            else:
                assert _abi.render_cut(p, case["cs"]) == cl["cs"], (case["cs"][:80], cl, p)
    return n


def assert_fixture_was_covered(n):
    """Nothing silently skipped: the fixture holds 1 084 cut clips (fwd 97 low / 88 high / 374 both, rev 111 / 81 / 333) and 183
    error clips in the accepted file-level cases."""
    for fwd in (True, False):
        assert sum(v for (s, _), v in n["cut"].items() if s == fwd) >= 500, n
        for sh in ("low", "high", "both"):
            assert n["cut"][(fwd, sh)] >= 80, n
    assert n["err"] >= 150 and n["uncut"] > 500 and n["irregular"] > 0, n


def test_emulated_kernel_equals_the_recorded_reference_vectors(T, emc):
    golden = X.golden_cs(T)
    paf, rows, out, where = X.golden_case_batch(T.api(), golden, _file_level, _accepted_text)
    assert all(_file_level(c) for c in rows) and len(rows) > 700
    assert sum(1 for c in rows if re.search(r":0\d", c["cs"])) >= 60   # tags with leading-zero runs
    view = paf.view()
    plans = X.emul_plans(emc[0], view, out)
    assert_fixture_was_covered(check_recorded(rows, out, where, plans))
    # fewer blocks than chunks (the grid-stride loop) and lists longer than a chunk: every contig's main / alt elements eight times
    big, idx = dict(out), {}
    for k in ("main", "alt"):
        o = out[k + "_off"]
        idx[k] = np.concatenate([np.tile(np.arange(o[x], o[x + 1]), 8) for x in range(out["n_contigs"])])
        big[k], big[k + "_off"] = out[k][idx[k]], o * 8
    assert len(big["main"]) > 2 * emc[0].emc_chunk()
    again = X.emul_plans(emc[0], view, big, 1)
    assert again["all"].tobytes() == plans["all"].tobytes()
    for k in ("main", "alt"):
        assert again[k].tobytes() == plans[k][idx[k]].tobytes()


@pytest.mark.ref
def test_emulated_kernel_equals_the_real_reference_codec_live(T, emc):
    if T.ref_cs() is None:
        pytest.skip("oracle/_ref/libaasm_ref_cs.so not built (no reference sources here)")
    rng = random.Random(20260117)
    rows, per = [], []
    for row in G.rows(rng.randrange(1 << 30), 700, 0):
        want = T.ref_cs_ranges(row)
        if want[0] == "err":
            continue
        clips = G.clips(rng, row, [(a, b, c) for a, b, c, _ in want[1]], 5)
        row = dict(row, clips=[])
        for cl in clips:
            we = T.ref_cs_edit(row, cl)
            row["clips"].append({"clip": list(cl), "err": [we[1], we[2]]} if we[0] == "err" else {"clip": list(cl), "cs": we[1], "mat": we[2], "aln": we[3], "cut": we[4]})
        rows.append(row)
        per.append({"main": [tuple(cl) + (0,) for cl in clips]})
    out = X.elements(per)
    where = {"main": [(i, j) for i, r in enumerate(rows) for j in range(len(r["clips"]))], "alt": [], "all": []}
    rb = X.RowsBatch(rows)                                           # (owns the arrays the view points at)
    n = check_recorded(rows, out, where, X.emul_plans(emc[0], rb.view, out))
    assert sum(n["cut"].values()) > 1500 and n["err"] > 100, n


def edge_file(T):
    """-> (Paf with the tags in its view, rows, clip pools) of the chunk-edge cases."""
    text, rows, pools = X.edge_text(T, _paf_line)
    return T.api().Paf.parse(text, device_ranges=True), rows, pools


def assert_edge_case(T, va, out, plans, case):
    n_main, n_alt, n_all, mode, _ = case
    assert (len(out["main"]), len(out["alt"]), len(out["all"])) == (n_main, n_alt, n_all)
    n_cut = sum(int((plans[k]["flags"] & _abi.AASM_CUT_IS_CUT != 0).sum()) for k in X.LISTS)
    total = n_main + n_alt + n_all
    assert n_cut == (total if mode == "cut" else 0 if mode == "none" else n_cut) and (mode != "mixed" or 0.3 * total < n_cut < 0.7 * total)
    n = X.check_by_key(T, va, out, plans)
    assert n["elements"] > 0 and (mode == "none" or n["cut"] > 0)


@pytest.mark.parametrize("case", X.edge_cases(), ids=lambda c: "%d_%d_%d_%s" % c[:4])
def test_emulated_kernel_at_the_chunk_edges(T, emc, case):
    """Lists of 1, 2047, 2048, 2049, 4096 and 4097 elements, all cut (the LDS list fills to exactly a chunk), none cut and mixed;
    contigs without elements on the chunk edges, .all paths that end on them or straddle them, empty paths; one block per chunk
    and one block for all of them.  Every plan against the host codec."""
    assert emc[0].emc_chunk() == X.CHUNK
    paf, rows, pools = edge_file(T)
    out = X.edge_lists(rows, pools, *case)
    va = X.view_arrays(paf.view())
    plans = X.emul_plans(emc[0], paf.view(), out)
    assert_edge_case(T, va, out, plans, case)
    again = X.emul_plans(emc[0], paf.view(), out, 1)
    for k in X.LISTS:
        assert again[k].tobytes() == plans[k].tobytes()


def test_emulated_kernel_flags_elements_outside_their_contig(T, emc):
    """AASM_CUT_E_RECORD: ctg_index -1 and ctg_index = the contig's record count (in the last contig: record n_records), as the
    first and the last element of a chunk and inside: flags exactly 0x80, every other word 0, the neighbours untouched."""
    paf, rows, pools = edge_file(T)
    good, bad, where = X.record_fault_lists(rows, pools)
    va = X.view_arrays(paf.view())
    assert X.record_of(bad, va["ctg_rec_off"])["main"][-1] == len(rows) == paf.view().n_records
    for max_blocks in (0, 1):
        gp = X.emul_plans(emc[0], paf.view(), good, max_blocks)
        X.check_record_faults(gp, X.emul_plans(emc[0], paf.view(), bad, max_blocks), where)
    assert not any(int(f) & _abi.AASM_CUT_E_RECORD for k in X.LISTS for f in gp[k]["flags"])


def test_emulated_kernel_equals_the_host_codec_on_random_clips(T, emc):
    """tests/cs_cases.py's random clips (ends on matched bases, anywhere in the record, inconsistent reference spans) of 1 400
    accepted rows against the host codec: the corpus the live-reference test runs where the reference is built."""
    rows, per = X.random_clip_corpus(T)
    out = X.elements(per)
    rb = X.RowsBatch(rows)
    va = {**rb.a, "ref_str": np.array([r["rs"] for r in rows], np.int64), "ref_end": np.array([r["re"] for r in rows], np.int64)}
    n = X.check_against_host(T, va, out, X.emul_plans(emc[0], rb.view, out))
    assert n["cut"] > 1500 and n["errors"] > 100 and n["irregular"] > 0, n


# ---- 3. the kernel against the host codec on solver output -------------------------------------------------------------------
def solved_case(T, case):
    nc, nr, seed, K, dense, dup, shuf, heavy, nsl = case
    paf = T.api().Paf.synth(nc, nr, seed, dense=dense, heavy_tail=heavy, dup_every=dup, shuffle=shuf)
    return paf, T.oracle_solve(paf.batch(), K, nsl)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_emulated_kernel_equals_the_host_codec_on_solver_output(T, emc, case):
    paf, out = solved_case(T, case)
    view = paf.view()
    plans = X.emul_plans(emc[0], view, out)
    n = X.check_against_host(T, X.view_arrays(view), out, plans)
    assert n["elements"] == len(out["main"]) + len(out["alt"]) + len(out["all"]) and n["errors"] == 0
    if case[1] > 1:
        assert n["cut"] >= 0.25 * n["elements"], n                  # (the oracle gives 32-80 % on these shapes)
    if case[5] and case[3] > 1:
        assert len(out["all"]) > 0 and any(int(f) & 1 for f in plans["all"]["flags"])   # the tie shapes exercise .all


# ---- 4. the planned writer -------------------------------------------------------------------------------------------------
def _both_ways(T, emc, paf, out, tmp_path, stem):
    plans = X.emul_plans(emc[0], paf.view(), out)
    bo, keep = X.pack_out(out)
    want = X.write_three(paf, bo, tmp_path, stem + "_walk")
    got = X.write_three(paf, bo, tmp_path, stem + "_plan", cuts=plans)
    assert got == want
    return plans, bo, keep, want


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_planned_writer_writes_the_same_bytes(T, emc, case, tmp_path):
    paf, out = solved_case(T, case)
    plans, _, _, want = _both_ways(T, emc, paf, out, tmp_path, "s")
    assert len(want[0]) > 0


@pytest.mark.parametrize("name", ["tiny", "dense"])
def test_planned_writer_writes_the_same_bytes_for_the_golden_files(T, emc, name, tmp_path):
    paf = T.api().Paf.read(os.path.join(T.GOLDEN, "files", name + ".paf"))
    out = T.oracle_solve(paf.batch(), 10000)
    _both_ways(T, emc, paf, out, tmp_path, name)


def test_planned_writer_reads_the_plans(T, emc, tmp_path):
    """Seeded faults: a changed head_keep changes the file; an error flag fails the append with the host codec's message; a
    stretch outside the tag, a plan of the wrong kind and wrong counts fail cleanly; nothing is left behind."""
    api = T.api()
    paf, out = solved_case(T, CASES[2])
    plans, bo, keep, want = _both_ways(T, emc, paf, out, tmp_path, "f")
    X.seeded_writer_faults(api, paf, bo, plans, want, tmp_path)


# ---- 5. damaged tags under the host address sanitizer -------------------------------------------------------------------------
def test_damaged_tags_stay_inside_the_tag_under_the_sanitizer(T, emc, tmp_path):
    rows, per = X.damaged_corpus()
    assert set(G.DAMAGED) <= {r["cs"] for r in rows} and len(rows) > 800
    out = X.elements(per)
    rb = X.RowsBatch(rows)
    plans = X.emul_plans(emc[0], rb.view, out)["main"]
    # the same through the sanitizer build: a read behind a tag ends the program
    words = [np.array([len(rows), len(out["main"]), int(rb.a["rec_cs_off"][-1])], np.int64), rb.a["qry_str"], rb.a["qry_end"], rb.a["rec_cs_off"], out["main_off"], out["main"]]
    blob = b"".join(np.ascontiguousarray(w).tobytes() for w in words) + rb.a["aln_fwd"].tobytes() + rb.a["cs_text"].tobytes()
    (tmp_path / "in.bin").write_bytes(blob + b"\0" * (-len(blob) % 8 + 8))
    r = subprocess.run([emc[1], str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    san = np.frombuffer((tmp_path / "out.bin").read_bytes(), _abi.CUT_DT)
    assert san.tobytes() == plans.tobytes()
    # flags are an error or a plan; where the host codec accepts the clip the plan is its answer
    va = {**rb.a, "ref_str": np.array([r["rs"] for r in rows], np.int64), "ref_end": np.array([r["re"] for r in rows], np.int64)}
    n_err = n_plan = n_no_prefix = 0
    for i, p in enumerate(plans):
        row = rows[i // 10]
        f, ln = int(p["flags"]), len(row["cs"])
        e = out["main"][i]
        want = T.product_cs_edit(row, (int(e["qs"]), int(e["qe"]), int(e["rs"]), int(e["re"])), 7, 9)
        if not row["cs"].startswith("cs:Z:") and (int(e["qs"]), int(e["qe"])) != (row["qs"], row["qe"]):
            n_no_prefix += 1
            assert f == _abi.AASM_CUT_IS_CUT | _abi.AASM_CUT_E_TAG  # (the first thing the walk looks at)
        if f & _abi.AASM_CUT_ERRORS:
            n_err += 1
            assert f & ~_abi.AASM_CUT_IS_CUT in (0x10, 0x20, 0x40) and p.tobytes()[:40] == b"\0" * 40
            assert want[0] == "err"
            if want[2] in X.ERR_FLAG:                                # no tokenizer error anywhere in the tag: the same finding
                assert f & _abi.AASM_CUT_ERRORS == X.ERR_FLAG[want[2]]
            continue
        n_plan += 1
        assert f & ~(_abi.AASM_CUT_IS_CUT | _abi.AASM_CUT_IRREGULAR) == 0 and int(p["reserved"]) == 0
        assert (p["keep_lo"] == p["keep_hi"] == 0) or 5 <= p["keep_lo"] < p["keep_hi"] <= ln
        if want[0] == "ok":
            X.check_against_host(T, va, {**out, "n_contigs": len(rows)}, {"main": plans, "alt": [], "all": []}, {"main": [i]})
        else:                                                        # the walk ended before the malformed operation: a tokenizer error, never a clip error
            assert want[2] not in X.ERR_FLAG, (row, e, want, p)
    assert n_plan >= len(rows) and n_err >= n_no_prefix > 0          # (every row's whole-record clip is a plan)
