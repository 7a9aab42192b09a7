"""Helpers of the cut-plan tests (tests/test_cuts_cpu.py, tests/test_gpu_cuts.py): the emulated kernel, batches made by hand
from cs-codec cases, the host codec's answer per element, results as the C structures the writers take."""
import ctypes as C
import gzip
import json
import os

import numpy as np

import aasm_testlib
from alignasm_amd._abi import (AASM_CUT_E_EDIT, AASM_CUT_E_INS_CLIP, AASM_CUT_E_RECORD, AASM_CUT_E_TAG, AASM_CUT_ERRORS, AASM_CUT_IRREGULAR, AASM_CUT_IS_CUT, AASM_E_INVAL,
                               AASM_E_PARSE, CUT_DT, OUT_ELEM_DTYPE, BatchIn, BatchOut, DevCuts,
                               DevOut, OutSizes, render_cut)

LISTS = ("main", "alt", "all")


def _declare(lib):
    lib.emc_chunk.restype = C.c_int64


def build_emul(san=False):
    """tests/host_emul/cuts_emul.cpp -> its library, or with san (library, path of cuts_emul_san)."""
    return aasm_testlib.build_emul("cuts", san, _declare)


def golden_cs(T):
    with gzip.open(os.path.join(T.GOLDEN, "ref_cs.json.gz"), "rb") as f:
        return json.loads(f.read())


class RowsBatch:
    """One-record contigs made from cs-codec rows {cs, fwd, qs, qe}: host arrays + the BatchIn view over them."""

    def __init__(self, rows):
        n = len(rows)
        tags = [r["cs"].encode() for r in rows]
        self.a = {
            "ctg_rec_off": np.arange(n + 1, dtype=np.int64), "qry_str": np.array([r["qs"] for r in rows], np.int64),
            "qry_end": np.array([r["qe"] for r in rows], np.int64), "aln_fwd": np.array([1 if r["fwd"] else 0 for r in rows], np.uint8),
            "rec_cs_off": np.concatenate([[0], np.cumsum([len(t) for t in tags])]).astype(np.int64),
            "cs_text": np.frombuffer(b"".join(tags) + b"\0" * 8, np.uint8).copy(),
        }
        self.view = BatchIn()
        self.view.n_contigs = self.view.n_records = n
        for k, v in self.a.items():
            setattr(self.view, k, v.ctypes.data)


def elements(per_contig):
    """per_contig: for every contig {"main": [...], "alt": [...], "all": [[...], ...]} of (qs, qe, rs, re, ctg_index) ->
    the result arrays of unpack_out() (status 0, no stats)."""
    out = {k: [] for k in LISTS}
    off = {"main_off": [0], "alt_off": [0], "all_path_off": [0], "all_elem_off": [0]}
    for c in per_contig:
        for k in ("main", "alt"):
            out[k] += [e + (1 if k == "alt" else 0,) for e in c.get(k, ())]
            off[k + "_off"].append(len(out[k]))
        for path in c.get("all", ()):
            out["all"] += [e + (0,) for e in path]
            off["all_elem_off"].append(len(out["all"]))
        off["all_path_off"].append(len(off["all_elem_off"]) - 1)
    r = {k: np.array(v, np.int64) for k, v in off.items()}
    for k in LISTS:
        r[k] = np.array(out[k], OUT_ELEM_DTYPE) if out[k] else np.zeros(0, OUT_ELEM_DTYPE)
    r["n_contigs"] = len(per_contig)
    r["status"] = np.zeros(len(per_contig), np.int32)
    return r


def _ptr(a):
    return a.ctypes.data if a.size else None


def sizes_of(out):
    return OutSizes(int(out["n_contigs"]), len(out["main"]), len(out["alt"]), len(out["all_elem_off"]) - 1, len(out["all"]))


def emul_plans(lib, view, out, max_blocks=0):
    """The emulated kernel on host arrays -> {"main", "alt", "all"}: CUT_DT arrays (every plan must be written: the arrays
    start as 0x5a bytes)."""
    keep = {k: np.ascontiguousarray(out[k]) for k in ("main_off", "alt_off", "all_path_off", "all_elem_off") + LISTS}
    plans = {k: np.frombuffer(b"\x5a" * (48 * len(out[k])), CUT_DT).copy() for k in LISTS}
    dev_out = DevOut(_ptr(keep["main_off"]), _ptr(keep["alt_off"]), _ptr(keep["all_path_off"]), _ptr(keep["all_elem_off"]), _ptr(keep["main"]),
                     _ptr(keep["alt"]), _ptr(keep["all"]), None)
    dst = DevCuts(*(_ptr(plans[k]) for k in LISTS))
    sz = sizes_of(out)
    rc = lib.emc_cut_plans(C.byref(view), C.byref(sz), C.byref(dev_out), C.byref(dst), C.c_int64(max_blocks))
    assert rc == 0, rc
    return plans


def device_plans(api, db, out, stream=None):
    """aasm_cut_plans_device on a DeviceBatch and result arrays uploaded from numpy -> the plans, fetched to the host."""
    import torch
    dev = torch.device("cuda", db.device)
    st = stream or torch.cuda.current_stream(dev)
    with torch.cuda.stream(st):
        t = {k: torch.from_numpy(np.ascontiguousarray(out[k]).view(np.int64).reshape(-1)).to(dev) for k in ("main_off", "alt_off", "all_path_off", "all_elem_off") + LISTS}
        p = {k: torch.full((len(out[k]), 6), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device=dev) for k in LISTS}
    ptr = lambda x: x.data_ptr() if x.numel() else None   # noqa: E731
    dev_out = DevOut(ptr(t["main_off"]), ptr(t["alt_off"]), ptr(t["all_path_off"]), ptr(t["all_elem_off"]), ptr(t["main"]), ptr(t["alt"]), ptr(t["all"]), None)
    rc = api.cut_plans_raw(db.dev_view, sizes_of(out), dev_out, DevCuts(*(ptr(p[k]) for k in LISTS)), db.device, st.cuda_stream)
    assert rc == 0, (rc, api.LIB.aasm_last_error())
    st.synchronize()
    return api.cuts_to_numpy({k + "_cut": p[k] for k in LISTS})


def record_of(out, rec_off):
    """{"main", "alt", "all"}: the batch record of every element (contig from the offsets, as the kernel finds it)."""
    c_main = np.repeat(np.arange(out["n_contigs"]), np.diff(out["main_off"]))
    c_alt = np.repeat(np.arange(out["n_contigs"]), np.diff(out["alt_off"]))
    path_c = np.repeat(np.arange(out["n_contigs"]), np.diff(out["all_path_off"]))
    c_all = np.repeat(path_c, np.diff(out["all_elem_off"])) if len(path_c) else np.zeros(0, np.int64)
    return {k: rec_off[c].astype(np.int64) + out[k]["ctg_index"] for k, c in (("main", c_main), ("alt", c_alt), ("all", c_all))}


def tag_of(view_arrays, r):
    a, b = int(view_arrays["rec_cs_off"][r]), int(view_arrays["rec_cs_off"][r + 1])
    return view_arrays["cs_text"][a:b].tobytes().decode("latin-1")


def view_arrays(view: BatchIn):
    """numpy copies of what the kernel reads from a BatchIn with cs text."""
    from alignasm_amd._abi import _np_from
    c, r = int(view.n_contigs), int(view.n_records)
    a = {"ctg_rec_off": _np_from(view.ctg_rec_off, c + 1, np.int64), "qry_str": _np_from(view.qry_str, r, np.int64), "qry_end": _np_from(view.qry_end, r, np.int64),
         "aln_fwd": _np_from(view.aln_fwd, r, np.uint8), "rec_cs_off": _np_from(view.rec_cs_off, r + 1, np.int64)}
    a["ref_str"] = _np_from(view.ref_str, r, np.int64) if view.ref_str else np.zeros(r, np.int64)
    a["ref_end"] = _np_from(view.ref_end, r, np.int64) if view.ref_end else np.zeros(r, np.int64)
    a["cs_text"] = _np_from(view.cs_text, int(a["rec_cs_off"][-1]), np.uint8)
    return a


ERR_FLAG = {"Alignment was clipped inside a cs insertion": 0x20, "Edited cs tag does not match edited PAF coordinates": 0x40}


def check_against_host(T, va, out, plans, which=None):
    """Every element's plan (or those of `which`: {list: indices}) against aasm_cs_edit on the record's tag: is_cut, mat_num,
    aln_len, the rendered text (plans without IRREGULAR), the error.  Returns counts {elements, cut, irregular, errors}."""
    rec = record_of(out, va["ctg_rec_off"])
    n = {"elements": 0, "cut": 0, "irregular": 0, "errors": 0}
    for k in LISTS:
        idx = range(len(out[k])) if which is None else which.get(k, ())
        for i in idx:
            r, e, p = int(rec[k][i]), out[k][i], plans[k][i]
            row = {"cs": tag_of(va, r), "fwd": bool(va["aln_fwd"][r]), "qs": int(va["qry_str"][r]), "qe": int(va["qry_end"][r]), "rs": int(va["ref_str"][r]), "re": int(va["ref_end"][r])}
            want = T.product_cs_edit(row, (int(e["qs"]), int(e["qe"]), int(e["rs"]), int(e["re"])), 7, 9)
            n["elements"] += 1
            f = int(p["flags"])
            assert int(p["reserved"]) == 0
            if want[0] == "err":
                n["errors"] += 1
                assert f & AASM_CUT_ERRORS == ERR_FLAG[want[2]], (k, i, row["cs"][:60], want, f)
                continue
            assert not f & AASM_CUT_ERRORS, (k, i, row["cs"][:60], want, f)
            assert bool(f & AASM_CUT_IS_CUT) == want[4], (k, i)
            if not want[4]:
                assert p.tobytes() == b"\0" * 48, (k, i)
                continue
            n["cut"] += 1
            assert (int(p["mat_num"]), int(p["aln_len"])) == (want[2], want[3]), (k, i, row["cs"][:60], want, p)
            if f & AASM_CUT_IRREGULAR:
                n["irregular"] += 1
            else:
                assert render_cut(p, row["cs"]) == want[1], (k, i, row["cs"][:60], want[1][:60], p)
    return n


def pack_out(out):
    """unpack_out()'s arrays as a BatchOut over them (keep the returned arrays alive while it is used)."""
    keep = {k: np.ascontiguousarray(out[k]) for k in ("main_off", "alt_off", "all_path_off", "all_elem_off", "status") + LISTS}
    bo = BatchOut()
    bo.n_contigs = int(out["n_contigs"])
    bo.main_off, bo.alt_off, bo.all_path_off, bo.all_elem_off = (keep[k].ctypes.data for k in ("main_off", "alt_off", "all_path_off", "all_elem_off"))
    bo.main_elems, bo.alt_elems, bo.all_elems = (keep[k].ctypes.data for k in LISTS)
    bo.n_all_paths = len(keep["all_elem_off"]) - 1
    bo.ctg_status = keep["status"].ctypes.data
    return bo, keep


def write_three(paf, bo, d, stem, cuts=None):
    paths = [os.path.join(str(d), stem + s) for s in (".aln.paf", ".aln.alt.paf", ".aln.all.paf")]
    paf.write_outputs(bo, *paths, cuts=cuts)
    return [open(p, "rb").read() for p in paths]


def seeded_writer_faults(api, paf, bo, plans, want, tmp_path):
    """The planned writer really reads the plans (`want`: the three files of the walking writer): a changed head_keep changes the
    main file; an error flag fails the append with the host codec's code and message; a stretch outside the tag, a plan of the
    wrong kind and wrong counts fail cleanly (AASM_E_INVAL); a failed append leaves no file behind."""
    import pytest
    heads = np.flatnonzero(plans["main"]["head_keep"] > 0)
    stretch = np.flatnonzero(plans["main"]["keep_hi"] > plans["main"]["keep_lo"])
    uncut = np.flatnonzero(plans["main"]["flags"] == 0)
    assert len(heads) and len(stretch) and len(uncut)

    def seeded(i, **fields):
        p = {k: v.copy() for k, v in plans.items()}
        for f, v in fields.items():
            p["main"][f][i] = v
        return p
    got = write_three(paf, bo, tmp_path, "f_head", cuts=seeded(heads[0], head_keep=plans["main"]["head_keep"][heads[0]] + 1))
    assert got[0] != want[0] and got[1:] == want[1:]
    texts = {AASM_CUT_E_INS_CLIP: "Alignment was clipped inside a cs insertion", AASM_CUT_E_EDIT: "Edited cs tag does not match edited PAF coordinates",
             AASM_CUT_E_TAG: "PAF record does not contain a short-form cs:Z tag"}
    for flag, text in texts.items():
        with pytest.raises(api.AlignasmError) as e:
            write_three(paf, bo, tmp_path, "f_err%d" % flag, cuts=seeded(stretch[0], flags=AASM_CUT_IS_CUT | flag))
        assert e.value.code == AASM_E_PARSE and text in str(e.value)
    big = 1 << 40                                                    # far behind any tag
    for what, p in (("hi", seeded(stretch[0], keep_hi=big)), ("lo", seeded(stretch[0], keep_lo=-3)), ("lo_gt_hi", seeded(stretch[0], keep_lo=plans["main"]["keep_hi"][stretch[0]] + 1)),
                    ("kind", seeded(uncut[0], flags=AASM_CUT_IS_CUT)), ("kind2", seeded(stretch[0], flags=0)), ("record", seeded(uncut[0], flags=AASM_CUT_E_RECORD)),
                    ("count", {**plans, "main": plans["main"][:-1]})):
        with pytest.raises(api.AlignasmError) as e:
            write_three(paf, bo, tmp_path, "f_" + what, cuts=p)
        assert e.value.code == AASM_E_INVAL, what
    left = [f for f in os.listdir(tmp_path) if f.startswith(("f_err", "f_hi", "f_lo", "f_kind", "f_record", "f_count"))]
    assert left == []


def golden_case_batch(api, golden, file_level, accepted_text):
    """The recorded accepted cases as one parsed file (device ranges: cs text in the view) + one hand-made element per recorded
    clip, dealt over main / alt / .all -> (paf, rows, out, where): where[list][i] = (row index, clip index)."""
    rows, text = accepted_text(golden)
    paf = api.Paf.parse(text, device_ranges=True)
    per, where, tmp = [], {k: [] for k in LISTS}, []
    for i, c in enumerate(rows):
        if i % 16 == 0:
            per.append({"main": [], "alt": [], "all": [[], []]})
            tmp.append({"main": [], "alt": [], "all": [[], []]})
        for j, cl in enumerate(c.get("clips", ())):
            e = tuple(cl["clip"]) + (i % 16,)
            k = LISTS[(i + j) % 3]
            if k == "all":
                per[-1]["all"][j % 2].append(e); tmp[-1]["all"][j % 2].append((i, j))
            else:
                per[-1][k].append(e); tmp[-1][k].append((i, j))
    for t in tmp:                                                    # the element order elements() produces
        where["main"] += t["main"]; where["alt"] += t["alt"]; where["all"] += t["all"][0] + t["all"][1]
    return paf, rows, elements(per), where


# ---- hand-made lists for the kernel's chunk loop (tests/test_cuts_cpu.py in the emulation, tests/test_gpu_cuts.py on the card) ----
CHUNK = 2048                                                         # AASM_CUT_CHUNK (the emulation library reports it: emc_chunk)
EDGE_SIZES = (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1)
# elements per contig (main, alt), cycled until the list is full: offsets meet both chunk edges, with contigs of no element on them
CONTIG_PATTERN = (1, 0, CHUNK - 2, 1, 0, 0, 1, CHUNK - 1, 0, 1)
# elements per .all path: empty paths, path ends on the edges, and (the second one) paths that straddle them
PATH_PATTERNS = ((0, 1, 1500, CHUNK - 1501, 0, 0, 1, 1300, CHUNK - 1301, 0, 1), (3, 0, 2000, 100, 0, 1945, 60, 0, 1))
EDGE_CONTIGS, EDGE_RECORDS = 24, 3


def _split(n, pattern):
    """n items dealt into pieces of the pattern's sizes, cycled; the empty pieces in between are kept."""
    out, k = [], 0
    while n > 0:
        out.append(min(n, pattern[k % len(pattern)]))
        n -= out[-1]
        k += 1
    return out


def edge_text(T, paf_line):
    """A small file of EDGE_CONTIGS contigs x EDGE_RECORDS records made from valid cs-codec rows -> (text, rows, per row a pool of
    re-cut clips with exact reference coordinates, every one accepted or refused by the host codec alone)."""
    import random
    import cs_cases as G
    rng = random.Random(2048)
    rows, pools = [], []
    for row in G.rows(31, 200, 0):
        got = T.product_cs_ranges(row)
        if got[0] == "err" or row["qe"] - row["qs"] < 3 or len(row["cs"]) > 400:
            continue
        pool = [c for c in G.clips(rng, row, [(a, b, c) for a, b, c, _ in got[1]], 12) if (c[0], c[1]) != (row["qs"], row["qe"])]
        if len(pool) >= 4:
            rows.append(row); pools.append(pool)
        if len(rows) == EDGE_CONTIGS * EDGE_RECORDS:
            break
    assert len(rows) == EDGE_CONTIGS * EDGE_RECORDS
    text = b"".join(paf_line(r, "e%d" % (i // EDGE_RECORDS)) for i, r in enumerate(rows))
    return text, rows, pools


def edge_lists(rows, pools, n_main, n_alt, n_all, mode, variant=0):
    """Result arrays with exactly n_main / n_alt / n_all elements laid out by CONTIG_PATTERN and PATH_PATTERNS[variant].
    mode: "cut" (every element re-cut), "none" (every element spans its record), "mixed"."""
    import random
    rng = random.Random("%d %d %d %s %d" % (n_main, n_alt, n_all, mode, variant))

    def element(c):
        i = rng.randrange(EDGE_RECORDS)
        row, pool = rows[c * EDGE_RECORDS + i], pools[c * EDGE_RECORDS + i]
        if mode == "none" or (mode == "mixed" and rng.random() < 0.5):
            return (row["qs"], row["qe"], row["rs"], row["re"], i)
        return tuple(rng.choice(pool)) + (i,)
    per = [{"main": [], "alt": [], "all": []} for _ in range(EDGE_CONTIGS)]
    for k, n in (("main", n_main), ("alt", n_alt)):
        sizes = _split(n, CONTIG_PATTERN)
        assert len(sizes) <= EDGE_CONTIGS - 2
        for c, m in enumerate(sizes):                                # (contig 0 ... ; the last two contigs hold nothing)
            per[c + (1 if k == "alt" else 0)][k] = [element(c + (1 if k == "alt" else 0)) for _ in range(m)]
    paths = _split(n_all, PATH_PATTERNS[variant])
    c = 0
    for p in range(0, len(paths), 2):                                # two paths per contig, every third contig without any
        if c % 3 == 2:
            c += 1
        per[c]["all"] = [[element(c) for _ in range(m)] for m in paths[p:p + 2]]
        c += 1
    assert c <= EDGE_CONTIGS
    return elements(per)


def edge_cases():
    """(n_main, n_alt, n_all, mode, variant): every list at every size of EDGE_SIZES in every mode."""
    out = []
    for m, mode in enumerate(("cut", "none", "mixed")):
        for s in range(len(EDGE_SIZES)):
            out.append((EDGE_SIZES[s], EDGE_SIZES[(s + 2) % 6], EDGE_SIZES[(s + 4) % 6], mode, (s + m) % 2))
    return out


def check_by_key(T, va, out, plans):
    """check_against_host on one element of every distinct (record, clip); every other element's plan equals its
    representative's byte for byte.  Returns check_against_host's counts (of the representatives)."""
    rec = record_of(out, va["ctg_rec_off"])
    which = {}
    for k in LISTS:
        if not len(out[k]):
            continue
        key = np.stack([rec[k], out[k]["qs"], out[k]["qe"], out[k]["rs"], out[k]["re"]], 1)
        _, first, inverse = np.unique(key, axis=0, return_index=True, return_inverse=True)
        p = np.ascontiguousarray(plans[k]).view(np.int64).reshape(-1, 6)
        assert np.array_equal(p, p[first[inverse.reshape(-1)]]), k
        which[k] = [int(i) for i in first]
    return check_against_host(T, va, out, plans, which)


RECORD_PLAN = np.array([0, 0, 0, 0, 0, AASM_CUT_E_RECORD], np.int64).tobytes()


def record_fault_lists(rows, pools):
    """-> (good, bad, where): lists of 2 * CHUNK + 1 elements each, and the same with ctg_index -1 or the contig's record count
    at where[list]: the first and the last element of both chunks and a few inside.  The last main element belongs to the
    file's last contig, where the record index of the second kind is n_records."""
    good = edge_lists(rows, pools, 2 * CHUNK + 1, 2 * CHUNK + 1, 2 * CHUNK + 1, "mixed", 0)
    off, last = good["main_off"], rows[(EDGE_CONTIGS - 1) * EDGE_RECORDS]
    off[(off == off[-1]) & (np.arange(len(off)) < EDGE_CONTIGS)] = off[-1] - 1
    good["main"][-1] = (last["qs"], last["qe"], last["rs"], last["re"], 0, 0)
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
    where = {}
    for k in LISTS:
        where[k] = [0, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 777, 2 * CHUNK, 1, 3000]
        for j, i in enumerate(where[k]):
            bad[k]["ctg_index"][i] = -1 if j % 2 == 0 else EDGE_RECORDS
    return good, bad, where


def check_record_faults(good_plans, bad_plans, where):
    for k in LISTS:
        g = np.ascontiguousarray(good_plans[k]).view(np.int64).reshape(-1, 6)
        b = np.ascontiguousarray(bad_plans[k]).view(np.int64).reshape(-1, 6)
        assert len(b) == 2 * CHUNK + 1
        for i in where[k]:
            assert b[i].tobytes() == RECORD_PLAN, (k, i, b[i])       # flags exactly 0x80, every other word 0
        keep = np.ones(len(b), bool)
        keep[where[k]] = False
        assert np.array_equal(g[keep], b[keep]), k                   # the neighbours' plans are untouched


def damaged_corpus():
    """The rows and clips of the damaged-tag test: a few valid tags, every damaged one (both strands); ten clips per row."""
    import random
    import cs_cases as G
    rng = random.Random(77)
    rows = [r for r in G.rows(5, 60, 400)]
    rows = rows[:60] + rows[2 * (60 + len(G.ODD_VALID)):]
    per = []
    for r in rows:
        qs, qe = r["qs"], r["qe"]
        cl = [(qs, qe), (qs + 1, qe), (qs, qe - 1), (qs - 1, qe + 1), (qe, qs)]
        for _ in range(5):
            a = rng.randint(qs, qe)
            cl.append((a, rng.randint(a, qe)))
        per.append({"main": [(a, b, r["rs"], r["re"], 0) for a, b in cl]})
    return rows, per


def random_clip_corpus(T, n_valid=700, n_clips=5):
    """tests/cs_cases.py's rows the host codec takes, with their random clips (ends on matched bases, anywhere, inconsistent
    reference spans) as main elements of one-record contigs -> (rows, per_contig)."""
    import random
    import cs_cases as G
    rng = random.Random(20261017)
    rows, per = [], []
    for row in G.rows(rng.randrange(1 << 30), n_valid, 0):
        got = T.product_cs_ranges(row)
        if got[0] == "err":
            continue
        rows.append(row)
        per.append({"main": [tuple(cl) + (0,) for cl in G.clips(rng, row, [(a, b, c) for a, b, c, _ in got[1]], n_clips)]})
    return rows, per
