"""Helpers of the cut-plan tests (tests/test_cuts_cpu.py, tests/test_gpu_cuts.py): the emulated kernel, batches made by hand
from cs-codec cases, the host codec's answer per element, results as the C structures the writers take."""
import ctypes as C
import gzip
import json
import os
import subprocess

import numpy as np

from alignasm_amd._abi import (AASM_CUT_E_EDIT, AASM_CUT_E_INS_CLIP, AASM_CUT_E_RECORD, AASM_CUT_E_TAG, AASM_CUT_ERRORS, AASM_CUT_IRREGULAR, AASM_CUT_IS_CUT, AASM_E_INVAL,
                               AASM_E_PARSE, CUT_DT, OUT_ELEM_DTYPE, BatchIn, BatchOut, DevCuts,
                               DevOut, OutSizes, render_cut)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LISTS = ("main", "alt", "all")


def build_emul(out_dir):
    """tests/host_emul_cuts built into out_dir -> (library, path of the sanitizer program)."""
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "host_emul_cuts"), f"OUT={out_dir}"], check=True)
    lib = C.CDLL(os.path.join(str(out_dir), "libaasm_emul_cuts.so"))
    lib.emc_chunk.restype = C.c_int64
    return lib, os.path.join(str(out_dir), "cuts_emul_san")


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
