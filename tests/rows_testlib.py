"""Helpers of the device-rows tests (tests/test_rows_cpu.py, tests/test_gpu_rows.py): the emulated kernels, batches made by hand,
the row layout restated in Python, and the same case on host arrays (emulation) or device tensors (the product's entries).

A case is a Case: the batch's arrays and the row columns as numpy arrays, a result in unpack_out()'s form and its cut plans.
Expected bytes never come from the code under test: the oracle's files, the host writers, or py_row() below with - for a tag
that is not a stretch of the record's own (AASM_CUT_IRREGULAR) - the I/O oracle's re-cut tag (oracle/paf_io_oracle.py)."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np

import aasm_testlib
import cuts_testlib as X
from alignasm_amd._abi import (AASM_CUT_IRREGULAR, AASM_CUT_IS_CUT, CUT_DT, OUT_ELEM_DTYPE, BatchIn, DevCuts, DevOut, DevRows, OutSizes, RowCols, RowsInfo,
                               _np_from, render_cut)

LISTS = X.LISTS
CHUNK = 128                                                          # AASM_ROWS_CHUNK (the emulation library reports it: emw_chunk)
LEN_CHUNK = 2048                                                     # the length pass's chunk (emw_len_chunk)
SAMPLE = 1024                                                        # AASM_ROWS_SAMPLE: the device writer's sampled row offsets (emw_sample)
IN_KEYS = (("ctg_rec_off", np.int64), ("qry_str", np.int64), ("qry_end", np.int64), ("qry_total", np.int64), ("ref_chr", np.int32), ("aln_fwd", np.uint8),
           ("map_qul", np.uint8), ("rec_cs_off", np.int64), ("cs_text", np.uint8))
COL_KEYS = (("ref_total", np.int64), ("mat_num", np.int32), ("aln_len", np.int32), ("row_index", np.int32), ("cord_type", np.uint8), ("names", np.uint8),
            ("ctg_name_off", np.int64), ("chr_name_off", np.int64))


def _declare(lib):
    lib.emw_chunk.restype = lib.emw_len_chunk.restype = C.c_int64
    lib.emw_cut_pieces.restype = lib.emw_cut_fetches.restype = lib.emw_sample.restype = C.c_int64
    assert lib.emw_chunk() == CHUNK and lib.emw_len_chunk() == LEN_CHUNK and lib.emw_sample() == SAMPLE


def build_emul(san=False):
    """tests/host_emul/rows_emul.cpp -> its library, or with san (library, path of rows_emul_san)."""
    return aasm_testlib.build_emul("rows", san, _declare)


# ---- the row layout, restated (the issue's contract; str() on Python ints) -------------------------------------------------------
def py_row(name, qtot, qs, qe, fwd, chr_name, rtot, rs, re, mat, aln, mq, is_alt, cord, row_index, tag):
    a, b = (rs, re) if fwd else (re, rs)
    cols = [name, str(qtot), str(qs), str(qe + 1), "+" if fwd else "-", chr_name, str(rtot), str(a), str(b + 1), str(mat), str(aln), str(mq),
            "tp:A:S" if is_alt else "tp:A:P", "xi:Z:%s_%d" % ("A" if cord else "P", row_index), tag]
    return ("\t".join(cols) + "\n").encode("latin-1")


class Case:
    def __init__(self, va, ca, out, plans):
        self.va = {k: np.ascontiguousarray(va[k], dt) for k, dt in IN_KEYS}
        self.ca = {k: np.ascontiguousarray(ca[k], dt) for k, dt in COL_KEYS}
        self.out = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in out.items()}
        self.plans = {k: np.ascontiguousarray(plans[k], CUT_DT) for k in LISTS}
        if self.va["cs_text"].size == 0:
            self.va["cs_text"] = np.zeros(8, np.uint8)
        if self.ca["names"].size == 0:
            self.ca["names"] = np.zeros(8, np.uint8)
        self.consistent, self.irregular, self._oracle = False, None, {}   # (consistent_case)

    n_chr = property(lambda self: len(self.ca["chr_name_off"]) - 1)
    n = property(lambda self: {k: len(self.out[k]) for k in LISTS})

    def host_structs(self):
        """(BatchIn, RowCols, OutSizes, DevOut, DevCuts) over the case's own numpy arrays."""
        view = BatchIn()
        view.n_contigs, view.n_records = len(self.va["ctg_rec_off"]) - 1, len(self.va["qry_str"])
        for k, _ in IN_KEYS:
            setattr(view, k, self.va[k].ctypes.data)
        cols = RowCols(self.n_chr, *(self.ca[k].ctypes.data for k, _ in COL_KEYS))
        p = lambda a: a.ctypes.data if a.size else None   # noqa: E731
        o = self.out
        dev_out = DevOut(p(o["main_off"]), p(o["alt_off"]), p(o["all_path_off"]), p(o["all_elem_off"]), p(o["main"]), p(o["alt"]), p(o["all"]), None)
        return view, cols, X.sizes_of(o), dev_out, DevCuts(*(p(self.plans[k]) for k in LISTS))

    # -- what the rows must be, from the layout restated above
    def name_of(self, c):
        a = self.ca
        return a["names"][int(a["ctg_name_off"][c]):int(a["ctg_name_off"][c + 1])].tobytes().decode("latin-1")

    def chr_of(self, j):
        a = self.ca
        return a["names"][int(a["chr_name_off"][j]):int(a["chr_name_off"][j + 1])].tobytes().decode("latin-1")

    def tag_of(self, r):
        return self.va["cs_text"][int(self.va["rec_cs_off"][r]):int(self.va["rec_cs_off"][r + 1])].tobytes().decode("latin-1")

    def _owners_of(self):
        """{list: per element (contig, name)}: the .all names carry the path's number inside its contig."""
        o, C_ = self.out, int(self.out["n_contigs"])
        own = {}
        for k in ("main", "alt"):
            own[k] = [(c, self.name_of(c)) for c in range(C_) for _ in range(int(o[k + "_off"][c]), int(o[k + "_off"][c + 1]))]
        own["all"] = [(c, "%s.%d" % (self.name_of(c), p - int(o["all_path_off"][c]) + 1)) for c in range(C_)
                      for p in range(int(o["all_path_off"][c]), int(o["all_path_off"][c + 1])) for _ in range(int(o["all_elem_off"][p]), int(o["all_elem_off"][p + 1]))]
        return own

    def oracle_cut(self, k, i):
        """(tag, mat_num, aln_len) of cut element i of list k from the I/O oracle's get_edited_paf_data, the counts wrapped to
        int32 as the product's counters wrap (aasm_cut.h); the oracle raises where tag and coordinates do not agree."""
        if (k, i) not in self._oracle:
            va, e, (c, _) = self.va, self.out[k][i], self.owners()[k][i]
            r = int(va["ctg_rec_off"][c]) + int(e["ctg_index"])
            row = types.SimpleNamespace(qry_str=int(va["qry_str"][r]), qry_end=int(va["qry_end"][r]), aln_fwd=bool(va["aln_fwd"][r]), cs_string=self.tag_of(r),
                                        mat_num=int(self.ca["mat_num"][r]), aln_len=int(self.ca["aln_len"][r]))
            tag, mat, aln, cut = aasm_testlib.io_oracle().get_edited_paf_data(int(e["qs"]), int(e["qe"]), int(e["rs"]), int(e["re"]), row)
            assert cut
            self._oracle[(k, i)] = (tag, wrap32(mat), wrap32(aln))
        return self._oracle[(k, i)]

    def owners(self):
        if getattr(self, "_owners", None) is None:
            self._owners = self._owners_of()
        return self._owners

    def py_rows(self, which=None):
        """{list: [row bytes]} by py_row.  The tag of a cut element: render_cut on a regular plan, the I/O oracle's on an irregular
        one; in a consistent case (consistent_case) tag, mat_num and aln_len of every cut element are the oracle's, whatever the
        plan says.  which: {list: indices} (default: all)."""
        va, ca, own, rows = self.va, self.ca, self.owners(), {}
        for k in LISTS:
            rows[k] = {}
            for i in (range(len(self.out[k])) if which is None else which.get(k, ())):
                e, p, (c, name) = self.out[k][i], self.plans[k][i], own[k][i]
                r = int(va["ctg_rec_off"][c]) + int(e["ctg_index"])
                cut = bool(int(p["flags"]) & AASM_CUT_IS_CUT)
                mat, aln = (int(p["mat_num"]), int(p["aln_len"])) if cut else (int(ca["mat_num"][r]), int(ca["aln_len"][r]))
                if cut and self.consistent:
                    tag, mat, aln = self.oracle_cut(k, i)
                elif cut and int(p["flags"]) & AASM_CUT_IRREGULAR:
                    tag = self.oracle_cut(k, i)[0]
                else:
                    tag = render_cut(p, self.tag_of(r))
                rows[k][i] = py_row(name, int(va["qry_total"][r]), int(e["qs"]), int(e["qe"]), bool(va["aln_fwd"][r]), self.chr_of(int(va["ref_chr"][r])), int(ca["ref_total"][r]),
                                    int(e["rs"]), int(e["re"]), mat, aln, int(va["map_qul"][r]), bool(e["is_alt"]), int(ca["cord_type"][r]), int(ca["row_index"][r]), tag)
        return rows


def wrap32(v):
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def hand_case(contigs, chr_names, per_contig, plans=None):
    """contigs: [(name, [record, ...])], a record a dict {cs, fwd, qs, qe} with optional qtot, rtot, chr, mat, aln, mq, row_index, cord;
    per_contig: X.elements()' input; plans: {list: CUT_DT array} (default: every element uncut, the zero plan)."""
    recs = [r for _, rs in contigs for r in rs]
    tags = [r["cs"].encode("latin-1") for r in recs]
    g = lambda k, d: [r.get(k, d) for r in recs]   # noqa: E731
    names = [n.encode("latin-1") for n, _ in contigs] + [n.encode("latin-1") for n in chr_names]
    ends = np.concatenate([[0], np.cumsum([len(n) for n in names])]).astype(np.int64)
    va = {"ctg_rec_off": np.concatenate([[0], np.cumsum([len(rs) for _, rs in contigs])]), "qry_str": g("qs", 0), "qry_end": g("qe", 0), "qry_total": g("qtot", 1000),
          "ref_chr": g("chr", 0), "aln_fwd": [1 if r["fwd"] else 0 for r in recs], "map_qul": g("mq", 60),
          "rec_cs_off": np.concatenate([[0], np.cumsum([len(t) for t in tags])]), "cs_text": np.frombuffer(b"".join(tags), np.uint8)}
    ca = {"ref_total": g("rtot", 5000), "mat_num": g("mat", 7), "aln_len": g("aln", 9), "row_index": g("row_index", 0), "cord_type": g("cord", 0),
          "names": np.frombuffer(b"".join(names), np.uint8), "ctg_name_off": ends[:len(contigs) + 1], "chr_name_off": ends[len(contigs):]}
    out = X.elements(per_contig)
    if plans is None:
        plans = {k: np.zeros(len(out[k]), CUT_DT) for k in LISTS}
    return Case(va, ca, out, plans)


def cut_plan(keep_lo=0, keep_hi=0, head=0, tail=0, mat=0, aln=0, flags=AASM_CUT_IS_CUT):
    return (keep_lo, keep_hi, head, tail, mat, aln, flags, 0)


def paf_case(lib, paf, out, plans):
    """The case of a parsed container (device ranges: cs text in the view), a result over it and its plans."""
    view = paf.view()
    c, r = int(view.n_contigs), int(view.n_records)
    va = X.view_arrays(view)
    va.update(qry_total=_np_from(view.qry_total, r, np.int64), ref_chr=_np_from(view.ref_chr, r, np.int32), map_qul=_np_from(view.map_qul, r, np.uint8))
    keep, cols = C.c_void_p(), RowCols()
    assert lib.emw_row_cols(paf._h, C.c_int64(0), C.c_int64(c), C.byref(keep), C.byref(cols)) == 0
    try:
        ca = {"ctg_name_off": _np_from(cols.ctg_name_off, c + 1, np.int64), "chr_name_off": _np_from(cols.chr_name_off, int(cols.n_chr) + 1, np.int64)}
        ca["names"] = _np_from(cols.names, int(ca["chr_name_off"][-1]), np.uint8)
        for k, dt in COL_KEYS[:5]:
            ca[k] = _np_from(getattr(cols, k), r, dt)
    finally:
        lib.emw_row_cols_free(keep)
    return Case(va, ca, out, plans)


# ---- the emulation ------------------------------------------------------------------------------------------------------------------
def emul_sizes(lib, case, max_blocks=0):
    """emw_rows_sizes -> (rc, info, {list: row_off array}); the offsets start as 0x5a bytes."""
    view, cols, sz, dev_out, dc = case.host_structs()
    off = {k: np.frombuffer(b"\x5a" * (8 * (n + 1)), np.int64).copy() for k, n in case.n.items()}
    info = RowsInfo()
    rc = lib.emw_rows_sizes(C.byref(view), C.byref(cols), C.byref(sz), C.byref(dev_out), C.byref(dc), C.byref(DevRows(*(off[k].ctypes.data for k in LISTS))),
                            C.c_int64(max_blocks), C.byref(info))
    return rc, info, off


def emul_format(lib, case, info, off, lst, e0, e1, max_blocks=0, pad=64):
    """emw_rows_format of rows [e0, e1) of list lst -> (rc, the bytes); the buffer has `pad` guard bytes on both sides, which must
    come back untouched."""
    view, cols, sz, dev_out, dc = case.host_structs()
    o = off[LISTS[lst]] if 0 <= lst < 3 else []
    ok = 0 <= e0 <= e1 < len(o)
    nb = int(o[e1] - o[e0]) if ok else 0
    buf = np.full(nb + 2 * pad, 0xEE, np.uint8)
    rc = lib.emw_rows_format(C.byref(view), C.byref(cols), C.byref(sz), C.byref(dev_out), C.byref(dc), C.byref(DevRows(*(off[k].ctypes.data for k in LISTS))),
                             C.byref(info), int(lst), C.c_int64(e0), C.c_int64(e1), C.c_void_p(buf.ctypes.data + pad), C.c_int64(max_blocks))
    assert (buf[:pad] == 0xEE).all() and (buf[pad + nb:] == 0xEE).all(), "bytes outside the range's text were written"
    return rc, buf[pad:pad + nb].tobytes()


def emul_texts(lib, case, max_blocks=0):
    """Sizes + the three lists formatted whole -> (info, offsets, [main, alt, all] bytes); the result must have no flagged element."""
    rc, info, off = emul_sizes(lib, case, max_blocks)
    assert rc == 0 and info.n_flagged == 0, (rc, info.n_flagged, info.bad_list, info.bad_elem, hex(info.bad_flags))
    texts = []
    for l, k in enumerate(LISTS):
        rc, t = emul_format(lib, case, info, off, l, 0, case.n[k], max_blocks)
        assert rc == 0 and len(t) == info.bytes[l]
        texts.append(t)
    return info, off, texts


def check_offsets(off, texts):
    """row_off are the prefix sums of the rows' lengths: every row of a text ends with its only line feed."""
    for k, t in zip(LISTS, texts):
        ends = np.flatnonzero(np.frombuffer(t, np.uint8) == 10) + 1
        assert off[k][0] == 0 and np.array_equal(off[k][1:], ends), k


def emul_cut_pieces(lib, off, limit, lst=1):
    """rows_cut_pieces on the offsets `off` (n + 1 of them) -> (pieces as an [m, 5] array of list, e0, e1, b0, b1, its fetches as
    an [f, 3] array of first, stride, count)."""
    off = np.ascontiguousarray(off, np.int64)
    n = len(off) - 1
    out = np.full((n + 1, 5), -7, np.int64)
    m = lib.emw_cut_pieces(C.c_void_p(off.ctypes.data), C.c_int64(n), C.c_int64(int(off[-1])), int(lst), C.c_int64(int(limit)), C.c_void_p(out.ctypes.data), C.c_int64(n + 1))
    assert 0 <= m <= n, m
    calls = np.zeros((n // SAMPLE + 3, 3), np.int64)
    f = lib.emw_cut_fetches(C.c_void_p(calls.ctypes.data), C.c_int64(len(calls)))
    assert 0 <= f <= len(calls), f
    return out[:m], calls[:f]


def check_pieces(off, limit, pieces, calls, lst=1):
    """The piece cutter's contract on offsets `off` (numpy, n + 1 of them) -> (pieces made of whole sample blocks, pieces inside
    a block whose rows were fetched)."""
    n, total = len(off) - 1, int(off[-1])
    if n == 0:
        assert len(pieces) == 0 and len(calls) == 0
        return 0, 0
    starts = list(range(0, n, SAMPLE))
    block_bytes = {s: int(off[min(n, s + SAMPLE)] - off[s]) for s in starts}
    assert len(pieces) >= 1 and pieces[0][1] == 0 and pieces[-1][2] == n
    for a, b in zip(pieces[:-1], pieces[1:]):
        assert a[2] == b[1], "gap or overlap"
    for l, e0, e1, b0, b1 in pieces.tolist():
        assert l == lst and 0 <= e0 < e1 <= n and b0 == off[e0] and b1 == off[e1]
        assert b1 - b0 <= limit or e1 - e0 == 1, (e0, e1, b1 - b0, limit)
    if limit >= total:
        assert len(pieces) == 1
    if all(v <= limit for v in block_bytes.values()):
        assert all(int(p[1]) % SAMPLE == 0 for p in pieces)
    # the fetches: the samples once, then the rows of every block that does not fit (and holds more than one row), once each
    assert calls[0].tolist() == [0, SAMPLE, n // SAMPLE + 1]
    fine = [s for s in starts if block_bytes[s] > limit and min(n, s + SAMPLE) - s > 1]
    assert calls[1:].tolist() == [[s, 1, min(n, s + SAMPLE) - s + 1] for s in fine], (calls[1:].tolist(), fine)
    inside = sum(1 for p in pieces.tolist() if any(s <= p[1] and p[2] <= min(n, s + SAMPLE) for s in fine))
    return len(pieces) - inside, inside


# ---- the sanitizer program --------------------------------------------------------------------------------------------------------------
def san_input(case):
    """rows_emul_san's input file (tests/host_emul/rows_emul.cpp)."""
    va, ca, o = case.va, case.ca, case.out
    w8 = lambda b: b + b"\0" * (-len(b) % 8)   # noqa: E731
    i64 = lambda a: np.ascontiguousarray(a, np.int64).tobytes()   # noqa: E731
    names, text = ca["names"][:int(ca["chr_name_off"][-1])].tobytes(), va["cs_text"][:int(va["rec_cs_off"][-1])].tobytes()
    hdr = [len(va["ctg_rec_off"]) - 1, len(va["qry_str"]), case.n_chr, len(o["main"]), len(o["alt"]), len(o["all_elem_off"]) - 1, len(o["all"]), len(names), len(text)]
    parts = [i64(hdr), i64(va["qry_total"]), i64(va["qry_str"]), i64(va["qry_end"]), i64(ca["ref_total"]), i64(va["rec_cs_off"]), i64(va["ctg_rec_off"]),
             i64(ca["ctg_name_off"]), i64(ca["chr_name_off"]), i64(o["main_off"]), i64(o["alt_off"]), i64(o["all_path_off"]), i64(o["all_elem_off"])]
    parts += [np.ascontiguousarray(o[k], OUT_ELEM_DTYPE).tobytes() for k in LISTS] + [case.plans[k].tobytes() for k in LISTS]
    parts += [w8(np.ascontiguousarray(a, np.int32).tobytes()) for a in (va["ref_chr"], ca["mat_num"], ca["aln_len"], ca["row_index"])]
    parts += [w8(va["aln_fwd"].tobytes() + va["map_qul"].tobytes() + ca["cord_type"].tobytes()), w8(names), w8(text)]
    return b"".join(parts)


def run_san(san, case, d, stem):
    """-> the three lists' text, back to back; the program must end with 0 (the sanitizer ends it otherwise)."""
    src, dst = os.path.join(str(d), stem + ".in"), os.path.join(str(d), stem + ".out")
    with open(src, "wb") as f:
        f.write(san_input(case))
    r = subprocess.run([san, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return open(dst, "rb").read()


# ---- the product's entries on device tensors ----------------------------------------------------------------------------------------
class DeviceCase:
    """A Case uploaded through torch: the C structures over device tensors (kept alive here)."""

    def __init__(self, case, device=0):
        import torch
        self.case, self.device = case, device
        dev = torch.device("cuda", device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)   # noqa: E731
        self.t = {"va": {k: up(v) for k, v in case.va.items()}, "ca": {k: up(v) for k, v in case.ca.items()},
                  "out": {k: up(case.out[k]) for k in ("main_off", "alt_off", "all_path_off", "all_elem_off") + LISTS}, "plans": {k: up(case.plans[k]) for k in LISTS}}
        p = lambda x: x.data_ptr() if x.numel() else None   # noqa: E731
        self.view = BatchIn()
        self.view.n_contigs, self.view.n_records = len(case.va["ctg_rec_off"]) - 1, len(case.va["qry_str"])
        for k, _ in IN_KEYS:
            setattr(self.view, k, p(self.t["va"][k]))
        self.cols = RowCols(case.n_chr, *(p(self.t["ca"][k]) for k, _ in COL_KEYS))
        o = self.t["out"]
        self.dev_out = DevOut(p(o["main_off"]), p(o["alt_off"]), p(o["all_path_off"]), p(o["all_elem_off"]), p(o["main"]), p(o["alt"]), p(o["all"]), None)
        self.cuts = DevCuts(*(p(self.t["plans"][k]) for k in LISTS))
        self.sz = X.sizes_of(case.out)
        self.off = {k: torch.full((n + 1,), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device=dev) for k, n in case.n.items()}
        self.ro = DevRows(*(self.off[k].data_ptr() for k in LISTS))
        self.info = RowsInfo()

    def sizes(self, api, flags=0, stream=0):
        return api.rows_sizes_raw(self.view, self.cols, self.sz, self.dev_out, self.cuts, self.ro, self.info, flags, self.device, stream)

    def format(self, api, lst, e0, e1, flags=0, pad=64, stream=0, on=None):
        """-> (rc, bytes): rows [e0, e1) of list lst; pad guard bytes on both sides must come back untouched.
        on: a torch stream - the buffer's 0xEE fill is enqueued on it right before the format call on the same stream, with no
        synchronize in between (a fill that overtakes the kernel shows as 0xEE bytes in the text)."""
        import torch
        o = self.off[LISTS[lst]] if 0 <= lst < 3 else None
        ok = o is not None and 0 <= e0 <= e1 < o.numel()
        nb = int((o[e1] - o[e0]).item()) if ok else 0
        dev = torch.device("cuda", self.device)
        if on is not None:
            with torch.cuda.stream(on):
                buf = torch.full((nb + 2 * pad,), 0xEE, dtype=torch.uint8, device=dev)
            rc = api.rows_format_raw(self.view, self.cols, self.sz, self.dev_out, self.cuts, self.ro, self.info, lst, e0, e1, buf.data_ptr() + pad, flags, self.device, on.cuda_stream)
            with torch.cuda.stream(on):
                h = buf.cpu().numpy()
        else:
            buf = torch.full((nb + 2 * pad,), 0xEE, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(self.device)
            rc = api.rows_format_raw(self.view, self.cols, self.sz, self.dev_out, self.cuts, self.ro, self.info, lst, e0, e1, buf.data_ptr() + pad, flags, self.device, stream)
            torch.cuda.synchronize(self.device)
            h = buf.cpu().numpy()
        assert (h[:pad] == 0xEE).all() and (h[pad + nb:] == 0xEE).all(), "bytes outside the range's text were written"
        return rc, h[pad:pad + nb].tobytes()

    def texts(self, api, flags=0):
        rc = self.sizes(api, flags)
        assert rc == 0 and self.info.n_flagged == 0, (rc, api.LIB.aasm_last_error(), self.info.n_flagged, self.info.bad_list, self.info.bad_elem, hex(self.info.bad_flags))
        out = []
        for l, k in enumerate(LISTS):
            rc, t = self.format(api, l, 0, self.case.n[k], flags)
            assert rc == 0 and len(t) == self.info.bytes[l], (rc, api.LIB.aasm_last_error())
            out.append(t)
        return out

    def offsets(self):
        return {k: v.cpu().numpy() for k, v in self.off.items()}


# ---- hand-made cases shared by both tiers -------------------------------------------------------------------------------------------
TAG = "cs:Z::6*ag:4+tt:3-c:12*ct:9"                                   # 27 bytes; operations start at 5, 7, 10, 12, 15, 17, 19, 22, 25


def alignment_case():
    """One list whose contig names have lengths 1 .. 17, so consecutive rows start at every offset mod 16, crossed with stretches of
    0, 1, 7, 8, 9, 15, 16, 17, 31 and 33 bytes and head / tail present or absent; reference names of 1 and of 300 bytes."""
    long_tag = "cs:Z:" + ":7" * 40
    contigs, per, plans = [], [], []
    for ln in range(1, 18):
        contigs.append(("n" * ln, [{"cs": long_tag, "fwd": ln % 2 == 0, "qs": 10, "qe": 289, "chr": ln % 2, "mat": ln, "aln": ln + 1}]))
        els = []
        for j, st in enumerate((0, 1, 7, 8, 9, 15, 16, 17, 31, 33)):
            for hd, tl in ((0, 0), (5, 0), (0, 123), (1234567, 3)):
                lo = 5 + 2 * ((ln + j) % 3)
                els.append((11 + j, 280 - j, 100, 400, 0))
                plans.append(cut_plan(lo, lo + st, hd, tl, 100 + j, 200 + j))
        per.append({"main": els})
    return hand_case(contigs, ["c", "R" * 300], per, {"main": np.array(plans, CUT_DT), "alt": np.zeros(0, CUT_DT), "all": np.zeros(0, CUT_DT)})


def long_case():
    """read_cases' 1 MiB tag and its 70 000-operation tag, each once uncut and once cut in the middle."""
    import read_cases as RC
    big, many = "cs:Z:" + RC.long_tag(1 << 20).decode(), "cs:Z:" + ":1*ac" * 70000
    contigs = [("big", [{"cs": big, "fwd": True, "qs": 0, "qe": 10 ** 7}]), ("many", [{"cs": many, "fwd": False, "qs": 5, "qe": 10 ** 7}])]
    per = [{"main": [(0, 10 ** 7, 1, 2, 0), (7, 9999, 1, 2, 0)]}, {"main": [(5, 10 ** 7, 3, 4, 0)], "alt": [(6, 10 ** 6, 3, 4, 0)]}]
    mid = lambda t: (len(t) // 3, 2 * len(t) // 3)   # noqa: E731
    plans = {"main": np.array([cut_plan(flags=0), cut_plan(*mid(big), 3, 4, 5, 6), cut_plan(flags=0)], CUT_DT),
             "alt": np.array([cut_plan(*mid(many), 0, 9, 1, 2)], CUT_DT), "all": np.zeros(0, CUT_DT)}
    return hand_case(contigs, ["chrL"], per, plans)


def sized_case(n_main, n_alt=0, n_all=0):
    """Lists of exactly these sizes over contigs of 3 records (24 of them or more): the contig pattern of the cut-plan tests scaled
    to the fill chunk (contigs without elements at chunk edges), every third element cut."""
    pat = (1, 0, CHUNK - 2, 1, 0, 0, 1, CHUNK - 1, 0, 1)
    paths = X._split(n_all, (0, 1, 100, CHUNK - 101, 0, 0, 1, 90, CHUNK - 91, 0, 1))
    nc = max(24, len(X._split(n_main, pat)) + 2, len(X._split(n_alt, pat)) + 3, 3 * len(paths) // 4 + 4)
    contigs = [("ctg%d" % c, [{"cs": TAG, "fwd": (c + i) % 2 == 0, "qs": 100, "qe": 134, "chr": i % 2, "row_index": 3 * c + i, "cord": i % 2} for i in range(3)]) for c in range(nc)]
    stretches = ((5, 7), (7, 15), (10, 27), (5, 5), (12, 25))
    plans, per = {k: [] for k in LISTS}, [{"main": [], "alt": [], "all": []} for _ in range(nc)]

    def element(k, i):
        if i % 3 == 2:
            plans[k].append(cut_plan(*stretches[i % 5], i % 4, (i // 4) % 3, i, 2 * i))
            return (101 + i % 5, 133, 7, 40, i % 3)
        plans[k].append(cut_plan(flags=0))
        return (100, 134, 7, 41, i % 3)
    for k, n in (("main", n_main), ("alt", n_alt)):
        i = 0
        for c, m in enumerate(X._split(n, pat)):
            per[c + (1 if k == "alt" else 0)][k] = [element(k, i + j) for j in range(m)]
            i += m
    c, i = 0, 0
    for p in range(0, len(paths), 2):
        if c % 3 == 2:
            c += 1
        per[c]["all"] = []
        for m in paths[p:p + 2]:
            per[c]["all"].append([element("all", i + j) for j in range(m)])
            i += m
        c += 1
    assert c <= nc
    return hand_case(contigs, ["chrA", "chromosome_B"], per, {k: np.array(v, CUT_DT) if v else np.zeros(0, CUT_DT) for k, v in plans.items()})


# ---- consistent hand cases: tags, coordinates and cuts that the I/O oracle accepts ------------------------------------------------------
def cs_ops(tag):
    return re.findall(r":[0-9]+|\*[a-z][a-z]|[+-][a-z]+", tag[5:])


def cs_spans(ops):
    """(query bases, reference bases) a tag's operations consume."""
    q = r = 0
    for op in ops:
        n = int(op[1:]) if op[0] == ":" else 1 if op[0] == "*" else len(op) - 1
        q += n if op[0] != "-" else 0
        r += n if op[0] != "+" else 0
    return q, r


def consistent_case(contigs, chr_names, per_contig):
    """hand_case for records whose tag consumes exactly [qs, qe] (qe follows from the tag; `rs`: the reference start, default 1000)
    and elements (ctg_index, a, b): the record without its first a and its last b query bases, both ends inside the ':' runs at
    the tag's ends, so the reference coordinates follow from the query cut.  The case's expectation is the I/O oracle's on every
    cut element (Case.py_rows); case.irregular[list][i]: whether the plan must be AASM_CUT_IRREGULAR, from the tag alone - a ':'
    run that is kept whole is written with a leading zero.  The plans are the zero plans until consistent_plans() sets them."""
    contigs = [(name, [dict(r) for r in recs]) for name, recs in contigs]
    info = []
    for _, recs in contigs:
        for r in recs:
            ops = cs_ops(r["cs"])
            assert "cs:Z:" + "".join(ops) == r["cs"] and ops[0][0] == ":" and ops[-1][0] == ":"
            q, rb = cs_spans(ops)
            r["qe"] = r["qs"] + q - 1
            info.append((ops, rb))
    first = np.concatenate([[0], np.cumsum([len(recs) for _, recs in contigs])])
    irregular = {k: [] for k in LISTS}

    def element(c, k, el):
        ci, a, b = el
        rec = contigs[c][1][ci]
        ops, rb = info[int(first[c]) + ci]
        rs0 = rec.get("rs", 1000)
        lo, hi = (a, b) if rec["fwd"] else (b, a)                  # bases taken from the tag's first / last run
        n_lo, n_hi = int(ops[0][1:]), int(ops[-1][1:])
        assert 0 <= lo and 0 <= hi and (lo < n_lo and hi < n_hi if len(ops) > 1 else lo + hi < n_lo), (c, el)
        whole = ops[(1 if lo else 0):len(ops) - (1 if hi else 0)] if len(ops) > 1 else ([] if lo or hi else ops)
        irregular[k].append(bool(a or b) and any(op[0] == ":" and op[1] == "0" for op in whole))
        ers, ere = (rs0 + a, rs0 + rb - 1 - b) if rec["fwd"] else (rs0 + rb - 1 - a, rs0 + b)
        return (rec["qs"] + a, rec["qe"] - b, ers, ere, ci)
    per = []
    for c, lists in enumerate(per_contig):
        per.append({k: [element(c, k, el) for el in lists.get(k, ())] for k in ("main", "alt")})
    for c, lists in enumerate(per_contig):                           # (.all after main and alt: the order of X.elements()' lists)
        per[c]["all"] = [[element(c, "all", el) for el in path] for path in lists.get("all", ())]
    case = hand_case(contigs, chr_names, per)
    case.consistent, case.irregular = True, {k: np.array(v, bool) for k, v in irregular.items()}
    return case


def check_consistent_plans(case, plans):
    """Plans of a consistent case (from the cut-plan kernel) against the oracle and the builder: an uncut element has the zero
    plan; a cut one the flags IS_CUT [| IRREGULAR] exactly, and the oracle's counts."""
    for k in LISTS:
        assert len(plans[k]) == len(case.out[k]) == len(case.irregular[k]), k
        va, own = case.va, case.owners()[k]
        for i, (e, p) in enumerate(zip(case.out[k], plans[k])):
            r = int(va["ctg_rec_off"][own[i][0]]) + int(e["ctg_index"])
            if int(e["qs"]) == int(va["qry_str"][r]) and int(e["qe"]) == int(va["qry_end"][r]):
                assert p.tobytes() == b"\0" * 48 and not case.irregular[k][i], (k, i)
                continue
            _, mat, aln = case.oracle_cut(k, i)
            want = AASM_CUT_IS_CUT | (AASM_CUT_IRREGULAR if case.irregular[k][i] else 0)
            assert (int(p["flags"]), int(p["mat_num"]), int(p["aln_len"])) == (want, mat, aln), (k, i, p, want, mat, aln)


def consistent_plans(emc, case):
    """The emulated cut-plan kernel's plans of a consistent case, checked (check_consistent_plans) and set as the case's."""
    plans = X.emul_plans(emc, case.host_structs()[0], case.out)
    check_consistent_plans(case, plans)
    case.plans, case._joined = {k: np.ascontiguousarray(plans[k], CUT_DT) for k in LISTS}, None
    return case


def irregular_tag(i):
    """":20" mid ":00" 10^(i % 19) "*ct:30": mid holds i % 9 runs with a leading zero, each before a substitution, an insertion or
    a deletion; the long run prints with 1 .. 19 digits (above 2^31 the counters wrap: wrap32)."""
    mid = "".join(":0%d" % (1 + (i + j) % 12) + ("*ac", "+gt", "-a")[j % 3] for j in range(i % 9))
    return "cs:Z::20" + mid + ":00" + str(10 ** (i % 19)) + "*ct:30"


def irregular_alignment_case(n=3 * CHUNK + 1):
    """One list of n rows, every one irregular: both strands alternating, contig names of 1 .. 17 bytes, irregular_tag(i) cut by
    1 + i % 19 bases at one end and 2 + i % 17 at the other.  mat_num and aln_len are the oracle's Python ints wrapped to int32."""
    contigs = [("n" * (1 + i % 17), [{"cs": irregular_tag(i), "fwd": i % 2 == 0, "qs": 5 + i, "mq": i % 256, "row_index": i}]) for i in range(n)]
    case = consistent_case(contigs, ["chrA"], [{"main": [(0, 1 + i % 19, 2 + i % 17)]} for i in range(n)])
    assert case.irregular["main"].all()
    return case


def irregular_stats(rows):
    """Of expected rows (bytes, in list order) with a re-cut tag: the text offsets mod 8 at which the tags' bodies start, the
    bodies' lengths mod 8, and the digit counts of their runs."""
    at, lens, digits, o = set(), set(), set(), 0
    for row in rows:
        j = row.index(b"\tcs:Z:") + 6
        at.add((o + j) % 8); lens.add((len(row) - 1 - j) % 8)
        digits.update(len(m) for m in re.findall(rb":([0-9]+)", row[j:]))
        o += len(row)
    return at, lens, digits


REG_TAG, IRR_TAG = "cs:Z::20*ag:4+tt:3-c:12*ct:30", "cs:Z::20*ag:04+tt:3-c:012*ct:30"


def kinds_case(kinds, all_paths=None):
    """A consistent case from {list: "UIR.." per row}: U an uncut element, R a cut with a regular plan (REG_TAG), I a cut with an
    irregular one (IRR_TAG, both strands).  Every contig has the same three records; main and alt rows are dealt over the contigs
    by sized_case's pattern, .all rows over all_paths: per contig the sizes of its paths (default: two paths per contig)."""
    pat = (1, 0, CHUNK - 2, 1, 0, 0, 1, CHUNK - 1, 0, 1)
    split = {k: X._split(len(kinds.get(k, "")), pat) for k in ("main", "alt")}
    if all_paths is None:
        sizes = X._split(len(kinds.get("all", "")), (0, 1, 100, CHUNK - 101, 0, 0, 1, 90, CHUNK - 91, 0, 1))
        all_paths = [sizes[p:p + 2] for p in range(0, len(sizes), 2)]
    assert sum(sum(p) for p in all_paths) == len(kinds.get("all", ""))
    nc = max(3, len(split["main"]) + 1, len(split["alt"]) + 2, len(all_paths) + 1)
    contigs = [("k%d" % c, [{"cs": REG_TAG, "fwd": c % 2 == 0, "qs": 100 + c, "chr": c % 2, "row_index": 3 * c}, {"cs": IRR_TAG, "fwd": True, "qs": 7, "row_index": 3 * c + 1, "cord": 1},
                            {"cs": IRR_TAG, "fwd": False, "qs": 10 ** 12, "rs": 5, "row_index": 3 * c + 2}]) for c in range(nc)]

    def element(kind, i):
        return {"U": (i % 3, 0, 0), "R": (0, i % 4, 1 + i % 5), "I": (1 + i % 2, 1 + i % 6, i % 5)}[kind]
    per = [{"main": [], "alt": [], "all": []} for _ in range(nc)]
    for k in ("main", "alt"):
        i = 0
        for c, m in enumerate(split[k]):
            per[c + (1 if k == "alt" else 0)][k] = [element(kinds[k][i + j], i + j) for j in range(m)]
            i += m
    i = 0
    for c, paths in enumerate(all_paths):
        for m in paths:
            per[c]["all"].append([element(kinds["all"][i + j], i + j) for j in range(m)])
            i += m
    case = consistent_case(contigs, ["chrA", "chromosome_B"], per)
    for k in LISTS:
        assert "".join("I" if x else "-" for x in case.irregular[k]) == "".join(x if x == "I" else "-" for x in kinds.get(k, "")), k
    return case


MIXED_N = 3 * CHUNK + 5
MIXED_PATHS = [[1 + (p + 1) % 3 for p in range(101)]]                   # contig 0: 101 paths (.1, .10 and .100 hold two elements each)


def mixed_kinds():
    """{list: kinds} of irregular_mixed_case: MIXED_N rows per list.  Irregular: the first and the last row of the list, rows
    CHUNK - 1, CHUNK and 2 CHUNK - 1, in .all both rows of the paths .1, .10 and .100, and every seventh row elsewhere - except in
    chunk 2, which holds none.  The rows beside those edges are uncut, regular and irregular ones."""
    out = {}
    for k in LISTS:
        kind = ["UR"[i % 2] if i // CHUNK == 2 else "URUIRUR"[i % 7] for i in range(MIXED_N)]
        for i, x in ((0, "I"), (1, "U"), (CHUNK - 2, "R"), (CHUNK - 1, "I"), (CHUNK, "I"), (CHUNK + 1, "I"), (2 * CHUNK - 2, "U"), (2 * CHUNK - 1, "I"),
                     (2 * CHUNK, "R"), (MIXED_N - 2, "I"), (MIXED_N - 1, "I")):
            kind[i] = x
        if k == "all":
            ends = np.concatenate([[0], np.cumsum(MIXED_PATHS[0])])
            for p in (0, 9, 99):
                assert ends[p + 1] - ends[p] == 2 and ends[p + 1] < 2 * CHUNK
                kind[int(ends[p])] = kind[int(ends[p]) + 1] = "I"
        out[k] = "".join(kind)
    return out


def irregular_mixed_case():
    kinds = mixed_kinds()
    rest = X._split(MIXED_N - sum(MIXED_PATHS[0]), (0, 60, CHUNK - 3, 1, 0, 70))
    return kinds_case(kinds, MIXED_PATHS + [[]] + [rest[p:p + 2] for p in range(0, len(rest), 2)])


LONG_UNIT = ":01*ac"


def long_irregular_case():
    """"cs:Z::5" + ":01*ac" * 70 000 + ":5" cut on both strands, and a tag of about 1 MiB built the same way: every ":01" comes out
    as ":1", so a rendered tag is shorter than its source by the number of its units.  Each long row has short rows (uncut, regular)
    before and behind it in its chunk."""
    many, mib = "cs:Z::5" + LONG_UNIT * 70000 + ":5", "cs:Z::5" + LONG_UNIT * ((1 << 20) // len(LONG_UNIT)) + ":5"
    contigs = [("s", [{"cs": REG_TAG, "fwd": True, "qs": 100}]), ("many", [{"cs": many, "fwd": True, "qs": 0}, {"cs": many, "fwd": False, "qs": 7}]),
               ("t", [{"cs": REG_TAG, "fwd": False, "qs": 50}]), ("mib", [{"cs": mib, "fwd": False, "qs": 3}]), ("u", [{"cs": REG_TAG, "fwd": True, "qs": 9}])]
    per = [{"main": [(0, 0, 0), (0, 3, 1)], "alt": [(0, 2, 2)]}, {"main": [(0, 2, 2)], "alt": [(1, 3, 1)], "all": [[(1, 4, 4)]]}, {"main": [(0, 1, 0)], "alt": [(0, 0, 0)], "all": [[(0, 0, 5)]]},
           {"main": [(0, 1, 3)]}, {"main": [(0, 0, 0), (0, 5, 5)], "all": [[(0, 0, 0)], [(0, 1, 1)]]}]
    case = consistent_case(contigs, ["chrL"], per)
    assert case.irregular["main"].tolist() == [False, False, True, False, True, False, False] and case.irregular["alt"].tolist() == [False, True, False]
    return case


def joined_py(case):
    if case.consistent and getattr(case, "_joined", None):           # (a consistent case is not edited once it has its plans)
        return list(case._joined)
    rows = case.py_rows()
    out = [b"".join(rows[k][i] for i in range(len(case.out[k]))) for k in LISTS]
    if case.consistent:
        case._joined = list(out)
    return out


def oracle_checked_irregular(T, exp, plans):
    """Plans of a text_fuzz run the oracle accepts against the I/O oracle alone (exp: text_fuzz.expected()): cut or not, the
    counts, and on a regular plan the rendered tag -> {list: indices of the irregular plans}."""
    io, sol, st, out = T.io_oracle(), exp.sol, exp.st, {}
    paths = [c for c in range(sol["n_contigs"]) for _ in range(int(sol["all_path_off"][c]), int(sol["all_path_off"][c + 1]))]
    owner = {"main": np.repeat(np.arange(sol["n_contigs"]), np.diff(sol["main_off"])), "alt": np.repeat(np.arange(sol["n_contigs"]), np.diff(sol["alt_off"])),
             "all": np.repeat(np.array(paths, np.int64), np.diff(sol["all_elem_off"]))}
    for k in LISTS:
        assert len(plans[k]) == len(sol[k]) == len(owner[k]), k
        out[k] = []
        for i, (e, p) in enumerate(zip(sol[k], plans[k])):
            row = st.paf_data[int(owner[k][i])][int(e["ctg_index"])]
            tag, mat, aln, cut = io.get_edited_paf_data(int(e["qs"]), int(e["qe"]), int(e["rs"]), int(e["re"]), row)
            f = int(p["flags"])
            assert f & ~AASM_CUT_IRREGULAR == (AASM_CUT_IS_CUT if cut else 0), (k, i, f)
            if cut:
                assert (int(p["mat_num"]), int(p["aln_len"])) == (wrap32(mat), wrap32(aln)), (k, i)
                if f & AASM_CUT_IRREGULAR:
                    out[k].append(i)
                else:
                    assert render_cut(p, row.cs_string) == tag, (k, i)
    return out
