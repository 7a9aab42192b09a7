"""Helpers of the tests of the --alt merge on the device (tests/test_alt_device_cpu.py, tests/test_gpu_alt_device.py): the host
route that is the yardstick, the emulated merge, the I/O oracle's independent reading, the comparisons."""
import ctypes as C

import numpy as np

import aasm_testlib
import read_cols_testlib as XR
import read_testlib as X
from alignasm_amd._abi import BatchIn, RowCols

def _declare(lib):
    lib.emalt_merge.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_double, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emalt_free.argtypes = [C.c_void_p]
    lib.emalt_host_cols.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emalt_host_cols_free.argtypes = [C.c_void_p]
    lib.emalt_counter.restype = C.c_int64
    lib.aasm_last_error.restype = C.c_char_p


def build_emul(san=False):
    """tests/host_emul/alt_emul.cpp -> its library, or with san (library, path of alt_emul_san)."""
    return aasm_testlib.build_emul("alt", san, _declare)


def host_cols(lib, paf):
    """rows_host_cols (aasm_rows.h) of a container, what aasm_paf_upload_rows(0, C) uploads, through the emulation library."""
    view = paf.view()
    keep, cols = C.c_void_p(), RowCols()
    assert lib.emalt_host_cols(paf._h, C.byref(keep), C.byref(cols)) == 0
    try:
        return XR.cols_arrays(cols, int(view.n_contigs), int(view.n_records))
    finally:
        lib.emalt_host_cols_free(keep)


def emul_cols(lib):
    """cols_of for the CPU tier: the container's row columns through the emulation library."""
    return lambda paf: host_cols(lib, paf)


def uploaded_cols(api):
    """cols_of for the GPU tier: aasm_paf_upload_rows(0, C) on the container, fetched back."""
    fetch = X.hip_fetcher(api)
    return lambda paf: XR.uploaded_cols(api, paf, fetch)


def host_batch(api, cols_of, main):
    """The main file as the host reader leaves it: {"view", "cols"} and the container."""
    paf = api.Paf.parse(main, device_ranges=True)
    return {"view": X.view_arrays(paf.view()), "cols": cols_of(paf)}, paf


def host_route(api, cols_of, case):
    """The yardstick: parse(main, device ranges) -> merge_alt_mem(alt, baseline) -> batch + row columns (cols_of(container)).
    -> (main arrays, merged arrays); raises AlignasmError where the host finds the alt text bad."""
    before, paf = host_batch(api, cols_of, case["main"])
    paf.merge_alt(case["alt"], case["baseline"])
    return before, {"view": X.view_arrays(paf.view()), "cols": cols_of(paf)}


def host_verdict(api, cols_of, case):
    """(code, message) of the host route on a text it finds bad, or None."""
    try:
        host_route(api, cols_of, case)
    except api.AlignasmError as e:
        return e.code, str(e).split(": ", 1)[1]
    return None


def expected_decline(api, cols_of, case):
    """(code, message) a declined case must give: the host's where it names a fault, else the device's own (case["says"])."""
    v = host_verdict(api, cols_of, case)
    assert (v is None) == (case["says"] is not None), (case["name"], v)
    return v if v is not None else (-7, case["says"])


def diff(want, got):
    return [f"view.{k}" for k in X.diff_views(want["view"], got["view"])] + [f"cols.{k}" for k in XR.diff_cols(want["cols"], got["cols"])]


def emul_merge(lib, api, case, flags=0, max_blocks=0):
    """emalt_merge on the host reader's container of the main file -> (code, message, merged arrays or None)."""
    paf = api.Paf.parse(case["main"], device_ranges=True)
    up, view, cols, nb = C.c_void_p(), BatchIn(), RowCols(), C.c_int64(-1)
    rc = lib.emalt_merge(paf._h, case["alt"], len(case["alt"]), case["baseline"], flags, max_blocks, C.byref(up), C.byref(view), C.byref(cols), C.byref(nb))
    if rc != 0:
        assert not up
        return rc, (lib.aasm_last_error() or b"").decode(), None
    try:
        va = X.view_arrays(view)
        ca = XR.cols_arrays(cols, va["n_contigs"], va["n_records"])
        assert nb.value == len(ca["names"])
    finally:
        lib.emalt_free(up)
    return 0, "", {"view": va, "cols": ca}


def check_against_oracle(T, case, got):
    """oracle/paf_io_oracle.py's merge_alt on its own reading of both texts against a merged batch: the solver's arrays, the tags,
    the alt rows' labels and every record's reference name."""
    io = T.io_oracle()
    st = io.read_paf(case["main"])
    io.merge_alt(st, case["alt"], case["baseline"])
    want = {k: np.asarray(v, np.int64) for k, v in io.to_arrays(st).items()}
    for k in ("ctg_rec_off", "qry_str", "qry_end", "ref_str", "ref_end", "qry_total", "ref_chr", "aln_fwd", "map_qul", "rec_rng_off"):
        assert np.array_equal(want[k], got["view"][k].astype(np.int64)), k
    recs = [r for ctg in st.paf_data for r in ctg]
    tags = [r.cs_string.encode() for r in recs]
    assert got["view"]["cs_text"].tobytes() == b"".join(tags)
    assert [(int(t), int(i)) for t, i in zip(got["cols"]["cord_type"], got["cols"]["row_index"])] == [tuple(r.cord) for r in recs]
    names, off, C_ = got["cols"]["names"].tobytes(), got["cols"]["chr_name_off"], got["view"]["n_contigs"]
    chr_names = [names[int(off[j]):int(off[j + 1])].decode() for j in range(len(off) - 1)]
    assert chr_names == [st.chr_rev[j] for j in range(len(st.chr_rev))]
    coff = got["cols"]["ctg_name_off"]
    assert [names[int(coff[c]):int(coff[c + 1])].decode() for c in range(C_)] == st.ctg_names
