"""Helpers of the tests of the device reader's resident row columns (tests/test_read_cols_cpu.py, tests/test_gpu_read_cols.py):
the emulated reader with row columns, aasm_row_cols as numpy arrays (host or device memory), the yardstick's columns."""
import ctypes as C

import numpy as np

import aasm_testlib
import read_testlib as X
from alignasm_amd._abi import BatchIn, RowCols

# per-record columns of aasm_row_cols
ROW_KEYS = (("ref_total", np.int64), ("mat_num", np.int32), ("aln_len", np.int32), ("row_index", np.int32), ("cord_type", np.uint8))


def _declare(lib):
    lib.emrc_parse.argtypes = [C.c_char_p, C.c_int64, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emrc_free.argtypes = [C.c_void_p]
    lib.emrc_counter.restype = lib.emrc_pack_lanes.restype = C.c_int64
    lib.aasm_last_error.restype = C.c_char_p


def build_emul(san=False):
    """tests/host_emul/read_cols_emul.cpp -> its library, or with san (library, path of read_cols_emul_san)."""
    return aasm_testlib.build_emul("read_cols", san, _declare)


def cols_arrays(cols: RowCols, n_contigs, n_records, fetch=X.host_fetch):
    """aasm_row_cols as numpy copies; fetch(ptr, n, dtype) reads host or device memory."""
    a = {"n_chr": int(cols.n_chr)}
    a["ctg_name_off"] = fetch(cols.ctg_name_off, n_contigs + 1, np.int64)
    a["chr_name_off"] = fetch(cols.chr_name_off, a["n_chr"] + 1, np.int64)
    a["names"] = fetch(cols.names, int(a["chr_name_off"][-1]), np.uint8)
    for k, dt in ROW_KEYS:
        a[k] = fetch(getattr(cols, k), n_records, dt)
    return a


def diff_cols(want, got):
    """Names of the entries of two cols_arrays() results that differ."""
    return [k for k in want if not np.array_equal(np.asarray(want[k]), np.asarray(got[k]))]


def emul_parse(lib, text, flags=0, max_blocks=0, device_text=False):
    """emrc_parse -> (code, message, the view's arrays or None, the columns' arrays or None)."""
    up, view, cols, nb = C.c_void_p(), BatchIn(), RowCols(), C.c_int64(-1)
    rc = lib.emrc_parse(text, len(text), flags, max_blocks, 1 if device_text else 0, C.byref(up), C.byref(view), C.byref(cols), C.byref(nb))
    if rc != 0:
        assert not up
        return rc, (lib.aasm_last_error() or b"").decode(), None, None
    try:
        va = X.view_arrays(view)
        ca = cols_arrays(cols, va["n_contigs"], va["n_records"])
        assert nb.value == len(ca["names"])
    finally:
        lib.emrc_free(up)
    return 0, "", va, ca


def host_cols(rows_lib, paf):
    """The yardstick: rows_host_cols (aasm_rows.h) of a host-read container, through the rows emulation's emw_row_cols."""
    view = paf.view()
    keep, cols = C.c_void_p(), RowCols()
    assert rows_lib.emw_row_cols(paf._h, C.c_int64(0), C.c_int64(int(view.n_contigs)), C.byref(keep), C.byref(cols)) == 0
    try:
        return cols_arrays(cols, int(view.n_contigs), int(view.n_records))
    finally:
        rows_lib.emw_row_cols_free(keep)


def uploaded_cols(api, paf, fetch):
    """The yardstick on the device: aasm_paf_upload_rows on a host-read container, fetched back."""
    view = paf.view()
    up, cols = C.c_void_p(), RowCols()
    rc = api.LIB.aasm_paf_upload_rows(paf._h, C.c_int64(0), C.c_int64(int(view.n_contigs)), 0, C.byref(up), C.byref(cols))
    assert rc == 0, api.LIB.aasm_last_error()
    try:
        return cols_arrays(cols, int(view.n_contigs), int(view.n_records), fetch)
    finally:
        api.LIB.aasm_upload_free(up)
