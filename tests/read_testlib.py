"""Helpers of the device reader's tests (tests/test_read_cpu.py, tests/test_gpu_read.py): the emulated reader, a batch view as
numpy arrays (host or device memory), the comparisons against the host reader and the I/O oracle."""
import ctypes as C
import os

import numpy as np

import aasm_testlib
from alignasm_amd._abi import BatchIn, _np_from

# name -> (dtype, length from (C, R, cs bytes)); rng_* stay NULL in the cs form
VIEW_ARRAYS = {
    "ctg_rec_off": (np.int64, lambda c, r, t: c + 1), "qry_str": (np.int64, lambda c, r, t: r), "qry_end": (np.int64, lambda c, r, t: r),
    "ref_str": (np.int64, lambda c, r, t: r), "ref_end": (np.int64, lambda c, r, t: r), "qry_total": (np.int64, lambda c, r, t: r),
    "ref_chr": (np.int32, lambda c, r, t: r), "aln_fwd": (np.uint8, lambda c, r, t: r), "map_qul": (np.uint8, lambda c, r, t: r),
    "rec_rng_off": (np.int64, lambda c, r, t: r + 1), "rec_cs_off": (np.int64, lambda c, r, t: r + 1), "cs_text": (np.uint8, lambda c, r, t: t),
}


def _declare(lib):
    lib.emr_parse_device.argtypes = [C.c_char_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emr_free.argtypes = [C.c_void_p]
    lib.emr_counter.restype = C.c_int64
    lib.emr_tile.restype = C.c_int64
    lib.aasm_last_error.restype = C.c_char_p
    lib.aasm_paf_free.argtypes = [C.c_void_p]
    lib.aasm_paf_batch.argtypes = [C.c_void_p, C.c_void_p]
    lib.aasm_paf_to_text.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.aasm_paf_write_outputs.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p]


def build_emul(san=False):
    """tests/host_emul/read_emul.cpp -> its library, or with san (library, path of read_emul_san)."""
    return aasm_testlib.build_emul("read", san, _declare)


def host_fetch(ptr, n, dtype):
    return _np_from(ptr, n, dtype)


def view_arrays(view: BatchIn, fetch=host_fetch):
    """The arrays of a batch view in its cs form as numpy copies; fetch(ptr, n, dtype) reads host or device memory."""
    c, r = int(view.n_contigs), int(view.n_records)
    a = {"n_contigs": c, "n_records": r, "n_ranges": int(view.n_ranges)}
    assert not view.rng_qry_l and not view.rng_qry_r and not view.rng_ref_l and view.cs_text and view.rec_cs_off
    a["rec_cs_off"] = fetch(view.rec_cs_off, r + 1, np.int64)
    t = int(a["rec_cs_off"][-1])
    for name, (dt, n) in VIEW_ARRAYS.items():
        if name != "rec_cs_off":
            a[name] = fetch(getattr(view, name), n(c, r, t), dt)
    return a


def diff_views(want, got):
    """Names of the entries of two view_arrays() results that differ."""
    return [k for k in want if not np.array_equal(np.asarray(want[k]), np.asarray(got[k]))]


class EmulPaf:
    """A container the emulation library returned, through that library's own codec entries."""

    def __init__(self, lib, handle):
        self.lib, self._h = lib, handle

    def view(self):
        v = BatchIn()
        assert self.lib.aasm_paf_batch(self._h, C.byref(v)) == 0
        return v

    def to_text(self):
        p, n = C.c_void_p(), C.c_int64()
        assert self.lib.aasm_paf_to_text(self._h, C.byref(p), C.byref(n)) == 0
        try:
            return C.string_at(p, n.value)
        finally:
            C.CDLL(None).free(p)

    def write_outputs(self, out, *paths):
        assert self.lib.aasm_paf_write_outputs(self._h, C.byref(out), *(os.fsencode(p) for p in paths)) == 0, self.lib.aasm_last_error()

    def __del__(self):
        if self._h:
            self.lib.aasm_paf_free(self._h)
            self._h = None


def emul_parse(lib, text, flags=0, max_blocks=0, want_paf=True, want_view=True):
    """emr_parse_device -> (code, message, EmulPaf or None, the view's arrays or None)."""
    h, up, view = C.c_void_p(), C.c_void_p(), BatchIn()
    rc = lib.emr_parse_device(text, len(text), flags, max_blocks, C.byref(h) if want_paf else None, C.byref(up) if want_view else None,
                              C.byref(view) if want_view else None)
    if rc != 0:
        assert not h and not up
        return rc, (lib.aasm_last_error() or b"").decode(), None, None
    arrays = None
    if want_view:
        try:
            arrays = view_arrays(view)
        finally:
            lib.emr_free(up)
    return 0, "", EmulPaf(lib, h) if want_paf else None, arrays


def host_read(api, text):
    """The yardstick: the host reader in the same mode -> (Paf, the container's arrays, to_text())."""
    paf = api.Paf.parse(text, device_ranges=True)
    return paf, view_arrays(paf.view()), paf.to_text()


def host_error(api, text):
    """(code, message) of the host reader on a bad text."""
    try:
        api.Paf.parse(text, device_ranges=True)
    except api.AlignasmError as e:
        return e.code, str(e).split(": ", 1)[1]
    raise AssertionError("the host reader takes this text")


def check_against_oracle(T, text, got, got_text):
    """The I/O oracle's independent reading of the text (read_paf + to_arrays) against a reader's arrays and row text: every
    solver array, the contig offsets and names, the reference names, the tags."""
    io = T.io_oracle()
    st = io.read_paf(text)
    want = {k: np.asarray(v, np.int64) for k, v in io.to_arrays(st).items()}
    for k in ("ctg_rec_off", "qry_str", "qry_end", "ref_str", "ref_end", "qry_total", "ref_chr", "aln_fwd", "map_qul", "rec_rng_off"):
        assert np.array_equal(want[k], got[k].astype(np.int64)), k
    recs = [r for ctg in st.paf_data for r in ctg]
    tags = [r.cs_string.encode() for r in recs]
    assert np.array_equal(got["rec_cs_off"], np.concatenate([[0], np.cumsum([len(t) for t in tags])]).astype(np.int64))
    assert got["cs_text"].tobytes() == b"".join(tags)
    rows = [ln.split(b"\t") for ln in got_text.split(b"\n") if ln]
    assert len(rows) == len(recs)
    names = [st.ctg_names[c].encode() for c, ctg in enumerate(st.paf_data) for _ in ctg]
    assert [f[0] for f in rows] == names
    assert [f[5] for f in rows] == [st.chr_rev[r.ref_chr].encode() for r in recs]
    assert [int(f[6]) for f in rows] == [r.ref_total for r in recs]
    assert [(int(f[9]), int(f[10])) for f in rows] == [(r.mat_num, r.aln_len) for r in recs]


def hip_fetcher(api):
    """fetch(ptr, n, dtype) for DEVICE memory, through the HIP runtime the library runs on."""
    hip = C.CDLL(api._torch_hip_runtime() or "libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def fetch(ptr, n, dtype):
        out = np.zeros(n, dtype)
        if n > 0:
            assert ptr
            assert hip.hipDeviceSynchronize() == 0
            assert hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0        # hipMemcpyDeviceToHost
        return out
    return fetch
