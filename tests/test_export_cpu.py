"""CPU tier of the device-side export (aasm_result_sizes / aasm_result_export): the C-ABI surface, the ctypes mirrors, one HIP
runtime per process whatever the import order, and the pack kernels (1-lane host emulation) against fetch_results."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "alignasm_amd.h")
NEW_FUNCS = ("aasm_result_sizes", "aasm_result_export")

# the shapes of tests/test_emul_vs_oracle.py: (contigs, recs, seed, K, dense, dup_every, shuffle, heavy_tail, nsl)
CASES = [
    (10, 100, 1, 10000, False, 0, False, False, False),
    (3, 700, 11, 4, False, 0, False, False, False),
    (3, 300, 31, 16, True, 0, False, False, False),
    (2, 300, 31, 10000, True, 0, False, False, False),
    (4, 300, 5, 10000, False, 3, False, False, False),       # co-optimal ties (.all paths)
    (6, 200, 7, 10000, False, 0, False, False, True),
    (3, 250, 8, 10000, True, 0, False, False, True),
    (6, 150, 9, 10000, False, 3, True, False, False),
    (40, 50, 10, 1, False, 0, False, True, False),
    (30, 40, 10, 10000, True, 0, True, True, False),
    (5, 1, 3, 10000, False, 0, False, False, False),         # single-record contigs
    (5, 2, 3, 10000, False, 0, False, False, False),
    (8, 40, 13, 10000, True, 1, True, False, False),         # every record duplicated
    (2, 2600, 17, 4, False, 3, True, False, False),
    (3, 1024, 19, 1, False, 0, True, False, False),
    (2, 1025, 23, 1, False, 5, True, False, False),
]
CASE_IDS = ["c%dx%d_s%d_k%d_%s%s%s%s%s" % (c[0], c[1], c[2], c[3], "D" if c[4] else "S", f"_dup{c[5]}" if c[5] else "",
                                           "_shuf" if c[6] else "", "_ht" if c[7] else "", "_nsl" if c[8] else "") for c in CASES]


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_declares_the_export():
    src = _header_text()
    assert re.search(r"int\s+aasm_result_sizes\s*\(\s*aasm_result\s*\*\s*res\s*,\s*aasm_out_sizes\s*\*\s*sz\s*\)", src)
    assert re.search(r"int\s+aasm_result_export\s*\(\s*aasm_result\s*\*\s*res\s*,\s*const\s+aasm_out_sizes\s*\*\s*sz\s*,\s*"
                     r"const\s+aasm_dev_out\s*\*\s*dst\s*,\s*void\s*\*\s*stream\s*\)", src)
    assert re.search(r"typedef\s+struct\s+aasm_out_sizes\s*\{", src) and re.search(r"typedef\s+struct\s+aasm_dev_out\s*\{", src)
    assert re.search(r"#define\s+AASM_ABI_VERSION\s+3\b", src)


def test_library_exports_the_export(T):
    api = T.api()
    for n in NEW_FUNCS:
        assert n in api.EXPORTED
        assert hasattr(api.LIB, n)
    assert api.LIB.aasm_abi_version() == 3


def test_ctypes_mirrors_have_the_header_sizes(tmp_path):
    """sizeof / offsetof of the two new structs from the system compiler against the ctypes mirrors."""
    from alignasm_amd import _abi
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    fields = {"aasm_out_sizes": [n for n, _ in _abi.OutSizes._fields_], "aasm_dev_out": [n for n, _ in _abi.DevOut._fields_]}
    lines = ['#include <cstdio>', '#include <cstddef>', '#include "alignasm_amd.h"', "int main() {"]
    for st, names in fields.items():
        lines.append(f'  std::printf("%zu\\n", sizeof({st}));')
        lines += [f'  std::printf("%zu\\n", offsetof({st}, {n}));' for n in names]
    lines.append("  return 0; }")
    (tmp_path / "probe.cpp").write_text("\n".join(lines) + "\n")
    subprocess.run([cxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), "probe.cpp", "-o", "probe"], cwd=tmp_path, check=True)
    got = [int(x) for x in subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for cls in (_abi.OutSizes, _abi.DevOut):
        want.append(C.sizeof(cls))
        want += [getattr(cls, n).offset for n, _ in cls._fields_]
    assert got == want
    assert C.sizeof(_abi.OutSizes) == 5 * 8 and C.sizeof(_abi.DevOut) == 8 * 8


@pytest.mark.parametrize("order", ["torch_first", "alignasm_first"])
def test_one_hip_runtime_per_process(order):
    """Whichever of torch and alignasm_amd a process imports first, exactly one libamdhip64 is mapped."""
    pytest.importorskip("torch")
    imports = "import torch; import alignasm_amd" if order == "torch_first" else "import alignasm_amd; import torch"
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); {imports}\n"
            "maps = set(l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l)\n"
            "print(len(maps)); print(*sorted(maps), sep='\\n')\n")
    r = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True, timeout=300)
    lines = r.stdout.split("\n")
    assert lines[0] == "1", r.stdout


# ---- the pack kernels, emulated, against fetch_results on the same workspace -------------------------------------------
@pytest.fixture(scope="module")
def emx(T):
    return T.build_emul("export")


def _emulated_export_and_fetch(emx, T, hb, K, nsl=False, **hooks):
    from alignasm_amd._abi import BatchOut, DevOut, OUT_ELEM_DTYPE, make_opts, unpack_out
    o = make_opts(K, nsl, 0, False, True, **hooks)
    sz = np.zeros(5, np.int64)
    assert emx.emx_solve_and_size(C.byref(hb.view), C.byref(o), sz.ctypes.data_as(C.c_void_p)) == 0
    c, nm, na, npth, ne = (int(x) for x in sz)
    got = {"main_off": np.full(c + 1, -7, np.int64), "alt_off": np.full(c + 1, -7, np.int64), "all_path_off": np.full(c + 1, -7, np.int64),
           "all_elem_off": np.full(npth + 1, -7, np.int64), "main": np.zeros(nm, OUT_ELEM_DTYPE), "alt": np.zeros(na, OUT_ELEM_DTYPE),
           "all": np.zeros(ne, OUT_ELEM_DTYPE), "status": np.full(c, 99, np.int32)}
    P = lambda a: a.ctypes.data if a.size else None   # noqa: E731
    dst = DevOut(P(got["main_off"]), P(got["alt_off"]), P(got["all_path_off"]), P(got["all_elem_off"]), P(got["main"]), P(got["alt"]),
                 P(got["all"]), P(got["status"]))
    assert emx.emx_export(C.byref(dst)) == 0
    out = BatchOut()
    assert emx.emx_fetch(C.byref(out)) == 0
    try:
        want = unpack_out(out)
        assert want["n_contigs"] == c and int(out.n_all_paths) == npth
    finally:
        emx.emul_free_out(C.byref(out))
    return want, got


def _assert_identical(want, got):
    for k in ("main_off", "alt_off", "all_path_off", "all_elem_off", "main", "alt", "all", "status"):
        assert want[k].dtype == got[k].dtype and want[k].shape == got[k].shape, k
        assert want[k].tobytes() == got[k].tobytes(), k


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_emulated_pack_equals_host_pack(emx, T, case):
    nc, nr, seed, K, dense, dup, shuf, heavy, nsl = case
    hb = T.synth(nc, nr, seed, dense=dense, dup_every=dup, shuffle=shuf, heavy_tail=heavy)
    want, got = _emulated_export_and_fetch(emx, T, hb, K, nsl)
    _assert_identical(want, got)
    if dup and K > 1:
        assert len(want["all"]) > 0                                  # (the tie shapes do exercise .all)


@pytest.mark.parametrize("case", [CASES[0], CASES[4], CASES[7], CASES[12], CASES[13]], ids=lambda c: "seq_c%dx%d_s%d" % (c[0], c[1], c[2]))
def test_emulated_pack_equals_host_pack_sequential_select(emx, T, case):
    """The sequential selection kernel clears .all (all_gen rises) where the plan-based pick never does."""
    nc, nr, seed, K, dense, dup, shuf, heavy, nsl = case
    hb = T.synth(nc, nr, seed, dense=dense, dup_every=dup, shuffle=shuf, heavy_tail=heavy)
    want, got = _emulated_export_and_fetch(emx, T, hb, K, nsl, sequential_select=True)
    _assert_identical(want, got)


@pytest.mark.parametrize("mode", ["slot_twice", "rank_out_of_range"])
def test_emulated_pack_marks_a_broken_rank_and_stays_in_bounds(emx, T, mode):
    """The place kernel's check of the seq-rank invariant: records broken on purpose after the solve mark their contig
    AASM_E_INTERNAL in the exported status, every other contig keeps fetch's status and lists, and the offsets stay inside the
    arrays the sizes gave (the arrays carry a guard entry past their end that nothing may touch)."""
    from alignasm_amd._abi import BatchOut, DevOut, OUT_ELEM_DTYPE, make_opts, unpack_out
    hb = T.synth(*CASES[4][:3], dup_every=3)                       # co-optimal ties: contigs with several .all paths
    o = make_opts(CASES[4][3], False, 0, False, True)
    sz = np.zeros(5, np.int64)
    assert emx.emx_solve_and_size(C.byref(hb.view), C.byref(o), sz.ctypes.data_as(C.c_void_p)) == 0
    out = BatchOut()
    assert emx.emx_fetch(C.byref(out)) == 0
    try:
        want = unpack_out(out)
    finally:
        emx.emul_free_out(C.byref(out))
    emx.emx_break_rank.restype = C.c_int64
    bad = int(emx.emx_break_rank(0 if mode == "slot_twice" else 1, sz.ctypes.data_as(C.c_void_p)))
    assert bad >= 0
    c, nm, na, npth, ne = (int(x) for x in sz)
    G = 3                                                            # guard entries past each array's end
    got = {"main_off": np.full(c + 1 + G, -7, np.int64), "alt_off": np.full(c + 1 + G, -7, np.int64),
           "all_path_off": np.full(c + 1 + G, -7, np.int64), "all_elem_off": np.full(npth + 1 + G, -7, np.int64),
           "main": np.zeros(nm + G, OUT_ELEM_DTYPE), "alt": np.zeros(na + G, OUT_ELEM_DTYPE), "all": np.zeros(ne + G, OUT_ELEM_DTYPE),
           "status": np.full(c + G, 99, np.int32)}
    for k in ("main", "alt", "all"):
        got[k]["qs"] = -7
    P = lambda a: a.ctypes.data   # noqa: E731
    dst = DevOut(*(P(got[k]) for k in ("main_off", "alt_off", "all_path_off", "all_elem_off", "main", "alt", "all", "status")))
    assert emx.emx_export(C.byref(dst)) == 0
    for k in ("main_off", "alt_off", "all_path_off", "all_elem_off"):
        assert (got[k][-G:] == -7).all(), k
    for k in ("main", "alt", "all"):
        assert (got[k]["qs"][-G:] == -7).all(), k
    assert (got["status"][-G:] == 99).all()
    st = got["status"][:c]
    assert st[bad] == -6                                             # AASM_E_INTERNAL
    assert np.array_equal(np.delete(st, bad), np.delete(want["status"], bad))
    po, eo = got["all_path_off"][:c + 1], got["all_elem_off"][:npth + 1]
    assert po[0] == 0 and (np.diff(po) >= 0).all() and po[-1] == npth
    assert eo[0] == 0 and (np.diff(eo) >= 0).all() and eo[-1] == ne
    assert got["main"][:nm].tobytes() == want["main"].tobytes() and got["alt"][:na].tobytes() == want["alt"].tobytes()
    wpo, weo = want["all_path_off"], want["all_elem_off"]
    for k in range(c):                                               # the other contigs' .all lists are fetch's
        if k == bad:
            continue
        assert po[k + 1] - po[k] == wpo[k + 1] - wpo[k]
        assert got["all"][eo[po[k]]:eo[po[k + 1]]].tobytes() == want["all"][weo[wpo[k]]:weo[wpo[k + 1]]].tobytes(), k
