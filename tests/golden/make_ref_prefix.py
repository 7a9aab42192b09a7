"""Regenerates tests/golden/ref_prefix.npz: vectors recorded from the REAL solve_ctg_read() prefix.

Needs oracle/_ref/libaasm_ref_prefix_mono.so (oracle/Makefile: /root/reference/src/paf_data.cpp:1-738 piped to g++
from where it lies + our epilogue; bump-allocator flavour, so that node address order == allocation order).
The file holds DATA only: the input batches (record coordinates + match ranges, from the seeded generators
tests/test_fuzz.py::make_batch and the product's synthetic-PAF generator) and, per contig, what the reference's
own statements computed from them - sorted order, part ids, every (i, j) cut, vertex ids, adjacency lists with
all weight fields, anom_dis[dest], d / best, both Kahn orders, every heap node and root, the k-walk distances
(all 10 000 for the batches marked full, the first 64 otherwise) - the arrays of aasm_testlib.PREFIX_NAMES.

    python tests/golden/make_ref_prefix.py          # ref_prefix.npz
    python tests/golden/make_ref_prefix.py wide     # ref_prefix_wide.npz: the same from tests/wide_cases.py's batches
                                                    # (coordinates, weights and score sums above 2^31 / 2^32, up to 2^40 - 1)
    python tests/golden/make_ref_prefix.py overhang # ref_prefix_overhang.npz: the same from tests/overhang_cases.py's rewrites
                                                    # (qry_end >= qry_total - 1: negative dest edges and walk sums)
    python tests/golden/make_ref_prefix.py enum     # ref_prefix_enum.npz: the same from tests/enum_cases.py's crafted contigs
                                                    # (walk-sum distributions chosen on purpose; all 10 000 distances)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import aasm_testlib as T   # noqa: E402
from test_fuzz import make_batch   # noqa: E402
import wide_cases as W   # noqa: E402
import overhang_cases as O   # noqa: E402
import enum_cases as E   # noqa: E402

KD = ("kd_qry", "kd_ref", "kd_anom", "kd_qnz", "kd_qtot")
KD_SHORT = 64

# (tag, maker, nsl, keep all 10 000 distances)
BATCHES = [
    ("fuzz0", lambda: make_batch(3, 6, 30, 400, 0), False, True),
    ("fuzz1", lambda: make_batch(4, 6, 30, 400, 1), False, True),
    ("fuzz2", lambda: make_batch(5, 6, 30, 400, 2), False, True),
    ("fuzz0n", lambda: make_batch(6, 6, 30, 400, 0), True, False),
    ("fuzz1n", lambda: make_batch(7, 6, 30, 400, 1), True, False),
    ("fuzz2n", lambda: make_batch(8, 6, 30, 400, 2), True, False),
    ("fuzz0b", lambda: make_batch(9, 8, 60, 400, 0), False, False),
    ("fuzz2b", lambda: make_batch(10, 8, 60, 400, 2), False, False),
    ("c1", lambda: T.synth(10, 100, 1), False, False),                         # BASELINE configs[0] in full
    ("c2one", lambda: T.synth(1, 1000, 11), False, True),                      # one contig of configs[1]'s size
    ("dense", lambda: T.synth(1, 300, 31, dense=True), False, True),
    ("densen", lambda: T.synth(2, 200, 31, dense=True), True, False),
    ("dup3", lambda: T.synth(2, 200, 5, dup_every=3), False, True),
    ("dupshuf", lambda: T.synth(3, 150, 9, dup_every=3, shuffle=True), False, False),
    ("nsl", lambda: T.synth(3, 200, 7), True, False),
    ("alldup", lambda: T.synth(4, 40, 13, dense=True, dup_every=1, shuffle=True), False, False),
    ("ragged", lambda: T.synth(8, 40, 10, dense=True, shuffle=True, heavy_tail=True), False, False),
]



def _shifted(base, oname):
    if isinstance(base, str):
        base = dict(W.narrow_bases(T))[base] if base != "crafted" else W.crafted()[1]
    return W.shift(base, *W.offsets(base)[oname])


# kept small (the file is ~0.4 MB): the synthetic batches are smaller than wide_cases.narrow_bases', and only the fuzz and
# crafted batches with few distances keep all 10 000
WIDE_BATCHES = [
    ("wf33_0", lambda: make_batch(1000, 4, 20, W.WIDE_L[0], 0), False, False),
    ("wf33_1", lambda: make_batch(1001, 4, 20, W.WIDE_L[0], 1), False, True),
    ("wf33_2n", lambda: make_batch(1002, 4, 20, W.WIDE_L[0], 2), True, False),
    ("wf39_0", lambda: make_batch(1003, 4, 20, W.WIDE_L[1], 0), False, False),
    ("wf39_1n", lambda: make_batch(1004, 4, 20, W.WIDE_L[1], 1), True, False),
    ("wf39_2", lambda: make_batch(1005, 4, 20, W.WIDE_L[1], 2), False, False),
    ("crafted", lambda: W.crafted()[1], False, True),
    ("crafted_n", lambda: W.crafted()[1], True, True),
    ("crafted_top", lambda: W.crafted(top=True)[1], False, True),
    ("crafted_x32", lambda: _shifted("crafted", "x32"), False, True),
    ("fz0_x31", lambda: _shifted("fz0", "x31"), False, False),
    ("fz2_x32", lambda: _shifted("fz2", "x32"), True, False),
    ("syn_x32", lambda: _shifted(T.synth(1, 60, 5, dup_every=3), "x32"), False, False),
    ("syn_top", lambda: _shifted(T.synth(1, 60, 9), "top"), False, False),
    ("dense_5g", lambda: _shifted(T.synth(1, 50, 31, dense=True), "5g"), False, False),
]


# six fuzz contigs of at most 30 records per mode at large coordinates (at L = 400 hardly a walk sum is negative), one contig whose
# 10 000 walks cross zero half-way, and one whose 10 000 negative sums spread over more than 50 000
OVERHANG_BATCHES = [
    ("ov_zero", lambda: O.overhang(make_batch(60, 6, 30, 10 ** 8, 0), "zero"), False, False),
    ("ov_longest", lambda: O.overhang(make_batch(61, 6, 30, 10 ** 8, 1), "longest"), False, False),
    ("ov_touch", lambda: O.overhang(make_batch(62, 6, 30, 10 ** 8, 2), "touch"), False, False),
    ("ov_median_n", lambda: O.overhang(make_batch(63, 6, 30, 10 ** 8, 0), "median"), True, False),
    ("ov_mixed", lambda: O.overhang(make_batch(64, 6, 30, 10 ** 8, 2), "mixed", 64), False, True),
    ("ov_centre", lambda: O.centre(T.synth(1, 300, 5, dup_every=3), 10000), False, True),
    ("ov_spread", lambda: O.overhang(T.synth(6, 30, 4).subset([3]), "zero"), False, True),
]


# the crafted contigs of tests/enum_cases.py in one batch (under 40 records each; equal sums compress to next to nothing)
ENUM_BATCHES = [
    ("enum", lambda: E.batch(E.contigs())[1], False, True),
]


def _narrow(a):
    return a.astype(np.int32) if a.size and np.abs(a).max() < 2 ** 31 else a       # storage only; the loader widens again


def main(batches=BATCHES, name="ref_prefix.npz", packed=False):
    """packed: the per-contig arrays of a batch are stored back to back, one array per name ({tag}/p/{name}), with their
    lengths in {tag}/p~n (contigs x names, -1 for a contig not recorded) - far fewer arrays in the file, and the same values
    (aasm_testlib.RefPrefixVectors reads both layouts)."""
    assert T.ref_prefix(True) is not None, "build oracle/_ref first (make -C oracle)"
    out = {}
    tags = []
    cols = [n + "~b" if n == "heap_right" else n for n in T.PREFIX_NAMES] + ["kfound"]
    for tag, mk, nsl, full in batches:
        hb = mk()
        tags.append(tag)
        out[f"{tag}/nsl"] = np.array([1 if nsl else 0], np.int8)
        out[f"{tag}/full"] = np.array([1 if full else 0], np.int8)
        for k, a in hb.arrays.items():
            if k == "rng_qry_r":
                out[f"{tag}/in/{k}~len"] = _narrow(a - hb.arrays["rng_qry_l"])                     # storage only: r - l
                continue
            if k.startswith("rng_"):
                out[f"{tag}/in/{k}~d"] = _narrow(np.diff(a.astype(np.int64), prepend=0))           # storage only: first differences
                continue
            out[f"{tag}/in/{k}"] = _narrow(a) if a.dtype == np.int64 else a
        off = hb.arrays["ctg_rec_off"]
        for c in range(len(off) - 1):
            if off[c + 1] - off[c] <= 1:
                continue
            r = T.ref_prefix_debug(hb, c, nsl=nsl, names=T.PREFIX_NAMES)
            o = T.oracle_debug(hb, c, 10000, nsl)
            for n in T.PREFIX_NAMES:
                assert np.array_equal(r[n], o[n]), (tag, c, n)                 # (not needed for the record; a generator-side sanity check)
                a = r[n]
                if n in KD and not full:
                    a = a[:KD_SHORT]
                if n == "heap_right":                           # storage only: distance back to the child (0 = none)
                    out[f"{tag}/c{c}/{n}~b"] = np.where(a >= 0, np.arange(len(a)) - a, 0).astype(np.int32)
                    continue
                out[f"{tag}/c{c}/{n}"] = _narrow(a)
            out[f"{tag}/c{c}/kfound"] = np.array([len(r["kd_qry"])], np.int32)
        if packed:
            lens = np.full((len(off) - 1, len(cols)), -1, np.int32)
            for c in range(len(off) - 1):
                if f"{tag}/c{c}/kfound" in out:
                    lens[c] = [len(out[f"{tag}/c{c}/{n}"]) for n in cols]
            for j, n in enumerate(cols):
                parts = [out.pop(f"{tag}/c{c}/{n}").astype(np.int64) for c in range(len(off) - 1) if lens[c, j] >= 0]
                out[f"{tag}/p/{n}"] = _narrow(np.concatenate(parts) if parts else np.zeros(0, np.int64))
            out[f"{tag}/p~n"] = lens
    if packed:
        out["packed_cols"] = np.array(cols)
    out["tags"] = np.array(tags)
    out["source"] = np.array(["reference paf_data.cpp:223-738 via oracle/_ref/libaasm_ref_prefix_mono.so (MAX_PATH_COUNT = 10000)"])
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **out)
    print("wrote %s: %d batches, %d arrays, %d bytes" % (path, len(tags), len(out), os.path.getsize(path)))


if __name__ == "__main__":
    if sys.argv[1:] == ["wide"]:
        main(WIDE_BATCHES, "ref_prefix_wide.npz", packed=True)
    elif sys.argv[1:] == ["overhang"]:
        main(OVERHANG_BATCHES, "ref_prefix_overhang.npz", packed=True)
    elif sys.argv[1:] == ["enum"]:
        main(ENUM_BATCHES, "ref_prefix_enum.npz", packed=True)
    else:
        main()
