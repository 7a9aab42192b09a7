"""Overhang corpus: records whose query interval runs to or past the query's end (qry_end >= qry_total - 1).

The edge of such a record into `dest` weighs (qry_total - qry_end - 1) * 2 <= 0 (the row fills of aasm_kernels.h; the
oracle's `add_edge(vtx_to_index(i, i), dest, dist)`), every src -> dest walk ends in exactly one such edge, and so walk score sums (qry + ref) go
negative.  The reference solves these records like any others, and the --alt merge produces them on purpose (appended rows
read qry_total = 0).  The other generators of the suite all keep qry_end < qry_total; this module rewrites `qry_total`, and
nothing else, of batches they made (a plain helper, imported by tests/test_overhang_cpu.py and tests/test_gpu_overhang.py):

  overhang(hb, mode)   zero / longest / touch / median / mixed: every dest edge negative, only the longest record's (-2), that
                       edge at exactly 0, about half of them, and totals that differ between the records of one contig;
  centre(hb, K)        a common qry_total per contig that puts the walk at a chosen rank at sum -1 or -2: the K walks of
                       the contig cross zero part-way through the enumeration;
  profile(hb, K)       per contig (found, negative, min sum, max sum) from the oracle alone: what a test's inputs do hold;
  overhang_text        the same rewrite on column 2 of PAF text, for the reader / writer / command-line routes;
  debug / expect       the oracle's intermediates of a contig, computed once per (batch contents, contig, K, nsl).
"""
import hashlib

import numpy as np

from alignasm_amd._abi import HostBatch

MODES = ("zero", "longest", "touch", "median", "mixed")


def _with_totals(hb, qt):
    A = {k: v.copy() for k, v in hb.arrays.items()}
    A["qry_total"] = np.asarray(qt, np.int64)
    return HostBatch(A)


def _mixed_pick(rng, n):
    """A seeded random half of n records (at least one of each kind where n >= 2)."""
    pick = np.zeros(n, bool)
    pick[rng.permutation(n)[:max(1, n // 2)]] = True
    return pick


def _contig_totals(mode, qe, qt, rng):
    if mode == "zero":
        return np.zeros_like(qt)
    if mode == "longest":
        return np.full_like(qt, qe.max())
    if mode == "touch":
        return np.full_like(qt, qe.max() + 1)
    if mode == "median":
        return np.full_like(qt, int(np.median(qe)) + 1)
    if mode == "mixed":
        return np.where(_mixed_pick(rng, len(qt)), 0, qt)
    raise ValueError("overhang mode %r: not one of %s" % (mode, MODES))


def overhang(hb, mode, seed=0) -> HostBatch:
    """The batch with `qry_total` rewritten per contig as `mode` says; every other array as it was."""
    off = hb.arrays["ctg_rec_off"]
    qt = hb.arrays["qry_total"].astype(np.int64).copy()
    rng = np.random.default_rng(seed)
    for c in range(len(off) - 1):
        a, b = int(off[c]), int(off[c + 1])
        if b > a:
            qt[a:b] = _contig_totals(mode, hb.arrays["qry_end"][a:b].astype(np.int64), qt[a:b], rng)
    return _with_totals(hb, qt)


# ---- the oracle's intermediates, once per (batch contents, contig, K, nsl) ---------------------------------------------------
_DEBUG = {}


def _key(hb):
    if not hasattr(hb, "_overhang_key"):
        h = hashlib.blake2b(digest_size=16)
        for k in sorted(hb.arrays):
            h.update(np.ascontiguousarray(hb.arrays[k]).tobytes())
        hb._overhang_key = h.hexdigest()
    return hb._overhang_key


def debug(hb, c, K=10000, nsl=False):
    k = (_key(hb), int(c), int(K), bool(nsl))
    if k not in _DEBUG:
        import aasm_testlib as T
        _DEBUG[k] = T.oracle_debug(hb, c, K, nsl)
    return _DEBUG[k]


def expect(hb, K=10000, nsl=False):
    """expect(c) for T.diff_intermediates: the oracle's intermediates of contig c, shared with profile()."""
    return lambda c: debug(hb, c, K, nsl)


def forget():
    _DEBUG.clear()


def sums(hb, c, K=10000, nsl=False):
    """The score sums (qry + ref) of contig c's walks in the oracle's order; empty for a contig of fewer than two records
    (no graph, no enumeration)."""
    off = hb.arrays["ctg_rec_off"]
    if off[c + 1] - off[c] <= 1:
        return np.zeros(0, np.int64)
    o = debug(hb, c, K, nsl)
    return (o["kd_qry"] + o["kd_ref"]).astype(np.int64)


def profile(hb, K=10000, nsl=False):
    """Per contig (found, n_negative, min_sum, max_sum) of the oracle's K walks; (0, 0, 0, 0) where nothing is enumerated."""
    rows = []
    for c in range(hb.n_contigs):
        s = sums(hb, c, K, nsl)
        rows.append((len(s), int((s < 0).sum()), int(s.min()), int(s.max())) if len(s) else (0, 0, 0, 0))
    return rows


def centre(hb, K, rank_frac=0.5, nsl=False):
    """-> HostBatch; its `.skipped` lists the contigs that could not be centred.  Every walk ends in one dest edge, so with one
    qry_total for all records of a contig, lowering it by d lowers every walk sum by 2 d and leaves their order alone.  Each
    contig gets the common qry_total at which its walk at rank rank_frac * found has sum -1 or -2: the walks before it are
    negative, the ones after it mostly are not.  A contig whose total would fall below 0 keeps its largest old total."""
    off = hb.arrays["ctg_rec_off"]
    qt = hb.arrays["qry_total"].astype(np.int64).copy()
    for c in range(len(off) - 1):
        a, b = int(off[c]), int(off[c + 1])
        if b - a > 1:
            qt[a:b] = qt[a:b].max()
    common = _with_totals(hb, qt)
    skipped = []
    for c in range(len(off) - 1):
        a, b = int(off[c]), int(off[c + 1])
        s = sums(common, c, K, nsl)
        if not len(s):
            continue
        at = int(s[min(len(s) - 1, int(rank_frac * len(s)))])
        d = (at + 2) // 2                                    # at - 2 d is -1 (at odd) or -2 (at even)
        if qt[a] - d < 0:
            skipped.append(c)
            continue
        qt[a:b] -= d
    out = _with_totals(hb, qt)
    out.skipped = skipped
    return out


# ---- PAF text -----------------------------------------------------------------------------------------------------------------
def overhang_text(text, mode, seed=0):
    """`text` (bytes) with column 2, the query's length, rewritten per query name as overhang() does per contig."""
    lines = text.split(b"\n")
    rows = [(i, ln.split(b"\t")) for i, ln in enumerate(lines) if ln]
    by_name = {}
    for i, f in rows:
        by_name.setdefault(f[0], []).append((i, f))
    rng = np.random.default_rng(seed)
    for name, group in by_name.items():                      # (dict order: first appearance in the text)
        qe = np.array([int(f[3]) - 1 for _, f in group], np.int64)          # (column 4 is one past the record's qry_end)
        qt = np.array([int(f[1]) for _, f in group], np.int64)
        for (i, f), v in zip(group, _contig_totals(mode, qe, qt, rng)):
            f[1] = b"%d" % int(v)
            lines[i] = b"\t".join(f)
    return b"\n".join(lines)
