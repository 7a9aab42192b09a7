"""Enumeration cases: crafted contigs whose walk-sum distribution is chosen on purpose, for K8's queues.

The k-walk enumeration pops walks in the order (score sum, anom, ratio qnz / qtot, heap node, insertion index).  What the
sorted-front / sorted-runs / far-tier queue of alignasm_amd/csrc/aasm_enum.h does - which compare decides, whether the
threshold T on the sum ever moves, how many pushes go to the far tier, how many entries wait at once, where runs are cut -
follows from how the walks' sums are distributed, and synth() batches hold whatever distribution they happen to hold.  This
module builds contigs that hold a named one (a plain helper, imported by tests/test_enum_cases_cpu.py,
tests/test_gpu_enum_edges.py and tools/k8_stress.py).

The piece (records as in wide_cases._batch):
  stages(s, m, lens, mapq)   s stages in series, each of m parallel records over one query span on distinct chromosomes, the
                             next stage's query start 51 past the longest record (capacity_cases.fan, s times).  Records of
                             neighbouring stages all link, records of one stage never do: m ** s walks, one record per stage
                             (where every length is positive and the stages do not reach into each other).  A record's
                             length moves the sums of the walks through it; its mapq (0 or not) moves their ratio alone.
                             colinear=g puts alternative 0 of every stage on chromosome 0, g bases of reference behind
                             alternative 0 of the stage before: at g = 2 000 (the translocation penalty) that link weighs
                             what the links between chromosomes weigh, with one anomaly fewer.
What a contig is, is never taken from these formulas: coverage() counts it from the oracle's walks and the emulation's
klast / kcand records, and tests/test_enum_cases_cpu.py asserts every fact named in contigs().
"""
from fractions import Fraction

import numpy as np

from wide_cases import _batch

QT = 10 ** 8                                           # qry_total of every contig but negative_ties


def stages(s, m, lens=900, mapq=60, colinear=None, q0=1000, r0=10 ** 6):
    """lens / mapq: a number, or f(stage, alternative); m: a number, or the stages' widths."""
    ms = [m] * s if isinstance(m, int) else list(m)
    assert len(ms) == s
    L = lens if callable(lens) else (lambda t, i: lens)
    M = mapq if callable(mapq) else (lambda t, i: mapq)
    out, q, r_col = [], q0, r0
    for t in range(s):
        ls = [L(t, i) for i in range(ms[t])]
        assert min(ls) > 0, (t, ls)
        for i, l in enumerate(ls):
            r, chr_ = r0 + 5 * 10 ** 6 * t + 7 * i, 1 + i + max(ms) * t
            if colinear is not None and i == 0:
                r, chr_ = r_col, 0
                r_col = r + l + colinear
            out.append((q, q + l - 1, r, r + l - 1, chr_, 1, M(t, i)))
        q += max(ls) + 51
    return out


def contigs():
    """[(name, qry_total, records)]: one contig per distribution (fewer than 40 records each).

    all_equal       4 096 walks of one sum, one anom, one ratio: every order decision is node:index, T never moves, the far tier
                    stays empty.  Heap nodes are numbered from dest outwards, so this order is depth-first and only a handful of
                    entries wait at once: the front alone serves it;
    all_equal_big   the same with more than 10 000 walks, for K = 10 000;
    equal_deep      6 561 walks of one sum and one anom with more than 1 000 entries waiting at once (alternative 0 of every
                    stage at mapq 0: the ratio orders breadth-first): flushes of I, merges down the levels, runs cut at
                    K - found and the bound that drops pushes, all with T where it started;
    ratio_only      one sum, one anom, 8 ratios (0 ... 7 records of mapq 0 among 7): key2's low 42 bits decide;
    all_distinct    4 096 walks of 4 096 sums (lengths 5 000 - i 2^t): every push but the first lies above T when it is made;
    clusters        four groups of 1 024 equal sums, 200 apart (the last stage's lengths differ by 200): a far-tier scan brings a
                    whole group near at once (I overflows inside eq_redistribute's loop);
    geometric       2 048 distinct sums (lengths 100 000 - i 3^t) with 11 distinct gaps, each more than twice the one before (a far
                    sample whose quartile lies far from its median);
    small_far       128 walks, 32 of them above the first sum: fewer than 64 far entries, the n < 64 sample path;
    few_2 ... few_5 2 ... 5 walks; chain: one walk (no sidetrack, no queue): the queue runs empty at once;
    negative_ties   qry_total = 0 (the last stage runs past the query's end): 1 024 walks, every sum negative, four groups of ties;
    anom_split      729 walks of one sum and 6 different anoms: alternative 0 of every stage is colinear with its neighbours on
                    chromosome 0 at a reference gap of 2 000, the translocation penalty.
    """
    C = [("all_equal", QT, stages(6, 4)),
         ("all_equal_big", QT, stages(7, 4)),
         ("equal_deep", QT, stages(8, 3, 900, lambda t, i: 0 if i == 0 else 60)),
         ("ratio_only", QT, stages(7, 3, 900, lambda t, i: 0 if i == 1 else 60)),
         ("all_distinct", QT, stages(12, 2, lambda t, i: 5000 - i * 2 ** t)),
         ("clusters", QT, stages(6, 4, lambda t, i: 900 - (200 * i if t == 5 else 0))),
         ("geometric", QT, stages(11, 2, lambda t, i: 100000 - i * 3 ** t)),
         ("small_far", QT, stages(6, [2, 2, 2, 2, 2, 4], lambda t, i: 900 - (300 if (t, i) == (5, 3) else 0))),
         ("chain", QT, stages(5, 1))]
    C += [(f"few_{w}", QT, stages(2, [w, 1])) for w in (2, 3, 5)] + [("few_4", QT, stages(2, 2))]
    C += [("negative_ties", 0, stages(5, 4, lambda t, i: 900 - (200 * i if t == 4 else 0))),
          ("anom_split", QT, stages(6, 3, colinear=2000))]
    return C


def batch(cs):
    """(names, HostBatch) of [(name, qry_total, records)]."""
    return [n for n, _, _ in cs], _batch([(qt, recs) for _, qt, recs in cs])


def join(parts):
    """One HostBatch of the contigs [(HostBatch, contig index)], in that order."""
    ones = [hb.subset([c]).arrays for hb, c in parts]
    A = {k: np.concatenate([a[k] for a in ones]) for k in ones[0] if k not in ("ctg_rec_off", "rec_rng_off")}
    A["ctg_rec_off"] = np.concatenate([[0], np.cumsum([len(a["qry_str"]) for a in ones])])
    A["rec_rng_off"] = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(a["rec_rng_off"]) for a in ones]))])
    return type(parts[0][0])(A)


def mixed(T):
    """(names, HostBatch): the crafted contigs in reverse order with synth() contigs between them - a queue that overruns its
    slice of the run storage (or its far tier behind the runs) lands in a neighbour that is checked, and the neighbours differ
    from the first batch's."""
    names, hb = batch(contigs())
    syn = [(T.synth(3, 60, 5, dup_every=3), c) for c in range(3)] + [(T.synth(1, 80, 31, dense=True), 0)]
    parts, out = [], []
    for i, c in enumerate(reversed(range(len(names)))):
        parts.append((hb, c)); out.append(names[c])
        if i % 4 == 1 and syn:
            parts.append(syn.pop(0)); out.append("synth_%d" % len(syn))
    return out, join(parts)


# ---- what the oracle and the emulation say -------------------------------------------------------------------------------------
K_ALL = 60000                                          # above every contig's walk count: the oracle lists all walks


def emul_enum(T, hb, K):
    """An emulated solve (the d-ary heap form) at K -> per contig (kfound, kd[:kfound], klast[:kfound], kcand rows of
    {heap node, predecessor}): the CPU reference of the pops' insertion indices and of every numbered push."""
    out = T.emul_solve(hb, K)
    nc, S = hb.n_contigs, 3 * K + 1
    kf = T.emul_debug("kfound", np.int32)[:nc]
    kd = T.emul_debug("kd", T.DIST_DT)[:nc * K]
    kl = T.emul_debug("klast", np.int32)[:nc * K]
    cand = T.emul_debug("kcand", np.int32)[:nc * S * 8].reshape(nc * S, 8)[:, :2]
    return out, [(int(kf[c]), kd[c * K:c * K + kf[c]].copy(), kl[c * K:c * K + kf[c]].copy(), cand[c * S:(c + 1) * S].copy()) for c in range(nc)]


def replay(o, found, klast, cand):
    """The pushes of every pop, from the oracle's heap arrays: the queue's first entry is src's heap root; a popped entry
    (node x, predecessor p, insertion index i) pushes the root of the heap of x's head vertex (predecessor i), then x's left
    and right child (predecessor p), each where it exists.  Checks cand (rows {heap node, predecessor}) against that and
    returns (pushes made, pushes made before pop t for every t, the peak of pushes so far - pops so far)."""
    left, right, hv, root = o["heap_left"], o["heap_right"], o["heap_v"], o["heap_root"]
    src = len(o["csr_rowptr"]) - 3
    if found <= 1 and root[src] < 0:
        return 0, np.zeros(1, np.int64), 0
    assert tuple(cand[0]) == (root[src], -1)
    nn, peak = 1, 1
    before = np.zeros(found + 1, np.int64)
    for t in range(1, found):
        before[t] = nn
        i = int(klast[t])
        assert 0 <= i < nn, (t, i, nn)
        x, p = int(cand[i, 0]), int(cand[i, 1])
        for node, pre in ((root[hv[x]], i), (left[x], p), (right[x], p)):
            if node >= 0:
                assert tuple(cand[nn]) == (node, pre), (t, nn)
                nn += 1
        peak = max(peak, nn - t)
    before[found] = nn
    return nn, before, peak


def facts(T, hb, c, K=None, run=None):
    """One contig's facts.  (a) W, the walk count; (b) distinct sums (and the sums, anoms, ratios themselves); from an emulated
    solve at K (default W + 1: nothing is cut or dropped, every push is popped): (c) far_pops, the pops whose sum exceeds the
    first queue entry's - T starts there and only a far-tier scan raises it; (d) far_pushes, the pushes above that sum (a
    push's sum is that of the pop that names it in klast); (e) peak, the most entries pending at once (pushes so far - pops
    so far), which is the kernel's own count where K >= pushes (peak_exact) and an upper bound of it otherwise; and where it
    is exact, scans / scan_near: the pops that rise above every sum before them (each needs a far-tier scan of its own), and
    the most entries one such scan must bring near (a lower bound: the pending entries of exactly the new sum)."""
    o = T.oracle_debug(hb, c, K_ALL)
    s = (o["kd_qry"] + o["kd_ref"]).astype(np.int64)
    W = len(s)
    assert W < K_ALL
    K = K or W + 1
    found, kd, klast, cand = (run or emul_enum(T, hb, K)[1])[c]
    assert found == min(W, K)
    pushes, before, peak = replay(T.oracle_debug(hb, c, K), found, klast, cand)
    es = (kd["qry"] + kd["ref"]).astype(np.int64)
    f = dict(W=W, sums=s, distinct=len(np.unique(s)), anoms=sorted(set(o["kd_anom"].tolist())), N=int(np.diff(hb.arrays["ctg_rec_off"])[c]),
             ratios=sorted({Fraction(int(a), max(int(b), 1)) for a, b in zip(o["kd_qnz"], o["kd_qtot"])}),
             K=K, pushes=pushes, peak=peak, peak_exact=K >= pushes, far_pops=0, far_pushes=0, scans=0, scan_near=0, first=None)
    if found > 1:
        f["first"] = first = int(es[1])
        f["far_pops"] = int((es[1:] > first).sum())
        f["far_pushes"] = None
        if f["peak_exact"]:
            assert found == pushes + 1 and sorted(klast[1:]) == list(range(pushes))    # every push is popped, once
            popped_at = np.zeros(pushes, np.int64)
            popped_at[klast[1:]] = np.arange(1, found)
            psum = es[popped_at]                                                       # ... so a push's sum is its pop's
            f["far_pushes"] = int((psum > first).sum())
            # a pop above every sum before it: the near tier was empty and T below this sum, so a scan ran just before it, and T
            # rose to this sum at least - every pending entry of exactly this sum came near in that one scan
            top = first
            for t in range(2, found):
                if es[t] > top:
                    top = int(es[t])
                    pending = (np.arange(pushes) < before[t]) & (popped_at >= t)
                    f["scans"] += 1
                    f["scan_near"] = max(f["scan_near"], int((pending & (psum == top)).sum()))
    return f


def coverage(T, cs=None):
    """{contig name: facts} of the crafted contigs, each from its own emulated solve at K = W + 1."""
    names, hb = batch(cs or contigs())
    W = [len(T.oracle_debug(hb, c, K_ALL)["kd_qry"]) for c in range(len(names))]
    out = {}
    for c, n in enumerate(names):
        one = hb.subset([c])
        out[n] = facts(T, one, 0, W[c] + 1)
    return out


def groups(sums):
    """The sorted distinct sums' (value, walks) and the gaps between neighbours."""
    u, cnt = np.unique(sums, return_counts=True)
    return u, cnt, np.diff(u)
