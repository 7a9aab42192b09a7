"""Capacity edges: crafted contigs that sit at, one below and one above each fixed-size structure of the kernels.

The kernels keep per-contig state in fixed-size LDS and lane structures and switch to another path once a contig outgrows one.
synth() batches land on these edges only by chance.  This module builds contigs that land on them exactly (a plain helper,
imported by tests/test_capacity_edges.py and tests/test_gpu_capacity_edges.py):

  ring     REVQ_N = 32, the LDS window of both sweeps' ready queues: the most entries waiting at once (tail - head) at
           30 ... 34, 63 ... 65 and 300, from a fan released at once;
  rows     AASM_LONG_ROW = 16 / AASM_MID_ROW = 96, row_fill_tile's one-lane / 16-lane / whole-wave split (and kb_topo_fill's
           split at 16): out-degree 15, 16, 17, 95, 96, 97 and 200, on an ordinary vertex (fan) and on src (mirrored fan);
  heap     HEAP_KMAX = 16, the staging slot of a vertex's sidetrack keys: 15 ... 49 sidetracks on two vertices that follow each
           other in the heap wave's order (so that the next vertex's keys are prefetched right after a refilled row);
  gb       GB_MAXV / GB_MAXE and GB_MAXV_L / GB_MAXE_L, which aasm_k46_graph form builds a contig (or the separate launches);
  rev_ord  REV_ORD_MIDV / REV_ORD_MAXV, the dense batch's reversed-CSR fill, chosen by its largest contig;
  ratio    the sparse / dense switch ET > 6 VT;
  mw       the several-waves heap class, I >= 6 V && V >= 128;
  tail     the chain class's long tail, N >= max(2048, 4 * mean records) in a batch of more than 1 536 contigs.

The pieces (records as in wide_cases._batch; checked against the oracle by coverage()):
  fan(a, m)     a colinear records, then m parallel ones over one query span on distinct chromosomes: V = a + m + 2, E = a + 2 m.
                The last chain record has out-degree m (m - 1 sidetracks), dest in-degree m; both sweeps release the m at once;
  mirror(m, a)  the same reflected: src has out-degree m, the first chain record in-degree m;
  twin(m)       two parallel records, then a fan of m: both have out-degree m and are the only children of one tree vertex;
  shape(n,a,m)  n overlapping records (V = 2 n + 1, E = n (n + 1): the dense piece), then fan(a, m):
                V = 2 n + 1 + a + m, E = n (n + 1) + a + 2 m - 1.
Every target below is asserted against the oracle's own intermediates (coverage()), never against the formulas.
"""
import numpy as np

from wide_cases import _batch, _chain

REVQ_N = 32
RING_M = (30, 31, 32, 33, 34, 63, 64, 65, 300)
ROW_D = (15, 16, 17, 95, 96, 97, 200)
HEAP_ST = (15, 16, 17, 31, 32, 33, 48, 49)
GB_V = (1791, 1792, 1793, 3584, 3585)                  # GB_MAXV = 1 792, GB_MAXV_L = 3 584
GB_E = (4095, 4096, 4097, 8192, 8193)                  # GB_MAXE = 4 096, GB_MAXE_L = 8 192
REV_ORD_V = (3072, 3073, 12288, 12289)                 # REV_ORD_MIDV, REV_ORD_MAXV
MW_VI = ((127, 6 * 127 - 1), (127, 6 * 127), (128, 6 * 128 - 1), (128, 6 * 128))
TAIL_N = (2047, 2048)
GROUPED_MIN = 2560                                     # AASM_GROUPED_MIN
QT = 10 ** 8                                           # every contig's qry_total


def fan(a, m, r0=10 ** 6):
    c = _chain(1000, r0, a, 900, 50, 40)
    q = c[-1][1] + 51
    return c + [(q, q + 899, r0 + 5 * 10 ** 6 + 7 * i, r0 + 5 * 10 ** 6 + 7 * i + 899, 1 + i, 1, 60) for i in range(m)]


def mirror(m, a, r0=10 ** 6):
    f = [(1000, 1899, r0 + 7 * i, r0 + 7 * i + 899, 1 + i, 1, 60) for i in range(m)]
    return f + _chain(1950, r0 + 5 * 10 ** 6, a, 900, 50, 40)


def twin(m, r0=10 ** 6):
    x = [(1000, 1899, r0, r0 + 899, 0, 1, 60), (1000, 1899, r0 + 3 * 10 ** 6, r0 + 3 * 10 ** 6 + 899, 1, 1, 60)]
    return x + [(1950, 2849, r0 + 5 * 10 ** 6 + 7 * i, r0 + 5 * 10 ** 6 + 7 * i + 899, 2 + i, 1, 60) for i in range(m)]


def shape(n, a, m, r0=10 ** 6):
    d = _chain(1000, r0, n, 900, -100, -100)
    q, r = d[-1][1] + 51, d[-1][3] + 41
    c = _chain(q, r, a, 900, 50, 40)
    q = c[-1][1] + 51
    return d + c + [(q, q + 899, r + 5 * 10 ** 6 + 7 * i, r + 5 * 10 ** 6 + 7 * i + 899, 1 + i, 1, 60) for i in range(m)]


def shape_for(V, E):
    """shape(n, a, m) with V vertices and E edges (by the formulas above): the smallest dense piece that leaves a >= 1, m >= 1."""
    for n in range(1, 400):
        m = (E - V + 2) - n * n + n
        a = V - 2 * n - 1 - m
        if m >= 1 and a >= 1:
            return shape(n, a, m)
    raise ValueError((V, E))


def chain(n):
    return _chain(1000, 10 ** 6, n, 900, 50, 40)


def pad(n):
    """n 2-record contigs (V = 4, E = 3)."""
    return [("pad", chain(2))] * n


def batch(contigs):
    """(names, HostBatch) of [(name, records)]."""
    return [n for n, _ in contigs], _batch([(QT, recs) for _, recs in contigs])


# ---- the batches ---------------------------------------------------------------------------------------------------
def ring_contigs():
    return [(f"fan_{m}", fan(1, m)) for m in RING_M] + [("mirror_64", mirror(64, 2))]


def row_contigs():
    return [(f"fan_{d}", fan(2, d)) for d in ROW_D] + [(f"mirror_{d}", mirror(d, 2)) for d in ROW_D]


def heap_contigs():
    return [(f"twin_{s}", twin(s + 1)) for s in HEAP_ST]


def gb_contigs():
    out = [(f"gbV_{v}", chain(v - 2)) for v in GB_V]
    out += [(f"gbE_{e}", shape_for(1500 if e <= 4097 else 3000, e)) for e in GB_E]
    return out


def dense_filler(VT, ET, extra=1):
    """A dense contig (n overlapping records) that lifts a batch of VT vertices / ET edges above ET > 6 VT."""
    n = 2
    while ET + n * (n + 1) <= 6 * (VT + 2 * n + 1) + extra:
        n += 1
    return ("dense_%d" % n, _chain(1000, 10 ** 6, n, 900, -100, -100))


def ratio_contigs(t):
    """A batch with ET - 6 VT = t: a chain longer than the graph-build forms take (so that the separate launches run and show the
    batch's form), a dense contig of surplus S = n (n + 1) - 6 (2 n + 1), and fan(a, m) (-5 a - 4 m - 12)."""
    L = 3600                                           # V = L + 2, E = L + 1: -5 L - 11
    n = 2
    while n * (n + 1) - 6 * (2 * n + 1) - 5 * L - 11 - 12 - t < 9:
        n += 1
    x = n * (n + 1) - 6 * (2 * n + 1) - 5 * L - 11 - 12 - t
    a = next(a for a in range(1, 5) if (x - 5 * a) % 4 == 0)
    return [("long", chain(L)), ("dense_%d" % n, _chain(1000, 10 ** 6, n, 900, -100, -100)), (f"ratio_{t}", fan(a, (x - 5 * a) // 4))]


def rev_ord_contigs(v):
    """A dense batch whose largest contig (a chain) has v vertices."""
    c = ("maxV_%d" % v, chain(v - 2))
    return [c, dense_filler(v + 43, v - 1 + 81), ("fan_40", fan(1, 40))]


def mw_contigs():
    return [(f"mw_V{v}_I{i}", shape_for(v, i + v - 1)) for v, i in MW_VI]


def tail_contigs():
    return pad(1600) + [(f"tail_{n}", chain(n)) for n in TAIL_N]


def grouped_contigs():
    """>= AASM_GROUPED_MIN contigs: the ring's fans two by two at indices 2k, 2k + 1 (one wave of the grouped sweep), 2-record
    contigs around them."""
    wide = ring_contigs()
    if len(wide) % 2:
        wide.append(("fan_33b", fan(3, 33)))
    out = pad(40)
    for i in range(0, len(wide), 2):
        out += wide[i:i + 2] + pad(6)
    return out + pad(GROUPED_MIN + 2 - len(out))


def batches():
    """{name: [(contig name, records)]}: every crafted batch of the capacity tests."""
    B = {"ring": ring_contigs(), "grouped": grouped_contigs(), "rows_sparse": row_contigs(), "heap": heap_contigs(),
         "gb": gb_contigs(), "mw": mw_contigs(), "tail": tail_contigs(), "ratio_0": ratio_contigs(0), "ratio_1": ratio_contigs(1)}
    rows = row_contigs()
    B["rows_dense"] = rows + [dense_filler(sum(2 * d + 8 for d in ROW_D), sum(4 * d + 4 for d in ROW_D))]
    for v in REV_ORD_V:
        B[f"rev_ord_{v}"] = rev_ord_contigs(v)
    return B


# ---- what the oracle says -----------------------------------------------------------------------------------------
def kahn(rowptr, col, reverse):
    """Replay of a sweep's queue (kb_rev_sweep / kb_fwd_sweep): sources in ascending id, then each popped vertex's in-list
    (reverse: ascending source, then row position) or row (forward), in list order.  -> (order, most entries waiting at once
    (tail - head, the popped one excluded), pops that find their entry outside the LDS window (the spill path))."""
    V = len(rowptr) - 1
    deg = np.diff(rowptr)
    src = np.repeat(np.arange(V), deg)
    if reverse:
        nxt = [[] for _ in range(V)]
        for e in range(len(col)):                      # edge ids ascend with (source, position): in-lists come out in list order
            nxt[col[e]].append(int(src[e]))
        cnt = deg.astype(np.int64).copy()
    else:
        nxt = [list(map(int, col[rowptr[v]:rowptr[v + 1]])) for v in range(V)]
        cnt = np.bincount(col, minlength=V).astype(np.int64)
    q = [v for v in range(V) if cnt[v] == 0]
    lds_hi = min(len(q), REVQ_N)
    head, occ, spills = 0, len(q), 0
    while head < len(q):
        if head >= lds_hi:
            spills += 1
        v = q[head]
        head += 1
        n0 = len(q)
        for u in nxt[v]:
            cnt[u] -= 1
            if cnt[u] == 0:
                q.append(u)
        nnew = len(q) - n0
        if lds_hi == n0:                               # the kernel's window bound (the slot of the entry at hand stays untouched)
            lds_hi += max(0, min(nnew, REVQ_N - 1 - (n0 - head)))
        occ = max(occ, len(q) - head)
    return q, occ, spills


def contig_facts(o):
    """From one contig's oracle intermediates: V, E, out / in-degrees, sidetracks per vertex, the two sweeps' replays."""
    rp, col = o["csr_rowptr"], o["csr_col"]
    V, E = len(rp) - 1, int(rp[-1])
    out = np.diff(rp)
    ind = np.bincount(col, minlength=V)
    best = o["sp_best"]
    st = out - (best >= 0)
    rq, rocc, rsp = kahn(rp, col, True)
    fq, focc, fsp = kahn(rp, col, False)
    assert np.array_equal(rq, o["rev_order"]) and np.array_equal(fq, o["fwd_order"]), "the replay's push order is not the sweeps'"
    # consecutive vertices of the heap wave's BFS order (the SP tree from dest, children in ascending id) - a vertex whose keys
    # are prefetched right after a row that went through the slot more than once
    kids = [[] for _ in range(V)]
    for u in range(V):
        if best[u] >= 0:
            kids[best[u]].append(u)
    bfs, i = [V - 1], 0
    while i < len(bfs):
        bfs += kids[bfs[i]]
        i += 1
    after_refill = [int(st[b]) for a, b in zip(bfs, bfs[1:]) if st[a] > 16 and st[b] > 0]
    return dict(V=V, E=E, I=max(0, E - (V - 1)), out=out, ind=ind, st=st, rev_occ=rocc, fwd_occ=focc, rev_spill=rsp,
                fwd_spill=fsp, after_refill=after_refill)


def facts(T, names, hb, K=4):
    """[(contig name, contig_facts)] of a batch (contigs of one record have no graph: None)."""
    off = hb.arrays["ctg_rec_off"]
    out = []
    for c, name in enumerate(names):
        if name == "pad" and c > 0 and names[c - 1] == "pad":
            out.append((name, out[-1][1]))             # (the 2-record filler: all alike)
            continue
        out.append((name, contig_facts(T.oracle_debug(hb, c, K)) if off[c + 1] - off[c] > 1 else None))
    return out


def batch_ratio(F):
    VT = sum(f["V"] for _, f in F if f)
    ET = sum(f["E"] for _, f in F if f)
    return VT, ET


def batch_facts(T, B=None):
    """{batch name: (names, HostBatch, [(contig name, contig_facts)])} of every crafted batch."""
    out = {}
    for bn, cl in (B or batches()).items():
        names, hb = batch(cl)
        out[bn] = (names, hb, facts(T, names, hb))
    return out


def coverage(T, BF=None):
    """Every target of the capacity tests, from the oracle's intermediates: -> (what each batch reaches, [targets missed])."""
    BF = BF or batch_facts(T)
    got, miss = {}, []

    def need(what, ok):
        if not ok:
            miss.append(what)

    def by_name(bn):
        return {n: f for n, f in BF[bn][2]}

    # 1 the sweeps' ring: the most entries waiting at once, in both sweeps, in the small batch (chain class / one wave a contig)
    # and in the grouped batch (two contigs a wave, each with its own ring: the wide ones at 2k, 2k + 1)
    for bn in ("ring", "grouped"):
        F = [f for n, f in BF[bn][2] if n != "pad"]
        got[bn] = {s: sorted({f[s + "_occ"] for f in F}) for s in ("rev", "fwd")}
        for s in ("rev", "fwd"):
            occ = got[bn][s]
            for m in RING_M[:-1]:
                need(f"{bn}: {s} queue at {m}", m in occ)
            need(f"{bn}: {s} queue >= 300", max(occ) >= 300)
            need(f"{bn}: {s} spill path", any(f[s + "_spill"] > 0 for f in F))
            need(f"{bn}: {s} at 31 without spill", any(f[s + "_occ"] == 31 and f[s + "_spill"] == 0 for f in F))
    names = BF["grouped"][0]
    wide = [i for i, n in enumerate(names) if n != "pad"]
    need("grouped: wide contigs pair up in waves", len(wide) % 2 == 0 and all(wide[i] % 2 == 0 and wide[i + 1] == wide[i] + 1
                                                                             for i in range(0, len(wide), 2)))
    need(f"grouped: >= {GROUPED_MIN} contigs", len(names) >= GROUPED_MIN)
    VT, ET = batch_ratio(BF["grouped"][2])
    need("grouped: sparse", ET <= 6 * VT)
    # 2 rows: out-degree (an ordinary vertex and src), in-degree, in a sparse and a dense batch
    for bn in ("rows_sparse", "rows_dense"):
        F = by_name(bn)
        got[bn] = dict(out=sorted({int(F[f"fan_{d}"]["out"].max()) for d in ROW_D}),
                       src=sorted({int(F[f"mirror_{d}"]["out"][F[f"mirror_{d}"]["V"] - 2]) for d in ROW_D}),
                       ind=sorted({int(F[f"fan_{d}"]["ind"].max()) for d in ROW_D}))
        for d in ROW_D:
            need(f"{bn}: out-degree {d}", d in got[bn]["out"])
            need(f"{bn}: src out-degree {d}", d in got[bn]["src"])
            need(f"{bn}: in-degree {d}", d in got[bn]["ind"])
        VT, ET = batch_ratio(BF[bn][2])
        need(f"{bn}: {'dense' if bn == 'rows_dense' else 'sparse'}", (ET > 6 * VT) == (bn == "rows_dense"))
    # 3 sidetracks per vertex, and a refilled row followed by the vertex whose keys were prefetched
    F = by_name("heap")
    got["heap"] = dict(st=sorted({int(f["st"].max()) for f in F.values()}), after_refill=sorted({s for f in F.values() for s in f["after_refill"]}))
    for s in HEAP_ST:
        need(f"heap: {s} sidetracks", s in got["heap"]["st"])
        if s > 16:
            need(f"heap: {s} sidetracks right after a refilled row", s in got["heap"]["after_refill"])
    # 4 the graph-build forms: (V, E) per contig, the other count at or below its limit
    F = by_name("gb")
    got["gb"] = {n: (f["V"], f["E"]) for n, f in F.items()}
    for v in GB_V:
        V, E = got["gb"][f"gbV_{v}"]
        need(f"gb: V = {v}", V == v and E <= (4096 if v <= 1792 else 8192))
    for e in GB_E:
        V, E = got["gb"][f"gbE_{e}"]
        need(f"gb: E = {e}", E == e and V <= (1792 if e <= 4096 else 3584))
    VT, ET = batch_ratio(BF["gb"][2])
    need("gb: sparse", ET <= 6 * VT)
    # 5 the dense batch's largest contig
    for v in REV_ORD_V:
        F = BF[f"rev_ord_{v}"][2]
        VT, ET = batch_ratio(F)
        got[f"rev_ord_{v}"] = (max(f["V"] for _, f in F), ET - 6 * VT)
        need(f"rev_ord: max V = {v}, dense", got[f"rev_ord_{v}"][0] == v and ET > 6 * VT)
    # 6 the batch ratio
    for t in (0, 1):
        VT, ET = batch_ratio(BF[f"ratio_{t}"][2])
        got[f"ratio_{t}"] = ET - 6 * VT
        need(f"ratio: ET = 6 VT + {t}", ET - 6 * VT == t)
    # 7 the classes
    F = by_name("mw")
    got["mw"] = {n: (f["V"], f["I"]) for n, f in F.items()}
    for v, i in MW_VI:
        need(f"mw: V = {v}, I = {i}", got["mw"][f"mw_V{v}_I{i}"] == (v, i))
    names, hb, F = BF["tail"]
    N = np.diff(hb.arrays["ctg_rec_off"])
    got["tail"] = (len(names), int(N.sum()) // len(names), [int(N[names.index(f"tail_{n}")]) for n in TAIL_N])
    need("tail: > 1 536 contigs, 4 x mean < 2 048", len(names) > 1536 and 4 * (int(N.sum()) // len(names)) < 2048)
    need("tail: 2 047 / 2 048 records", got["tail"][2] == list(TAIL_N))
    VT, ET = batch_ratio(F)
    need("tail: sparse", ET <= 6 * VT)
    return got, miss


def ring_spills(T, batches_, K=4):
    """Over [HostBatch]: (contigs with a graph, contigs whose reverse or forward sweep takes the ring's spill path, the most
    entries waiting at once anywhere)."""
    n = n_spill = top = 0
    for hb in batches_:
        off = hb.arrays["ctg_rec_off"]
        for c in range(len(off) - 1):
            if off[c + 1] - off[c] <= 1:
                continue
            f = contig_facts(T.oracle_debug(hb, c, K))
            n += 1
            n_spill += int(f["rev_spill"] > 0 or f["fwd_spill"] > 0)
            top = max(top, f["rev_occ"], f["fwd_occ"])
    return n, n_spill, top
