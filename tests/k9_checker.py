"""A third, independent reading of K9's path upgrade (reference: /root/reference/src/paf_data.cpp:750-792 `internal_shortest_path_recover`,
:795-921 `upgrade_edge_path_with_alt_path`) - plain Python, own shape, shares no code with oracle/ or with the product.

Why it exists: `paf_data.cpp:739+` cannot be compiled in this image (ankerl/unordered_dense.h is absent), so K9 is the one
stage for which "HIP == oracle" does not mean "== reference" (DESIGN.md section 2).  This module does NOT pin K9 to the reference
either; it is one more reading of the same source text, written differently, plus two things a reading cannot get wrong:

  * EXHAUSTIVE minimality: for every window DP whose window holds at most `brute_max` vertices, every a -> b path inside the
    window is enumerated (with the whitelist rule on the last hop), and no enumerated path may be smaller under the
    QRY_SCORE_MODE order (paf_data.hpp:142-159) than the path the product took; the product's path must be one of the enumerated
    ones and its distance the minimum;
  * the reference's own Debug asserts on the upgraded path (:913-918): first tail = src, last head = dest, consecutive edges
    chained, every edge an edge of the graph.

Inputs are the product's (or the emulation's) intermediates: the CSR graph, the forward Kahn order, the walk as recovered
from the heaps (`pathA`) and the upgraded path (`pathB`).  Everything up to `pathA` is pinned to the reference (K1 ... K8).

The second half reads the conversion and the selection (:1489-1649) the same way - `plan`, `walk_ok`, `convert`, `select`,
`contig_outputs`, `batch_findings` - and rebuilds every contig's main, alt and `.all` rows from the pinned intermediates
(sorted order, vertex ids, pair cut tables, the K distances, anom_dis[dest], the CSR), the batch's input records and the walks.
The product's own conclusions (cv_k, cv_kind, cv_cov, cv_out, mark_time, main_len) are never inputs; cv_k / cv_kind / cv_ord
are only compared with, to say where a finding sits."""
import numpy as np

# a K-path distance as the debug arrays hold it (PafDistance, paf_data.hpp:121-189: qry_score, ref_score, anom, qul_nonzero,
# qul_total), and an output row (PafOutputData, paf_data.hpp:86-105)
DIST_DT = np.dtype([("qry", np.int64), ("ref", np.int64), ("anom", np.int32), ("qnz", np.int32), ("qtot", np.int32), ("pad", np.int32)])
ROW_DT = np.dtype([("qs", np.int64), ("qe", np.int64), ("rs", np.int64), ("re", np.int64), ("ctg_index", np.int32), ("is_alt", np.int32)])


class Dist:
    """PafDistance (paf_data.hpp:121-189) as a tuple with the QRY_SCORE_MODE order."""
    __slots__ = ("q", "r", "a", "nz", "tot")

    def __init__(self, q=0, r=0, a=0, nz=0, tot=0):
        self.q, self.r, self.a, self.nz, self.tot = q, r, a, nz, tot

    def __add__(self, o):
        return Dist(self.q + o.q, self.r + o.r, self.a + o.a, self.nz + o.nz, self.tot + o.tot)

    def less_qry(self, o):
        """operator< in QRY_SCORE_MODE for two real distances (neither is max())."""
        if self.q != o.q:
            return self.q < o.q
        if self.r != o.r:
            return self.r < o.r
        if self.a != o.a:
            return self.a < o.a
        return self.nz * (o.tot or 1) > o.nz * (self.tot or 1)

    def key(self):
        return (self.q, self.r, self.a, self.nz, self.tot)


class Graph:
    """One contig's graph from the product's arrays (local vertex ids; src = V - 2, dest = V - 1)."""

    def __init__(self, rowptr, col, wq, wr, fl, v_i, v_j, fwd_order):
        self.V = len(rowptr) - 1
        self.rowptr, self.col, self.wq, self.wr, self.fl = rowptr, col, wq, wr, fl
        self.v_i, self.v_j = v_i, v_j
        self.order = fwd_order                                        # position -> vertex
        self.pos = np.empty(self.V, np.int64)
        self.pos[fwd_order] = np.arange(self.V)
        self.src, self.dest = self.V - 2, self.V - 1

    def out(self, u):
        for e in range(int(self.rowptr[u]), int(self.rowptr[u + 1])):
            f = int(self.fl[e])
            yield int(self.col[e]), Dist(int(self.wq[e]), int(self.wr[e]), f & 3, (f >> 2) & 1, (f >> 3) & 1)

    def has_edge(self, u, v):
        return v in self.col[int(self.rowptr[u]):int(self.rowptr[u + 1])]

    def edge_ids(self, us, vs):
        """Edge index of every (us[t], vs[t]), -1 where there is none (the first of parallel edges, if any)."""
        if not hasattr(self, "_skey"):
            rows = np.repeat(np.arange(self.V, dtype=np.int64), np.diff(self.rowptr).astype(np.int64))
            key = rows * self.V + self.col
            self._eord = np.argsort(key, kind="stable")
            self._skey = key[self._eord]
            self.parallel = bool((np.diff(self._skey) == 0).any())
        kk = np.asarray(us, np.int64) * self.V + np.asarray(vs, np.int64)
        pos = np.minimum(np.searchsorted(self._skey, kk), max(len(self._skey) - 1, 0))
        hit = (self._skey[pos] == kk) if len(self._skey) else np.zeros(len(kk), bool)
        return np.where(hit, self._eord[pos] if len(self._skey) else -1, -1)


def _hop_allowed(g, u, v, b, wl):
    """:767-773: with a whitelist the hop INTO b must come from a record vertex whose second index is the whitelisted record."""
    if wl is None or v != b:
        return True
    if u == g.src or u == g.dest:
        return False
    return int(g.v_j[u]) == wl


def window_dp(g, a, b, wl=None):
    """internal_shortest_path_recover (:750-792) as written: first-wins relaxation over the forward order.  Returns the vertex list
    a ... b ([] when a == b) and the distance of b."""
    if a == b:
        return [], None
    dist, pre = {a: Dist()}, {a: -1}
    for p in range(int(g.pos[a]), int(g.pos[b])):
        u = int(g.order[p])
        if u not in dist:
            continue
        du = dist[u]
        for v, w in g.out(u):
            if not _hop_allowed(g, u, v, b, wl):
                continue
            nd = du + w
            if v not in dist or nd.less_qry(dist[v]):
                dist[v], pre[v] = nd, u
    assert b in dist, "window DP: b unreachable (the reference's Debug assert :783)"
    path, x = [b], b
    while x != a:
        x = pre[x]
        path.append(x)
    return path[::-1], dist[b]


def enumerate_paths(g, a, b, wl=None, limit=200000):
    """Every a -> b path (a DAG: all of them stay inside the window of topological positions); None when there are more than
    `limit`, or when more than 4 * limit + 1000 prefixes had to be visited (prefixes that the whitelist never lets reach b are
    work too): None means too many paths OR too much work."""
    out, stack = [], [(a, [a], Dist())]
    pb = int(g.pos[b])
    steps = 0
    while stack:
        u, path, d = stack.pop()
        steps += 1
        if steps > 4 * limit + 1000:
            return None
        for v, w in g.out(u):
            if int(g.pos[v]) > pb or not _hop_allowed(g, u, v, b, wl):
                continue
            if v == b:
                out.append((path + [v], d + w))
                if len(out) > limit:
                    return None
            else:
                stack.append((v, path + [v], d + w))
    return out


def check_conversion(g, pathA, pathB, brute_max=12, stats=None):
    """pathA / pathB: lists of (u, v) edges (the walk from the heaps / the product's upgraded path).  Returns a list of findings
    (empty = fine).  Follows :801-912 edge by edge, computing every alt path with `window_dp`; wherever the window is small,
    the result is also checked against the exhaustive enumeration."""
    bad = []
    stats = stats if stats is not None else {}
    src, dest = g.src, g.dest
    # ---- the reference's asserts on the result (:913-918) + every edge exists
    if not pathB or pathB[0][0] != src or pathB[-1][1] != dest:
        return ["upgraded path does not run src -> dest"]
    for (u0, v0), (u1, v1) in zip(pathB, pathB[1:]):
        if v0 != u1:
            bad.append("upgraded path is not chained at %d -> %d | %d -> %d" % (u0, v0, u1, v1))
    for u, v in pathB:
        if not g.has_edge(u, v):
            bad.append("upgraded path uses %d -> %d, which is not an edge" % (u, v))
    if bad:
        return bad
    # ---- this reading's own upgrade of pathA
    mine = []                                                         # vertex pairs

    def alt(a, b, wl, drop_last, fallback):
        vs, d = window_dp(g, a, b, wl)
        if not vs:
            mine.extend(fallback)
            return
        nwin = int(g.pos[b]) - int(g.pos[a]) + 1
        stats["dp"] = stats.get("dp", 0) + 1
        win = None
        if "windows" in stats:                                        # one record per window DP, in call order (tests/k9_cases.py)
            pa = int(g.pos[a])
            rows = g.order[pa:pa + nwin - 1]                          # whole rows of the positions [pa, pa + W), as the kernel's forms count them
            win = dict(a=a, b=b, wl=wl, pa=pa, W=nwin - 1, E=int((g.rowptr[rows + 1] - g.rowptr[rows]).sum()), it=it, out_len=len(mine),
                       drop_last=drop_last, own=list(own_edges), res=list(zip(vs, vs[1:])), paths=None, ndist=None, skipped=False)
            win["differs"] = win["res"] != win["own"]
            stats["windows"].append(win)
        if nwin <= brute_max:
            allp = enumerate_paths(g, a, b, wl, limit=stats.get("path_limit", 200000))
            if allp is None and win is not None:
                win["skipped"] = True
            if allp is not None:
                if win is not None:
                    win["paths"], win["ndist"] = len(allp), len({dd.key() for _, dd in allp})
                stats["brute"] = stats.get("brute", 0) + 1
                stats["brute_paths"] = stats.get("brute_paths", 0) + len(allp)
                if vs not in [p for p, _ in allp]:
                    bad.append("window %d -> %d: the DP's path is not an a -> b path of the graph" % (a, b))
                for p, dd in allp:
                    if dd.less_qry(d):
                        bad.append("window %d -> %d (wl %r): path %r is smaller than the DP's %r" % (a, b, wl, p, vs))
                        break
                best = min(allp, key=lambda t: (t[1].q, t[1].r, t[1].a))
                if (best[1].q, best[1].r, best[1].a) != (d.q, d.r, d.a):
                    bad.append("window %d -> %d: DP distance %r is not the minimum %r" % (a, b, d.key(), best[1].key()))
        es = list(zip(vs, vs[1:]))
        if drop_last:
            es = es[:-1]
        mine.extend(es)

    it, n = 0, len(pathA)
    own_edges = []                                                    # the walk's edges the step at hand replaces (the window records read it)
    if n < 2 or pathA[0][0] != src or pathA[-1][1] != dest:
        return ["walk does not run src -> dest"]
    while it < n:
        u, v = pathA[it]
        own_edges[:] = pathA[it:it + 1] if v == dest and u != src else pathA[it:it + 2]
        if u == src or (v != dest and int(g.v_i[v]) == int(g.v_j[v])):
            cont = src if u == src else mine[-1][1]
            y = int(g.v_j[v])
            if u == src and not (int(g.v_i[v]) == y and v != dest):
                return ["walk starts with src -> %d, not a record vertex" % v]
            nu, nv = pathA[it + 1]
            if nu != v:
                return ["walk not chained at edge %d" % it]
            if nv == dest or int(g.v_i[nv]) == int(g.v_j[nv]):
                alt(cont, nv, y, True, [(u, v)])
            else:
                alt(cont, nv, None, False, [(u, v), (nu, nv)])
                it += 1
        elif v == dest:
            cont = mine[-1][1]
            alt(cont, v, None, False, [])
        else:                                                         # v = (x, y), x != y: the edge stays (:866-873)
            mine.append((u, v))
        it += 1
    if mine != list(pathB):
        k = next((i for i, (x, y) in enumerate(zip(mine, pathB)) if x != y), min(len(mine), len(pathB)))
        bad.append("upgraded path differs from this reading at edge %d: product %r, here %r (lengths %d / %d)" % (
            k, pathB[k] if k < len(pathB) else None, mine[k] if k < len(mine) else None, len(pathB), len(mine)))
    return bad


def chain_invariants_batch(voff, ctgV, rowptr, col, cv_ctg, cv_roff, cv_la, cv_path, rec_off, R0=0):
    """The asserts of :913-918 on EVERY conversion of a batch, vectorised enough for C3 / the C5 share: returns (#conversions
    checked, #edges checked, list of findings)."""
    bad, nedges = [], 0
    for j in range(len(cv_ctg)):
        la = int(cv_la[j])
        if la <= 0:
            bad.append("conversion %d: no walk" % j)
            continue
        c = int(cv_ctg[j])
        N = int(rec_off[c + 1] - rec_off[c])
        cap = N + 2
        base = 6 * int(cv_roff[j]) + 2 * cap
        pb = cv_path[base: base + 2 * cap].reshape(-1, 2)
        V = int(ctgV[c])
        ends = np.nonzero(pb[:, 1] == V - 1)[0]
        if pb[0, 0] != V - 2 or len(ends) == 0:
            bad.append("conversion %d (contig %d): upgraded path does not run src -> dest" % (j, c))
            continue
        lb = int(ends[0]) + 1
        pb = pb[:lb].astype(np.int64)
        if not (pb[1:, 0] == pb[:-1, 1]).all():
            bad.append("conversion %d (contig %d): upgraded path not chained" % (j, c))
        vb = int(voff[c])
        r0, r1 = rowptr[vb + pb[:, 0]], rowptr[vb + pb[:, 0] + 1]
        for t in range(lb):                                           # rows are short on sparse graphs; dense rows: one vectorised test per edge
            if not (col[int(r0[t]):int(r1[t])] == pb[t, 1]).any():
                bad.append("conversion %d (contig %d): %d -> %d is not an edge" % (j, c, pb[t, 0], pb[t, 1]))
                break
        nedges += lb
    return len(cv_ctg), nedges, bad


def collect(fetch, rec_off, full=False, K=None):
    """The arrays this checker reads, through `fetch(name, dtype)` (DeviceResult.debug of a keep_debug solve, or the emulation's
    fetch); `full` adds what `batch_findings` reads (K = the solve's max_paths).  Returns a dict; `graph_of(arr, c)` / `conversions_of(arr, c)` cut one contig out of it."""
    a = {"rec_off": np.asarray(rec_off, np.int64)}
    C = len(a["rec_off"]) - 1
    a["voff"] = fetch("voff", np.int64)[:C + 1]
    a["ctgV"] = fetch("ctgV", np.int32)[:C]
    VT = int(a["voff"][C])
    a["rowptr"] = fetch("csr_rowptr", np.int64)[:VT + 1]
    ET = int(a["rowptr"][VT]) if VT else 0
    a["col"] = fetch("csr_col", np.int32)[:ET]
    a["wq"] = fetch("csr_w_qry", np.int64)[:ET]
    a["wr"] = fetch("csr_w_ref", np.int32)[:ET]
    a["fl"] = fetch("csr_w_flags", np.uint8)[:ET]
    a["v_i"] = fetch("v_i", np.int32)[:VT]
    a["v_j"] = fetch("v_j", np.int32)[:VT]
    a["fwd_order"] = fetch("fwd_order", np.int32)[:VT]
    a["conv_off"] = fetch("conv_off", np.int64)[:C + 1]
    NCONV = int(a["conv_off"][C])
    a["cv_ctg"] = fetch("cv_ctg", np.int32)[:NCONV]
    a["cv_roff"] = fetch("cv_roff", np.int64)[:NCONV + 1]
    a["cv_la"] = fetch("cv_la", np.int32)[:NCONV]
    a["cv_path"] = fetch("cv_path", np.int32)
    if full:                                                          # what the conversion / selection reading needs
        R = int(a["rec_off"][C])
        a["perm"] = fetch("perm", np.int32)[:R]
        a["v_slot"] = fetch("v_slot", np.int64)[:VT]
        for k in ("ov_peq", "ov_per", "ov_stq", "ov_str"):
            a[k] = fetch(k, np.int64)
        a["kfound"] = fetch("kfound", np.int32)[:C]
        a["K"] = int(K)
        a["kd"] = fetch("kd", DIST_DT)[:C * a["K"]]
        a["anom_dest"] = fetch("anom_dest", np.int32)[:C]
        for k in ("cv_k", "cv_kind", "cv_ord"):                       # compared with only
            a[k] = fetch(k, np.int32)[:NCONV]
    return a


def graph_of(a, c):
    vb, V = int(a["voff"][c]), int(a["ctgV"][c])
    rp = a["rowptr"][vb:vb + V + 1]
    e0, e1 = int(rp[0]), int(rp[-1])
    return Graph(rp - e0, a["col"][e0:e1], a["wq"][e0:e1], a["wr"][e0:e1], a["fl"][e0:e1], a["v_i"][vb:vb + V], a["v_j"][vb:vb + V],
                 a["fwd_order"][vb:vb + V].astype(np.int64))


def conversions_of(a, c, as_arrays=False):
    """[(pathA, pathB)] of contig c, in conversion order; paths as lists of (u, v) (or (n, 2) int64 arrays)."""
    out = []
    N = int(a["rec_off"][c + 1] - a["rec_off"][c])
    cap = N + 2
    V = int(a["ctgV"][c])
    for j in range(int(a["conv_off"][c]), int(a["conv_off"][c + 1])):
        la = int(a["cv_la"][j])
        base = 6 * int(a["cv_roff"][j])
        pa = a["cv_path"][base: base + 2 * la].reshape(-1, 2)
        pb = a["cv_path"][base + 2 * cap: base + 4 * cap].reshape(-1, 2)
        ends = np.nonzero(pb[:, 1] == V - 1)[0]
        lb = int(ends[0]) + 1 if len(ends) else 0
        if as_arrays:
            out.append((pa.astype(np.int64), pb[:lb].astype(np.int64)))
        else:
            out.append(([(int(u), int(v)) for u, v in pa], [(int(u), int(v)) for u, v in pb[:lb]]))
    return out


# ---- conversion and selection (paf_data.cpp:1489-1649) -------------------------------------------------------------------------
# Branch counters, summed over whatever a test feeds in, so that a test can assert its inputs reach every branch:
COUNTERS = (
    "tie_run",               # a tie run longer than path 0 alone (:1596)
    "main_from_tie",         # main is a tie path, not path 0 (:1603-1606)
    "all_cleared",           # `.all` cleared while non-empty (:1606)
    "all_nonempty",          # `.all` non-empty at the end
    "k2_superseded",         # a new best ratio replacing an earlier one (:1625)
    "k3_converted",          # a walk at the current best's distance converted (:1636)
    "k3_replaced",           # ... and taking over the alt pick (:1641-1644)
    "k3_equal_cov",          # ... with coverage equal to the pick's (not taken)
    "alt_skipped_anom",      # no alt scan because min.anom == anom_dis[dest] (:1615)
    "alt_marked_later",      # an output row flagged alt whose record only a LATER conversion's walk marks
    "alt_never_marked",      # an output row flagged alt whose record no walk of the contig touches (the upgrade brought it in)
    "kept_by_earlier_mark",  # an output row not flagged although its own walk never touches it (an earlier conversion marked it)
    "clip_start",            # an output row whose start the pair cut tables changed
    "clip_end",              # an output row whose end the pair cut tables changed
)
I64 = 1 << 63
NO_MARK = 1 << 62


def _bump(stats, k, n=1):
    if stats is not None:
        stats[k] = stats.get(k, 0) + n


def plan(kd, found, anom_dest, stats=None):
    """The walks the reference converts, in call order, as [(k, kind)]: kind 0 = path 0 (:1589), 1 = the tie run (:1596-1611:
    score_sum and anom equal to path 0's, is_equal_paf_distance :1581-1583), 2 = a new best Δscore / Δanom ratio (:1625-1635),
    3 = a walk whose distance equals the current best's (:1636-1646).  The alt scan needs two distances or more and
    min.anom != anom_dis[dest] (:1615), and skips every walk without fewer anomalies (:1621).  The ratio test is the reference's
    int64 cross-multiplication, done here in Python ints: a product outside int64 is a finding, never an agreement.
    Returns (plan, findings)."""
    q, r, an = kd["qry"][:found].tolist(), kd["ref"][:found].tolist(), kd["anom"][:found].tolist()
    s0, a0 = q[0] + r[0], an[0]
    out, bad = [(0, 0)], []
    i = 1
    while i < found and q[i] + r[i] == s0 and an[i] == a0:
        out.append((i, 1))
        i += 1
    if i > 1:
        _bump(stats, "tie_run")
    if found >= 2 and a0 == anom_dest:
        _bump(stats, "alt_skipped_anom")
    elif found >= 2:
        ans_idx, ans_up, ans_down, n2 = -1, 0, 0, 0
        for i in np.nonzero(np.asarray(kd["anom"][:found]) < a0)[0].tolist():
            up, down = q[i] + r[i] - s0, a0 - an[i]
            lhs, rhs = up * ans_down, down * ans_up
            if not (-I64 <= lhs < I64 and -I64 <= rhs < I64):
                bad.append("alt scan at walk %d: %d * %d vs %d * %d leaves int64" % (i, up, ans_down, down, ans_up))
            if ans_idx == -1 or lhs < rhs:
                ans_idx, ans_up, ans_down = i, up, down
                out.append((i, 2))
                n2 += 1
            elif q[i] + r[i] == q[ans_idx] + r[ans_idx] and an[i] == an[ans_idx]:
                out.append((i, 3))
                _bump(stats, "k3_converted")
        _bump(stats, "k2_superseded", max(0, n2 - 1))
    return out, bad


def walk_ok(g, pathA, d):
    """The walk recovered for distance d as the reference asserts it (:1497-1499: src first, dest last), chained, every edge an
    edge of the graph - and the five weight fields of its edges summing to d: recovery returned walk k (up to walks of equal
    distance), not merely some src -> dest walk.  Returns findings."""
    pa = np.asarray(pathA, np.int64).reshape(-1, 2)
    if len(pa) < 2:
        return ["walk has %d edges" % len(pa)]
    bad = []
    if pa[0, 0] != g.src or pa[-1, 1] != g.dest:
        bad.append("walk runs %d -> %d, not src -> dest" % (pa[0, 0], pa[-1, 1]))
    if not (pa[1:, 0] == pa[:-1, 1]).all():
        bad.append("walk is not chained")
    e = g.edge_ids(pa[:, 0], pa[:, 1])
    if (e < 0).any():
        t = int(np.nonzero(e < 0)[0][0])
        return bad + ["walk uses %d -> %d, which is not an edge" % (pa[t, 0], pa[t, 1])]
    fl = g.fl[e].astype(np.int64)
    got = (int(g.wq[e].astype(np.int64).sum()), int(g.wr[e].astype(np.int64).sum()), int((fl & 3).sum()), int(((fl >> 2) & 1).sum()),
           int(((fl >> 3) & 1).sum()))
    want = (int(d["qry"]), int(d["ref"]), int(d["anom"]), int(d["qnz"]), int(d["qtot"]))
    if got != want:
        bad.append("walk weighs %r, its distance is %r%s" % (got, want, " (graph has parallel edges)" if g.parallel else ""))
    return bad


class Contig:
    """What the conversion of one contig reads: its graph, the pair cut table slot of each pair vertex (v_slot), the batch's cut
    tables (edited_loc_str / edited_loc_pre_end: ov_stq / ov_str / ov_peq / ov_per) and its records in sorted order
    (paf_ctg_data_sorted: the input records through perm, ctg_index = the record's index in its contig)."""

    def __init__(self, a, inp, c):
        b0, b1 = int(a["rec_off"][c]), int(a["rec_off"][c + 1])
        self.N = b1 - b0
        self.g = graph_of(a, c)
        vb = int(a["voff"][c])
        self.slot = a["v_slot"][vb:vb + self.g.V]
        self.ov = a
        perm = a["perm"][b0:b1].astype(np.int64)
        gi = b0 + perm
        self.rec = np.zeros(self.N, ROW_DT)
        for f, k in (("qs", "qry_str"), ("qe", "qry_end"), ("rs", "ref_str"), ("re", "ref_end")):
            self.rec[f] = inp[k][gi]
        self.rec["ctg_index"] = perm


def convert(ct, pathA, pathB, marks, ordinal):
    """edge_path_to_paf_path (:1489-1568) as conversion number `ordinal` of its contig.  marks (int64, keyed by ctg_index, one per
    contig for all its conversions: not_alt_vertex_map) holds the first conversion that marked each record.
    1) :1490-1496: mark x and y of every head v != dest of the UN-upgraded walk;
    2) :1502-1557: walk the upgraded path with the reference's case split - (u == src) a record vertex, whole; (v == dest)
       nothing; (x1 == x2, y1 == y2) record y, whole; (x1 == x2, y1 != y2) record y2, its start from edited_loc_str[y1][y2] and
       the previous row's end from edited_loc_pre_end[y1][y2]; (x1 != x2, y1 == y2) record y2, whole; (x1 != x2, y1 != y2)
       record y2, clipped as the second case by the pair (x2, y2) = (y1, y2);
    3) :1560-1566: a row is alt unless its record carries a mark.
    Returns (dict(rows, cov, own, clip_s, clip_e) or None, findings); cov = get_total_coverage (:1571-1579)."""
    g = ct.g
    pa = np.asarray(pathA, np.int64).reshape(-1, 2)
    hv = pa[:, 1][pa[:, 1] != g.dest]
    own = np.zeros(ct.N, bool)
    for x in (g.v_i[hv], g.v_j[hv]):
        ci = ct.rec["ctg_index"][x]
        own[ci] = True
        marks[ci] = np.minimum(marks[ci], ordinal)
    pb = np.asarray(pathB, np.int64).reshape(-1, 2)
    n = len(pb) - 1
    if n < 1 or pb[0, 0] != g.src or pb[-1, 1] != g.dest or (pb[:-1, 1] == g.dest).any() or (pb[1:, 0] == g.src).any():
        return None, ["upgraded path is not src -> ... -> dest"]
    u, v = pb[:n, 0], pb[:n, 1]
    from_src = u == g.src
    uu = np.where(from_src, v, u)
    x1, x2 = g.v_i[uu].astype(np.int64), g.v_j[uu].astype(np.int64)
    y1, y2 = g.v_i[v].astype(np.int64), g.v_j[v].astype(np.int64)
    u_rec, v_rec = (x1 == x2) | from_src, y1 == y2
    bad = []
    if not v_rec[0]:
        bad.append(":1507 src -> a pair vertex")
    clip = ~v_rec & ~from_src                                         # (x1 == x2, y1 != y2) and (x1 != x2, y1 != y2)
    if (x2[clip] != y1[clip]).any():
        bad.append(":1520 / :1541 a pair vertex that does not continue its predecessor's record")
    pr = ~u_rec & v_rec
    if (x2[pr] == y2[pr]).any():
        bad.append(":1533 a pair vertex followed by its own second record")
    rows = ct.rec[y2].copy()
    t = np.nonzero(clip)[0]
    sl = ct.slot[v[t]]
    rows["qs"][t], rows["rs"][t] = ct.ov["ov_stq"][sl], ct.ov["ov_str"][sl]
    rows["qe"][t - 1], rows["re"][t - 1] = ct.ov["ov_peq"][sl], ct.ov["ov_per"][sl]
    if (rows["qs"] > rows["qe"]).any():
        bad.append(":1561 a row with edited_qry_str > edited_qry_end")
    rows["is_alt"] = marks[rows["ctg_index"]] > ordinal
    cov = int((rows["qe"] - rows["qs"]).sum()) + int(np.abs(rows["re"] - rows["rs"]).sum())
    whole = ct.rec[y2]
    return dict(rows=rows, cov=cov, own=own, clip_s=(rows["qs"] != whole["qs"]) | (rows["rs"] != whole["rs"]),
                clip_e=(rows["qe"] != whole["qe"]) | (rows["re"] != whole["re"])), bad


def select(kinds, covs, stats=None):
    """:1585-1649 over the converted walks (their kinds and coverages, in call order) -> (main, alt or -1, [.all]) as indices.
    Path 0 is main to begin with; a tie walk with strictly larger coverage takes over and clears `.all`, one with equal coverage
    is appended (path 0 never is).  The alt: a kind 2 takes over and resets the running coverage; a kind 3 only with strictly
    larger coverage."""
    main, best, allp = 0, covs[0], []
    for t, kind in enumerate(kinds):
        if kind != 1:
            continue
        if covs[t] > best:
            if allp:
                _bump(stats, "all_cleared")
            main, best, allp = t, covs[t], []
        elif covs[t] == best:
            allp.append(t)
    if main:
        _bump(stats, "main_from_tie")
    if allp:
        _bump(stats, "all_nonempty")
    alt, best = -1, -1
    for t, kind in enumerate(kinds):
        if kind == 2:
            alt, best = t, covs[t]
        elif kind == 3 and covs[t] > best:
            alt, best = t, covs[t]
            _bump(stats, "k3_replaced")
        elif kind == 3 and covs[t] == best:
            _bump(stats, "k3_equal_cov")
    return main, alt, allp


def contig_outputs(a, inp, c, walks, stats=None):
    """One contig's rows: dict(main, alt, all = [rows], ok = False when the contig must have a nonzero status, plan, convs, pick),
    and findings.  `walks` = [(pathA, pathB)] in conversion order (the product's recovery and upgrade).  A single record is one
    whole row with ctg_index 0 (:235-239); a contig without a k-path distance has no rows (:732)."""
    none = np.zeros(0, ROW_DT)
    res = dict(main=none, alt=none, all=[], ok=True, plan=[], convs=[], pick=None)
    b0, b1 = int(a["rec_off"][c]), int(a["rec_off"][c + 1])
    N = b1 - b0
    if N == 0:
        return res, []
    if N == 1:
        row = np.zeros(1, ROW_DT)
        for f, k in (("qs", "qry_str"), ("qe", "qry_end"), ("rs", "ref_str"), ("re", "ref_end")):
            row[f] = inp[k][b0]
        res["main"] = row
        return res, []
    found, K = int(a["kfound"][c]), a["K"]
    if int(a["ctgV"][c]) == 0 or found <= 0:
        res["ok"] = False
        return res, []
    kd = a["kd"][c * K:c * K + found]
    pl, bad = plan(kd, found, int(a["anom_dest"][c]), stats)
    res["plan"] = pl
    if "cv_k" in a:
        j0, j1 = int(a["conv_off"][c]), int(a["conv_off"][c + 1])
        theirs = list(zip(a["cv_k"][j0:j1].tolist(), a["cv_kind"][j0:j1].tolist()))
        if theirs != pl or a["cv_ord"][j0:j1].tolist() != list(range(j1 - j0)):
            k = next((i for i, (x, y) in enumerate(zip(pl, theirs)) if x != y), min(len(pl), len(theirs)))
            return res, ["plan differs at conversion %d: product %r, here %r (lengths %d / %d)" % (
                k, theirs[k] if k < len(theirs) else None, pl[k] if k < len(pl) else None, len(theirs), len(pl))]
    if len(walks) != len(pl):
        return res, bad + ["%d walks for %d planned conversions" % (len(walks), len(pl))]
    ct = Contig(a, inp, c)
    marks = np.full(N, NO_MARK, np.int64)
    for t, ((k, kind), (pa, pb)) in enumerate(zip(pl, walks)):
        bad += ["conversion %d (walk %d): %s" % (t, k, x) for x in walk_ok(ct.g, pa, kd[k])]
        cv, b = convert(ct, pa, pb, marks, t)
        bad += ["conversion %d (walk %d): %s" % (t, k, x) for x in b]
        if cv is None:
            return res, bad
        res["convs"].append(cv)
    main, alt, allp = select([k for _, k in pl], [cv["cov"] for cv in res["convs"]], stats)
    res["pick"] = (main, alt, allp)
    res["main"] = res["convs"][main]["rows"]
    res["alt"] = res["convs"][alt]["rows"] if alt >= 0 else none
    res["all"] = [res["convs"][t]["rows"] for t in allp]
    if stats is not None:
        for t in [main] + ([alt] if alt >= 0 else []) + allp:
            cv = res["convs"][t]
            rows = cv["rows"]
            m = marks[rows["ctg_index"]]
            isalt = rows["is_alt"] != 0
            _bump(stats, "alt_marked_later", int((isalt & (m < NO_MARK)).sum()))
            _bump(stats, "alt_never_marked", int((isalt & (m == NO_MARK)).sum()))
            _bump(stats, "kept_by_earlier_mark", int((~isalt & ~cv["own"][rows["ctg_index"]]).sum()))
            _bump(stats, "clip_start", int(cv["clip_s"].sum()))
            _bump(stats, "clip_end", int(cv["clip_e"].sum()))
    return res, bad


def _rows_diff(want, got):
    if len(want) != len(got):
        return "%d rows, expected %d" % (len(got), len(want))
    for f in ROW_DT.names:
        d = np.nonzero(np.asarray(want[f], np.int64) != np.asarray(got[f], np.int64))[0]
        if len(d):
            return "row %d: %s = %d, expected %d" % (d[0], f, got[f][d[0]], want[f][d[0]])
    return None


def batch_findings(out, a, inp, walks_of, stats=None, contigs=None):
    """Every contig's main / alt / .all rows rebuilt and compared with the product's output `out` (main, alt, all, status and the
    four offset arrays).  a = collect(..., full=True); inp = the batch's input arrays; walks_of(c) = [(pathA, pathB)] of contig c.
    Returns (findings, per-contig results)."""
    C = len(a["rec_off"]) - 1
    bad, per = [], {}
    lens = {"main": np.zeros(C, np.int64), "alt": np.zeros(C, np.int64)}
    all_paths, all_lens = np.zeros(C, np.int64), []
    for c in range(C):
        res, b = contig_outputs(a, inp, c, walks_of(c) if int(a["rec_off"][c + 1] - a["rec_off"][c]) > 1 and int(a["ctgV"][c]) else [], stats)
        bad += ["contig %d: %s" % (c, x) for x in b]
        per[c] = res
        st = int(out["status"][c])
        if res["ok"] == (st != 0):
            bad.append("contig %d: status %d, expected %s" % (c, st, "0" if res["ok"] else "nonzero"))
        for key in ("main", "alt"):
            lens[key][c] = len(res[key])
            o = out[key + "_off"]
            if c + 1 < len(o):
                d = _rows_diff(res[key], out[key][int(o[c]):int(o[c + 1])])
                if d:
                    bad.append("contig %d %s: %s" % (c, key, d))
        all_paths[c] = len(res["all"])
        all_lens += [len(x) for x in res["all"]]
        po, eo = out["all_path_off"], out["all_elem_off"]
        if c + 1 < len(po):
            p0, p1 = int(po[c]), int(po[c + 1])
            if p1 - p0 != len(res["all"]) or (p1 > p0 and p1 >= len(eo)):
                bad.append("contig %d .all: %d paths, expected %d" % (c, p1 - p0, len(res["all"])))
            else:
                for i, rows in enumerate(res["all"]):
                    d = _rows_diff(rows, out["all"][int(eo[p0 + i]):int(eo[p0 + i + 1])])
                    if d:
                        bad.append("contig %d .all path %d: %s" % (c, i, d))
    cum = lambda x: np.concatenate([[0], np.cumsum(np.asarray(x, np.int64))])
    for key, want in (("main_off", cum(lens["main"])), ("alt_off", cum(lens["alt"])), ("all_path_off", cum(all_paths)), ("all_elem_off", cum(all_lens))):
        got = np.asarray(out[key], np.int64)
        if not (np.array_equal(got, want) or (len(got) == 0 and want.tolist() == [0])):     # (no .all path: no offsets at all)
            bad.append("%s differs from the rebuilt offsets" % key)
    for key in ("main", "alt"):
        if len(out[key]) != int(lens[key].sum()):
            bad.append("%s holds %d rows, expected %d" % (key, len(out[key]), int(lens[key].sum())))
    if len(out["all"]) != sum(all_lens):
        bad.append("all holds %d rows, expected %d" % (len(out["all"]), sum(all_lens)))
    return bad, per
