"""K9 cases: crafted contigs that put the window DP of the path upgrade (sel_ispr, alignasm_amd/csrc/aasm_kernels.h) and the
fixed-size structures around it on their form switches, with the facts measured and never taken from the builders' formulas.

sel_ispr picks one of five implementations of internal_shortest_path_recover by the window's positions W (= pb - pa in the
forward order) and the edges E of the rows of the positions [pa, pa + W): registers (W <= ISPR_REG_W, E <= 64, device only),
the cached LDS copy (W <= ISPR_CW, E <= ISPR_MAX_E), streamed on the narrow arrays (the copy does not fit), streamed on the
SelWide overlay (W <= ISPR_WIDE) and epoch-stamped global arrays beyond.  synth() batches reach these by chance and nothing
records which ran (a plain helper, imported by tests/test_k9_cases_cpu.py, tests/test_gpu_k9_edges.py and tools/k9_steps.py).

The pieces (records as in wide_cases._batch):
  detour(n, fills, pre, post, R)   `pre` colinear records on chromosome 0, then ONE part (a cover record spans it) that holds n
                short colinear records t_1 .. t_n on a chromosome of their own, one more record per entry k of `fills` over the
                span of t_k on yet another chromosome (`long_fills` more over the span of t_1 .. t_n: they link to nv
                alone), and nv, which continues chromosome 0 at a reference gap of R; then `post` colinear records.
                The last record p before the part links to every record of it, t_i to every t_j behind it.
                At R = 0 skipping the part (p -> nv, no anomaly) is the shortest walk, and the upgrade's window p .. x (x = the
                record after nv) fills t_1 .. t_n in again, because QRY_SCORE mode counts the query gap first: a result of n + 2
                edges that is NOT the walk's own two edges, chosen among 2^n (1 + ...) paths of many different distances.
                W = n + len(fills) + 3; the unsettled head sits at path edge `pre`, with `pre` edges in the output buffer.
                At a large R the walk goes through t_1 .. t_n itself, and its steps t_i -> t_i+1 -> t_i+2 are windows of W = 2
                with the edge t_i -> t_i+2 present: not settled, the DP has to run;
  chain(n)      n colinear records: a walk of n + 1 edges, every head settled (the run copy and the 64-edge path window);
  enum_cases.stages(2, (a, b))   a b walks of one sum and one anom: a tie run of a b - 1 walks, a b conversions.

  forks, clause3, bubble2   see their docstrings: tree segments of chosen lengths behind sidetracks, and the other-path clauses of
                the settled shortcut one at a time.

Facts come from a solve's intermediates (the emulation's on the CPU tier, which tests/test_k9_cases_cpu.py first compares
with the oracle's; the card's on the GPU tier) through k9_checker.check_conversion's window records, k9_checker.plan and
sp_best.  `known()`, `clauses()` and `walk_steps()` re-read sel_classify_edge's settled rule, the step loop's run copy and
sel_cw_fill's cache by hand: a FOURTH reading by the same author, not an independent fact.  On the CPU the counter test ties
it to the emulation slot by slot (calls, forms, cw_fills, edges copied in runs, settled d2 / d3); on the card nothing does.

What the scoring or the graph cannot produce, or what was not found (each argued, not measured):
  * a result of 30 edges on the LDS copy.  The walk's own edges are (u, v), (v, nv), so u and v lie in one part or in two
    neighbouring ones, and every vertex of the result lies between them: its 29 inner vertices end on 29 different records of
    those two parts, in query order.  Two records of one part that do not overlap always link (linkable: same part,
    qry_end < qry_str), as do any two of neighbouring parts, and a pair vertex (i, j) links to every later record as j does.
    29 such records carry 29 * 28 / 2 = 406 edges or more inside the window, above ISPR_MAX_E = 192: the form cannot see
    such a result.  The longest found is 16 edges (E = 137); the streamed form appends 37;
  * W = 63 at 191 ... 193 row edges with heads beyond the window: every record of the window's part links to every record of
    the part behind it, so one record more behind the window adds about 61 edges; built at W = 16 only;
  * the clauses u -> nv, u -> y -> nv and v -> y -> nv SMALLER than u -> v -> nv: where nv is a single-record vertex the window
    runs with the whitelist (the hop into nv only from v's record), so these paths are not candidates at all, whatever they
    weigh; they would need nv to be a pair vertex.  u -> y -> v LARGER: y lies in the query gap between u and v, so going
    through it always has the smaller query score.  Built: each of the three other clauses alone with the DP running and the
    path kept, u -> y -> v alone with the path changed;
  * v -> y -> nv alone: y and nv would have to share a part, which needs a record spanning both, and that record takes a
    position inside the window (dpos 4).  Not built;
(Alt candidates at plan index 29 and 293: `alt_low`, `alt_high`, the reference gap R tuned so that the walk without the
part comes after that many walks that skip some of t_1 .. t_9; K_BIG = 320 lets the plan see it.)"""
import numpy as np

import k9_checker as K
from capacity_cases import chain
from enum_cases import stages
from wide_cases import _batch, _chain

QT = 10 ** 8
K_SMALL, K_BIG = 4, 320                                               # K_BIG: above the longest tie run and above plan index 257
ISPR_REG_W, ISPR_CW, ISPR_WIDE, ISPR_MAX_E, SETTLE_SCAN_MAX, SEL_WIN, SEL_PLAN_KEEP = 16, 63, 127, 192, 48, 64, 64
PATH_LIMIT = 200000

# the host emulation's K9 counters (emul_k9_stats), by slot
K9_STAT_NAMES = ["conversions", "path_edges", "edges_copied_in_runs", "steps", "steps_pair_head", "steps_known", "ispr_calls", "ispr_w2_fast",
                 "ispr_lds_dp", "ispr_stream", "ispr_generic", "ispr_empty", "start_ne_u", "steps_to_dest", "cw_fills", "lds_dp_window_sum",
                 "settled_d2", "settled_d3"]

W_TARGETS = (1, 2, 15, 16, 17, 62, 63, 64, 65, 126, 127, 128, 129)
W_LONG = 200                                                          # > 192: more than three 64-position chunks of the generic form
LA_TARGETS = (63, 64, 65, 66, 127, 128, 129, 130)
HEAD_AT = (60, 61, 62, 63, 64, 65)                                    # the unsettled head's path edge = entries in the output buffer
TIE_WALKS = {63: (7, 9), 64: (8, 8), 65: (5, 13), 66: (6, 11), 128: (8, 16), 129: (3, 43)}   # walks of one sum -> stage widths
NCONV_TARGETS = (63, 64, 65, 66)
TIE_RUN_TARGETS = (63, 64, 65, 127, 128)
SEG_TARGETS = (15, 16, 17, 31, 32, 33)
DETOUR_N = 4                                                          # 2^4 ways through t_1 .. t_4: every window stays enumerable
LONG_RESULT_N = 14                                                    # a result of 16 edges on the LDS form, its 2^14 paths enumerated


def _part(recs, n, fills, long_fills, R, L, g, c0):
    """Appends one part behind recs[-1] (= p): cover, t_1 .. t_n, the fills, nv.  c0: the first chromosome the part may use."""
    p = recs[-1]
    q0 = p[1] + 52
    ts = []
    for i in range(n):
        qs, rs = q0 + i * (L + g), 5 * 10 ** 7 + 10 ** 5 * c0 + i * (L + g)
        ts.append((qs, qs + L - 1, rs, rs + L - 1, c0, 1, 60))
    fs = [(ts[k][0], ts[k][1], 9 * 10 ** 7 + 1000 * j, 9 * 10 ** 7 + 1000 * j + L - 1, c0 + 1 + j, 1, 60) for j, k in enumerate(fills)]
    fs += [(ts[0][0], ts[-1][1], 2 * 10 ** 8 + 10 ** 4 * j, 2 * 10 ** 8 + 10 ** 4 * j + ts[-1][1] - ts[0][0], c0 + 1 + len(fills) + j, 1, 60)
           for j in range(long_fills)]
    nq, nr = q0 + n * (L + g), p[3] + 1 + R
    nv = (nq, nq + 899, nr, nr + 899, 0, 1, 60)
    cover = (q0 - 1, nv[1], 3 * 10 ** 8 + 10 ** 6 * c0, 3 * 10 ** 8 + 10 ** 6 * c0 + nv[1] - q0 + 1, 0, 1, 60)
    recs += [cover] + ts + fs + [nv]
    return c0 + 1 + len(fills) + long_fills


def detour(n, fills=(), pre=2, post=2, R=0, L=100, g=10, long_fills=0, xtwin=False, more=()):
    """more: further parts, each dict(n, fills, long_fills, mid) behind `mid` colinear records; xtwin: the record behind the
    (first) part gets a twin on another chromosome, which every record of the part links to as well."""
    recs = _chain(1000, 10 ** 6, pre, 900, 50, 40)
    c0 = _part(recs, n, fills, long_fills, R, L, g, 1)
    for b in more:
        recs += _chain(recs[-1][1] + 51, recs[-1][3] + 41, b.get("mid", 1), 900, 50, 40)
        c0 = _part(recs, b["n"], b.get("fills", ()), b.get("long_fills", 0), R, L, g, c0)
    tail = _chain(recs[-1][1] + 51, recs[-1][3] + 41, post, 900, 50, 40)
    if xtwin:
        x = tail[0]
        tail.insert(1, (x[0], x[1], 4 * 10 ** 8, 4 * 10 ** 8 + x[1] - x[0], 999, 1, 60))
    return recs + tail


def forks(segs, pre=1):
    """`pre` colinear records, then per entry s of segs two equal records over one query span on chromosomes of their own
    and s colinear records behind them: 2^len(segs) walks of one sum.  The walks through a second record leave the tree
    there (a sidetrack) and follow it again for the s records behind."""
    recs = _chain(1000, 10 ** 6, pre, 900, 50, 40)
    for j, n in enumerate(segs):
        q = recs[-1][1] + 51
        recs += [(q, q + 899, 6 * 10 ** 7 + 10 ** 6 * j + 7 * i, 6 * 10 ** 7 + 10 ** 6 * j + 7 * i + 899, 10 + 2 * j + i, 1, 60) for i in range(2)]
        recs += _chain(q + 950, 10 ** 6 + 10 ** 5 * (j + 1), n, 900, 50, 40)
    return recs


def scan(j):
    """Two parallel records (the second shorter), one record c1, then c2 with j - 1 shorter twins (they start later: behind c2 in the order), then a chain: on the walk's
    edges (v1, c1), (c1, c2) the rows of v1, v2 and c1 hold 2 + j edges and no other path exists."""
    recs = bubble2(0)[:6]                                             # three colinear records, the two parallel ones, c1
    q = recs[-1][1] + 51
    recs += [(q + (10 if i else 0), q + 899, 7 * 10 ** 7 + 10 ** 4 * i, 7 * 10 ** 7 + 10 ** 4 * i + 899 - (10 if i else 0), 20 + i, 1, 60) for i in range(j)]
    return recs + _chain(q + 950, 9 * 10 ** 7, 2, 900, 50, 40)


def clause3(pre=2, post=2):
    """u and y under one cover, v alone in the next part, nv behind: u -> y -> v beside u -> v -> nv and no other path (dpos 3,
    y before v).  The shortest walk skips y (another chromosome), the upgrade fills it in."""
    recs = _chain(1000, 10 ** 6, pre, 900, 50, 40)
    p = recs[-1]
    q0 = p[1] + 52
    u = (q0, q0 + 899, p[3] + 41, p[3] + 41 + 899, 0, 1, 60)
    y = (u[1] + 11, u[1] + 110, 5 * 10 ** 7, 5 * 10 ** 7 + 99, 1, 1, 60)
    cover = (q0 - 1, y[1], 3 * 10 ** 8, 3 * 10 ** 8 + y[1] - q0 + 1, 0, 1, 60)
    v = (y[1] + 11, y[1] + 910, u[3] + 1, u[3] + 900, 0, 1, 60)
    return recs + [cover, u, y, v] + _chain(v[1] + 51, v[3] + 41, post, 900, 50, 40)


def bubble2(better):
    """Two parallel records between two chains, the second one shorter or longer: u -> y -> nv beside u -> v -> nv (dpos 3), y
    behind v in the order (better = 0) or before it (1)."""
    from capacity_cases import fan
    recs = fan(3, 2)
    a, b = recs[-2], recs[-1]
    w = recs[-1]                                                      # the worse one: shorter at its end (it sorts first: y before v) or at its start
    recs[-1] = ((w[0], w[1] - 100, w[2], w[3] - 100) if better else (w[0] + 100, w[1], w[2] + 100, w[3])) + w[4:]
    return recs + _chain(a[1] + 51, 8 * 10 ** 7, 3, 900, 50, 40)


def contigs():
    """[(name, records)] of the crafted batch."""
    C = [("w_%d" % w, detour(DETOUR_N, (0,) * (w - DETOUR_N - 3))) for w in W_TARGETS if w >= DETOUR_N + 3]
    C += [("w_long", detour(DETOUR_N, (0,) * (W_LONG - DETOUR_N - 3))),
          ("w_wide_late", detour(DETOUR_N, (DETOUR_N - 1,) * 90)),    # the fills behind t_1 .. t_3 in the order: sources of an earlier chunk
          ("w_generic_late", detour(DETOUR_N, (DETOUR_N - 1,) * 150)),
          ("w2_unsettled", detour(3, R=10 ** 5)),
          ("result_long", detour(LONG_RESULT_N)),
          ("result_35", detour(35))]                                  # a streamed result of 37 edges; 2^35 paths: the checker skips it
    C += [("lds_%d" % w, detour(1, (0,) * (w - 4))) for w in (62, 63, 64)]   # few row edges: the LDS copy up to W = 63
    C += [("e_%d" % (185 + a), detour(2, (0,) * a, long_fills=58 - a)) for a in (6, 7, 8)]   # W = 63 with 191, 192 | 193 row edges
    C += [("e16_63", detour(3, (0,), long_fills=9, xtwin=True)), ("e16_64", detour(3, (0,) * 9, long_fills=1)),   # W = 16: 63, 64 | 65
          ("e16_65", detour(3, (0, 0), long_fills=8, xtwin=True)),
          ("copy_edge", detour(4, (0,), more=[dict(n=3, mid=50)])),   # the second part's windows end on the copy's last position and one past it
          ("copy_cut_e", detour(16, more=[dict(n=3, mid=30)]))]       # the copy ends after 192 edges, the second part lies beyond it
    C += [("d3_u_y_nv_after", bubble2(0)), ("d3_u_y_nv_before", bubble2(1)), ("d3_u_nv", detour(1, R=10 ** 5)), ("d3_u_y_v", clause3()),
          ("segs_15", forks((15, 16, 16))), ("segs_31", forks((31, 32, 32)))]    # the last segment runs one edge further, to dest
    C += [("scan_48", scan(46)), ("scan_49", scan(47))]
    C += [("alt_low", detour(9, R=3500)), ("alt_high", detour(9, R=3900))]
    C += [("la_%d" % la, chain(la - 1)) for la in LA_TARGETS]
    C += [("head_%d" % h, detour(DETOUR_N, (0, 1), pre=h)) for h in HEAD_AT]
    C += [("ties_%d" % w, stages(2, ab)) for w, ab in TIE_WALKS.items()]
    return C


SKIPPED = {"result_35"}                               # contigs with a window of more than PATH_LIMIT a -> b paths


def batch(cs=None):
    cs = cs or contigs()
    return [n for n, _ in cs], _batch([(QT, recs) for _, recs in cs])


def mixed(T):
    """(names, HostBatch): the crafted contigs reversed, synth() contigs between them (enum_cases.mixed)."""
    from enum_cases import join
    names, hb = batch()
    syn = [(T.synth(3, 60, 5, dup_every=3), c) for c in range(3)] + [(T.synth(1, 80, 31, dense=True), 0)]
    parts, out = [], []
    for i, c in enumerate(reversed(range(len(names)))):
        parts.append((hb, c)); out.append(names[c])
        if i % 8 == 1 and syn:
            parts.append(syn.pop(0)); out.append("synth_%d" % len(syn))
    return out, join(parts)


# ---- facts -----------------------------------------------------------------------------------------------------------------------
def scan_edges(g, u, nv):
    """(dpos, edges of the rows sel_classify_edge scans) for a step from u to nv; dpos other than 2 / 3: no scan."""
    pu, dpos = int(g.pos[u]), int(g.pos[nv]) - int(g.pos[u])
    if dpos not in (2, 3):
        return dpos, 0
    return dpos, sum(int(g.rowptr[int(g.order[pu + t]) + 1] - g.rowptr[int(g.order[pu + t])]) for t in range(dpos))


def known(g, u, v, nv):
    """sel_classify_edge's `settled` for the edges (u, v), (v, nv), re-read: -> 0, or the dpos (2 / 3) it is settled at."""
    pu, pv, pnv = int(g.pos[u]), int(g.pos[v]), int(g.pos[nv])
    dpos = pnv - pu
    if dpos not in (2, 3):
        return 0
    rows = [int(g.order[pu + t]) for t in range(dpos)]
    heads = [[int(g.pos[h]) for h in g.col[int(g.rowptr[r]):int(g.rowptr[r + 1])]] for r in rows]
    if sum(len(h) for h in heads) > SETTLE_SCAN_MAX:
        return 0
    if dpos == 2:
        return 0 if pnv in heads[0] else 2
    py = pu + 1 if pv == pu + 2 else pu + 2
    hy, hv = heads[py - pu], heads[pv - pu]
    other = pnv in heads[0] or (py in heads[0] and pnv in hy) or ((py in heads[0] and pv in hy) if py < pv else (py in hv and pnv in hy))
    return 0 if other else 3


def form_of(w):
    """The form sel_ispr serves a window with, from W and the row edges (whole rows of [pa, pa + W)).  A window that lies inside
    the cached copy has E <= ISPR_MAX_E, and one that the copy cannot hold has more: the copy's state does not change the form."""
    if w["W"] > ISPR_WIDE:
        return "generic"
    if w["W"] > ISPR_CW:
        return "stream_wide"
    if w["E"] > ISPR_MAX_E:
        return "stream_narrow"
    return "reg" if w["W"] <= ISPR_REG_W and w["E"] <= SEL_WIN else "lds"


def walk_steps(g, pa, sett, windows):
    """The step loop of sel_upgrade over the walk pa, re-read (the fourth reading named in the module's docstring): which
    edges the run copy takes in one piece (emulation: up to 64 from the edge at hand; the card: up to the end of its 64-edge
    path window), and what the cached copy of sel_cw_fill holds at every window DP.  Annotates every called window with
    `hit` (served from a copy an earlier call filled), `o` (its offset in the copy), `ends` (pb - the copy's last position:
    0 = exactly on it), `cut_e` (the copy was cut short by ISPR_MAX_E, not by ISPR_CW or the contig's end), `at_end` (fewer
    than ISPR_CW positions were left).  -> dict(runs = [lengths], cw_fills)."""
    la, dest, src = len(pa), g.dest, g.src
    single = lambda v: v != dest and int(g.v_i[v]) == int(g.v_j[v])
    by_it = {w["it"]: w for w in windows}
    ptr = lambda p: int(g.rowptr[int(g.order[p])])                   # (rows of the topologically ordered copy: lengths, summed below)
    deg = [int(g.rowptr[int(g.order[p]) + 1] - g.rowptr[int(g.order[p])]) for p in range(g.V)]
    runs, fills, cw, last = [], 0, None, -1

    def dp(w):
        nonlocal cw, fills
        a0, W = w["pa"], w["W"]
        w["hit"], w["o"], w["ends"], w["cut_e"], w["at_end"], w["past"], w["prev_cut_e"] = False, 0, None, False, False, None, False
        if W > ISPR_WIDE:
            return
        if W > ISPR_CW:
            cw = None
            return
        if cw and a0 >= cw[0] and a0 + W <= cw[0] + cw[1]:
            w["hit"], w["o"] = True, a0 - cw[0]
        else:
            if cw and cw[0] <= a0 < cw[0] + cw[1]:                    # starts inside the copy, ends behind it: a refill
                w["past"] = a0 + W - (cw[0] + cw[1])
            w["prev_cut_e"] = bool(cw and cw[2])
            fills += 1
            n = min(g.V - a0, ISPR_CW)
            m, tot = 0, 0
            for t in range(1, n + 1):
                tot += deg[a0 + t - 1]
                if tot > ISPR_MAX_E:
                    break
                m = t
            if m < W:
                cw = None
                return
            cw = (a0, m, m < n, g.V - a0 < ISPR_CW)
        w["ends"], w["cut_e"], w["at_end"] = a0 + W - (cw[0] + cw[1]), cw[2], cw[3]

    it = 0
    while it < la:
        u, v = pa[it]
        if it > 0 and v != dest and (not single(v) or (sett[it] and last == u)):
            run = 0
            while it + run < la and run < SEL_WIN and not ((single(pa[it + run][1]) and not sett[it + run]) or pa[it + run][1] == dest):
                run += 1
            if run >= 2:
                runs.append(run)
                last = pa[it + run - 1][1]
                it += run
                continue
        if u != src and v != dest and not single(v):
            last = v
            it += 1
            continue
        if v == dest and u != src:
            dp(by_it[it])
            it += 1
            continue
        nv = pa[it + 1][1]
        nv_single = nv == dest or single(nv)
        start = src if u == src else last
        if sett[it] and start == u:
            last = v if nv_single else nv
        else:
            w = by_it.get(it)                                         # (none: a == b, the caller's own edges)
            res = []
            if w:
                assert w["a"] == start, (it, w["a"], start)
                dp(w)
                res = w["res"][:-1] if nv_single else w["res"]
            last = res[-1][1] if res else (v if nv_single else nv)
        it += 1 if nv_single else 2
    return dict(runs=runs, cw_fills=fills)


def clauses(g, u, v, nv):
    """Which other-path clauses of sel_classify_edge hold for (u, v), (v, nv) at dpos 3 -> (set of names, y before v)."""
    pu, pv, pnv = int(g.pos[u]), int(g.pos[v]), int(g.pos[nv])
    if pnv - pu != 3:
        return None
    y = int(g.order[pu + 1 if pv == pu + 2 else pu + 2])
    e = g.has_edge
    out = set()
    if e(u, nv): out.add("u_nv")
    if e(u, y) and e(y, nv): out.add("u_y_nv")
    if e(u, y) and e(y, v): out.add("u_y_v")
    if e(v, y) and e(y, nv): out.add("v_y_nv")
    return out, int(g.pos[y]) < pv


def segments(pa, best, dest):
    """Tree segments of the walk: -> (edges of the tree run behind each sidetrack, up to the next sidetrack or dest; sidetracks;
    tree runs in front of a sidetrack)."""
    tree = [int(best[u]) == v for u, v in pa]
    st = [t for t, x in enumerate(tree) if not x]
    after = [(st[k + 1] if k + 1 < len(st) else len(pa)) - t - 1 for k, t in enumerate(st)]
    before = [t - (st[k - 1] + 1 if k else 0) for k, t in enumerate(st)]
    return after, len(st), before


def contig_facts(a, c):
    """One contig of a solve (a = k9_checker.collect(..., full=True)): per conversion la, lb and the window records (with `form`
    and `called`: False where the kernel's settled shortcut answers without a DP), settled counts over every path edge, the
    edges the run copy takes; the plan's tie run and conversion count; the checker's findings."""
    g = K.graph_of(a, c)
    found, Kp = int(a["kfound"][c]), a["K"]
    pl, bad = K.plan(a["kd"][c * Kp:c * Kp + found], found, int(a["anom_dest"][c]))
    f = dict(V=g.V, E=int(g.rowptr[-1]), found=found, nconv=len(pl), tie_run=sum(1 for _, kind in pl if kind == 1),
             alt_idx=[k for k, kind in pl if kind >= 2], convs=[], bad=list(bad))
    for j, (pa, pb) in enumerate(K.conversions_of(a, c)):
        st = {"windows": [], "path_limit": PATH_LIMIT}
        f["bad"] += ["conversion %d: %s" % (j, x) for x in K.check_conversion(g, pa, pb, brute_max=10 ** 9, stats=st)]
        d2 = d3 = 0
        sett, scans = [], []
        for t in range(len(pa)):
            kn = known(g, pa[t][0], pa[t][1], pa[t + 1][1]) if t + 1 < len(pa) else 0
            sett.append(kn)
            if t + 1 < len(pa):
                scans.append(scan_edges(g, pa[t][0], pa[t + 1][1]) + (kn, frozenset((clauses(g, pa[t][0], pa[t][1], pa[t + 1][1]) or [()])[0])))
            d2 += kn == 2; d3 += kn == 3
        for w in st["windows"]:
            w["form"] = form_of(w)
            t = w["it"]
            w["called"] = not (pa[t][1] != g.dest and sett[t] and w["a"] == pa[t][0])
            w["late"] = any(int(g.pos[v]) - w["pa"] >= 64 for _, v in w["res"][:-1])     # the result passes a vertex of a later 64-position chunk
            w["clauses"] = clauses(g, w["own"][0][0], w["own"][0][1], w["own"][1][1]) if len(w["own"]) == 2 else None
            w["u_nv"] = len(w["own"]) == 2 and g.has_edge(w["own"][0][0], w["own"][1][1])
            w["beyond"] = any(int(g.pos[h]) > w["pa"] + w["W"] for p_ in range(w["pa"], w["pa"] + w["W"])
                              for h in g.col[int(g.rowptr[int(g.order[p_])]):int(g.rowptr[int(g.order[p_]) + 1])])   # a head behind the window's end
        segs = segments(pa, a["sp_best"][int(a["voff"][c]):], g.dest) if "sp_best" in a else ([], 0, [])
        sim = walk_steps(g, pa, sett, [w for w in st["windows"] if w["called"]])
        f["convs"].append(dict(la=len(pa), lb=len(pb), windows=st["windows"], settled_d2=d2, settled_d3=d3, runs=sim["runs"],
                               cw_fills=sim["cw_fills"], segs=segs[0], n_st=segs[1], st_before=segs[2], scans=scans))
    return f


def facts(T, hb, Kp, fetch=None):
    """[contig_facts] of a batch at K = Kp, from an emulated solve (or from `fetch` of a solve already made)."""
    if fetch is None:
        T.emul_solve(hb, Kp)
        fetch = T.emul_debug
    a = K.collect(fetch, hb.arrays["ctg_rec_off"], full=True, K=Kp)
    a["sp_best"] = fetch("sp_best", np.int32)
    return [contig_facts(a, c) for c in range(hb.n_contigs)]


FORMS = ("reg", "lds", "stream_narrow", "stream_wide", "generic")


def coverage(names, F):
    """names, F = {K: facts(...)} -> (what each contig reached, [targets missed])."""
    got, miss = {}, []
    wins = []                                                         # (contig, window) of every DP the kernel computes
    for Kp, fl in F.items():
        for n, f in zip(names, fl):
            ws = [w for cv in f["convs"] for w in cv["windows"] if w["called"]]
            wins += [(n, w) for w in ws]
            got.setdefault(n, {})[Kp] = dict(V=f["V"], E=f["E"], found=f["found"], nconv=f["nconv"], tie_run=f["tie_run"],
                                             la=[cv["la"] for cv in f["convs"]][:3],
                                             windows=sorted({(w["W"], w["E"], w["form"], w["differs"], len(w["res"])) for w in ws}))

    def need(what, ok):
        if not ok:
            miss.append(what)

    # A: window positions
    for W in W_TARGETS:
        need("A: a computed window of W = %d" % W, any(w["W"] == W for _, w in wins))
    need("A: W > 192", any(w["W"] > 192 for _, w in wins))
    for lo, hi in ((ISPR_CW + 1, ISPR_WIDE), (ISPR_WIDE + 1, 10 ** 9)):    # the result passes a vertex more than 64 positions behind pa
        need("A: W in %d .. : a result through a later chunk" % lo,
             any(lo <= w["W"] <= hi and w["differs"] and len(w["res"]) > 2 and w["late"] for _, w in wins))
    # B: row edges at a fixed form by W
    need("B: W = 16 with 63 and with 65 row edges whose rows hold heads beyond the window",
         all(any(w["W"] == ISPR_REG_W and w["E"] == E and w["differs"] and w["beyond"] for _, w in wins) for E in (63, 65)))
    # C: the cached copy
    need("C: a window served at an offset o > 0 from a copy an earlier call filled", any(w.get("hit") and w["o"] > 0 for _, w in wins))
    need("C: a window that ends exactly on the copy's last position", any(w.get("hit") and w["ends"] == 0 for _, w in wins))
    need("C: a window that ends one past it (a refill)", any(w.get("past") == 1 for _, w in wins))
    need("C: a copy cut short by ISPR_MAX_E, then a window beyond it", any(w.get("prev_cut_e") and w.get("past") is None for _, w in wins))
    need("C: a copy at the contig's end", any(w.get("at_end") for _, w in wins))
    for W, es in ((ISPR_REG_W, (63, 64, 65)), (ISPR_CW, (191, 192, 193))):
        for E in es:
            need("B: W = %d with %d row edges, a result that differs" % (W, E), any(w["W"] == W and w["E"] == E and w["differs"] for _, w in wins))
    need("A: the LDS copy at W = 63", any(w["W"] == ISPR_CW and w["form"] == "lds" and w["differs"] for _, w in wins))
    # the five forms: a result that is not the walk's own edges, chosen among candidates of different distances
    for fm in FORMS:
        need("form %s: a result that differs" % fm, any(w["form"] == fm and w["differs"] for _, w in wins))
        need("form %s: ... among two or more distinct distances, enumerated" % fm,
             any(w["form"] == fm and w["differs"] and (w["ndist"] or 0) >= 2 for _, w in wins))
    need("D: an unsettled window of dpos 2 (u -> nv present)", any(w["W"] == 2 and w["u_nv"] and not w["differs"] for _, w in wins))
    for cl, before in (("u_nv", True), ("u_y_nv", True), ("u_y_nv", False), ("u_y_v", True)):
        need("D: dpos 3, the clause %s alone, y %s v: the DP runs" % (cl, "before" if before else "behind"),
             any(w["clauses"] == ({cl}, before) for _, w in wins))
    need("D: u -> y -> v smaller than u -> v: the upgrade changes the path", any(w["clauses"] == ({"u_y_v"}, True) and w["differs"] for _, w in wins))
    cvs = [cv for fl in F.values() for f in fl for cv in f["convs"]]
    need("D: three rows of %d edges without another path: settled" % SETTLE_SCAN_MAX, any(sc == (3, SETTLE_SCAN_MAX, 3, frozenset()) for cv in cvs for sc in cv["scans"]))
    need("D: the same with %d edges: left to the DP" % (SETTLE_SCAN_MAX + 1), any(sc == (3, SETTLE_SCAN_MAX + 1, 0, frozenset()) for cv in cvs for sc in cv["scans"]))
    # F: the recovery
    for x in SEG_TARGETS:
        need("F: a tree segment of %d edges behind a sidetrack" % x, any(x in cv["segs"] for cv in cvs))
    need("F: a walk with three sidetracks or more", any(cv["n_st"] >= 3 for cv in cvs))
    need("F: a sidetrack whose tail is reached in the middle of a 16-hop record", any(b % 16 not in (0,) and b > 0 for cv in cvs for b in cv["st_before"]))
    # E: path lengths, the head's edge index and the output buffer's fill at a DP whose result differs, a long result
    las = {cv["la"] for fl in F.values() for f in fl for cv in f["convs"]}
    for la in LA_TARGETS:
        need("E: la = %d" % la, la in las)
    for h in HEAD_AT:
        need("E: a differing result at path edge %d with %d entries in the buffer" % (h, h),
             any(w["it"] == h and w["out_len"] == h and w["differs"] and len(w["res"]) >= 3 for _, w in wins))
    # (t_i links to every t_j behind it, so a part of n records has n (n - 1) / 2 + 3 n row edges: ISPR_MAX_E ends the LDS form at
    # n = 16, and 30 result edges on it are out of this builder's reach - argued, not measured; the streamed form appends 37)
    need("E: an LDS-form result of 16 edges", any(w["form"] == "lds" and len(w["res"]) >= 16 for _, w in wins))
    need("E: a streamed result of 30 edges or more", any(w["form"] == "stream_narrow" and len(w["res"]) >= 30 for _, w in wins))
    # G: plan
    allf = [f for fl in F.values() for f in fl]
    for x in NCONV_TARGETS:
        need("G: nconv = %d" % x, any(f["nconv"] == x for f in allf))
    for x in TIE_RUN_TARGETS:
        need("G: a tie run of %d" % x, any(f["tie_run"] == x for f in allf))
    need("G: an alt candidate (fewer anomalies than the main walk) converted from an index below 64", any(0 < i < 64 for f in allf for i in f["alt_idx"]))
    need("G: an alt candidate at index 257 or above (the second round of the plan's four-load loop)", any(i >= 257 for f in allf for i in f["alt_idx"]))
    need("G: found < 64 with a tie run", any(f["found"] < 64 and f["tie_run"] >= 62 for f in allf))
    # the enumeration: every window but the named contigs' is enumerated
    skipped = {n for fl in F.values() for n, f in zip(names, fl) for cv in f["convs"] for w in cv["windows"] if w["skipped"]}
    need("the checker skips exactly the named windows (skipped: %r)" % sorted(skipped), skipped == SKIPPED)
    return got, miss

