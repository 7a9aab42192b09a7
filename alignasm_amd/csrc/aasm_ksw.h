// aasm_ksw.h -- batched k shortest walks on caller-supplied graphs (row ★K): the solver's k_shortest_walks()
// (k_shortest_walks.hpp:177-249) with is_dag = true, or with is_dag = false under AASM_KSW_CYCLES (negative_edge = true with
// AASM_KSW_NEGATIVE beside it), and kth_shortest_walk_recover() (:252-290), one workgroup per graph.
//
// Kernel bodies (KCtx style, so tests/host_emul/graphs_emul.cpp compiles them for one lane on the host):
//   kb_ksw_tree   reversed CSR in the reference's list order (:180-183), Kahn order of the reversed graph (:132-156) fused
//                 with the DAG relaxation to the sink (:160-175; strict `>` in CALC_SUM order), the best EDGE beside best,
//                 cycle detection, the children of every tree vertex in ascending u (:191-194), the BFS from the sink, the
//                 exact sidetrack insert count and the number of walks (saturated at k): the bounds the host sizes by
//   kb_ksw_tree_cyc   the same stage for graphs that may hold cycles: the tree is the one dijkstra() from the sink over the
//                 reversed graph leaves (:69-87, kb_sssp_dijkstra's formulation), with a bound on its pushes and a guard that
//                 best[] is a tree into the sink; the number of walks is k as soon as a cycle lies between source and sink
//   kb_ksw_tree_bf    the same with the tree of bellman_ford() (:91-129, bf_spfa's formulation): negative weights, no bound on pushes
//   kb_ksw_heap   the persistent leftist heaps (:196-215, leftist_heap.hpp:29-40) in the reference's allocation order
//   kb_ksw_enum   k pops of the min-queue of (distance, node, insertion index) (:230-249): ties by arena index, the
//                 monotonic allocator's order (hazard B3)
//   kb_ksw_count / kb_ksw_fill   walk recovery as caller edge ids: lengths, per-graph scan, edges
// The sequential stages run on lane 0 of the graph's wave (the reference's order is sequential by definition); the
// recovery runs one walk per lane.  Every loop is bounded by the graph's size or by a capacity checked before a write.
#pragma once
#include "aasm_sssp.h"

namespace aasm {

#define AASM_KSW_MAX_V ((int64_t)1 << 20)     // vertices per graph: a walk sum over < 2^20 edges of |w| < 2^39 stays in int64
#define AASM_KSW_MAX_K ((int64_t)1 << 24)
#define AASM_KSW_MAX_WALK_EDGES ((int64_t)1 << 28)   // AASM_KSW_CYCLES: edges of one graph's walks together
#define AASM_KSW_SPINE 64                     // right-spine stack of one insert (a version of <= 2^31 keys has a spine <= 33)
#define AASM_KSW_DJ_PUSHES 64                 // dijkstra of kb_ksw_tree_cyc: at most 64 * (E + 2) pushes per graph
#define AASM_KSW_SAFE_SCORE ((int64_t)1 << 62)   // with cycles a walk has any number of edges: a queued distance stays below
#define AASM_KSW_SAFE_COUNT ((int32_t)1 << 30)   // these in |qry|, |ref| and in anom, qnz, qtot

// heap node (leftist_heap.hpp:18-27), 48 bytes: the value (u, v) is the edge e (u = its tail, v = col[e]) -
// the edge id is what tells parallel edges apart
struct __attribute__((aligned(16))) KswNode {
    Dist key;
    int32_t rank, left, right, e;   // arena indices local to the graph (-1 = nullptr); e local to the graph
};
// queue entry: std::tuple<Distance, heap_t *, int64_t> (:231), the pointer as the arena index
struct __attribute__((aligned(16))) KswQE {
    Dist d;
    int32_t hp, cur;
    int64_t pad;
};

struct KswArgs {
    int64_t n_graphs, k;
    const int64_t *voff, *rowptr, *w5;                  // caller layout (global vertex / edge ids)
    const int32_t *col, *src, *sink;
    // per vertex (global id)
    int32_t *roff, *deg, *order, *best, *bedge, *koff, *kids, *bfs, *depth, *hroot;
    Dist *d;
    int64_t *cnt;
    // per edge (global id)
    int32_t *rev, *etail;
    // per graph
    int32_t *status;
    int64_t *nbfs, *ins, *walks, *hcount, *nfound, *wtot;
    // sized per chunk of graphs by the host: graph g owns [aoff[g], aoff[g] + acap[g]) of the arena,
    // [qoff[g], + qcap[g]) of the queue, [rofs[g], + walks[g]) of the results, [wbase[g], + wtot[g]) of the walk edges
    const int64_t *aoff, *acap, *qoff, *qcap, *rofs, *wbase;
    KswNode *arena;
    KswQE *q;
    int32_t *qnode, *qprev, *rlast;
    Dist *rdist;
    int64_t *woff, *wedges;
    // AASM_KSW_CYCLES: graph g's dijkstra heap is [hoff[g], hoff[g + 1]) of dheap (empty: the graph is left as it is); with
    // AASM_KSW_NEGATIVE its bellman_ford queue ring
    int32_t cycles;
    const int64_t *hoff;
    DjEnt *dheap;
};

AASM_DEV bool ksw_is_ident(const Dist &c) { return dist_eq(c, dist_zero()); }

// tree[best[u]] in ascending u (its end is deg[], which must be 0 everywhere on entry), the BFS order from the sink with depth[]
// (-1 on entry), and the inserts the heap stage will make: nbfs[g], ins[g].  False when a vertex is reached twice (best[] is no
// tree; never in a DAG).
AASM_DEV bool ksw_tree_bfs(const KswArgs &a, int64_t g) {
    const int64_t vb = a.voff[g], V = a.voff[g + 1] - vb, eb = a.rowptr[vb];
    const int32_t t = a.sink[g];
    int32_t *deg = a.deg + vb, *koff = a.koff + vb, *kids = a.kids + vb, *bfs = a.bfs + vb, *depth = a.depth + vb;
    const int32_t *best = a.best + vb, *col = a.col + eb;
    const Dist *d = a.d + vb;
    const int64_t *rp = a.rowptr + vb;
    for (int64_t v = 0; v < V; v++) if (best[v] >= 0) deg[best[v]]++;
    int32_t run = 0;
    for (int64_t v = 0; v < V; v++) { const int32_t c = deg[v]; koff[v] = run; deg[v] = run; run += c; }
    for (int64_t v = 0; v < V; v++) if (best[v] >= 0) kids[deg[best[v]]++] = (int32_t)v;
    // BFS from the sink over the tree, counting the inserts the heap stage will make
    int64_t bh = 0, bt = 0, ins = 0;
    bfs[bt++] = t; depth[t] = 0;
    while (bh < bt) {
        const int32_t u = bfs[bh++];
        bool seen_p = false;
        for (int64_t e = rp[u] - eb; e < rp[u + 1] - eb; e++) {
            const int32_t v = col[e];
            if (dist_is_max(d[v])) continue;
            if (!seen_p && v == best[u] && ksw_is_ident(dist_sub(dist_add(edge_w5(a.w5, eb + e), d[v]), d[u]))) { seen_p = true; continue; }
            ins++;
        }
        for (int32_t j = koff[u]; j < deg[u]; j++) {
            const int32_t p = kids[j];
            if (depth[p] >= 0) return false;
            depth[p] = depth[u] + 1; bfs[bt++] = p;
        }
    }
    a.nbfs[g] = bt; a.ins[g] = ins;
    return true;
}

// ---- stage 1-2: reversed CSR, Kahn order + DAG relaxation, tree children, BFS, bounds ------------------------------------
AASM_DEV void kb_ksw_tree(const KCtx &k, const KswArgs &a) {
    const int64_t g = k.bid;
    if (g >= a.n_graphs || k.tid != 0) return;
    const int64_t vb = a.voff[g], V = a.voff[g + 1] - vb, eb = a.rowptr[vb], E = a.rowptr[vb + V] - eb;
    const int32_t s = a.src[g], t = a.sink[g];
    int32_t *roff = a.roff + vb, *deg = a.deg + vb, *order = a.order + vb, *best = a.best + vb, *bedge = a.bedge + vb;
    int32_t *koff = a.koff + vb, *depth = a.depth + vb;
    int32_t *rev = a.rev + eb, *etail = a.etail + eb;
    Dist *d = a.d + vb;
    int64_t *cnt = a.cnt + vb;
    const int64_t *rp = a.rowptr + vb;
    const int32_t *col = a.col + eb;
    for (int64_t v = 0; v < V; v++) {
        roff[v] = 0; d[v] = dist_max(); best[v] = -1; bedge[v] = -1; cnt[v] = 0; depth[v] = -1;
        deg[v] = (int32_t)(rp[v + 1] - rp[v]);                      // in-degree in the reversed graph = out-degree
        for (int64_t e = rp[v] - eb; e < rp[v + 1] - eb; e++) etail[e] = (int32_t)v;
    }
    // g_rev[v] lists the tails of v's in-edges in ascending (tail, list position) order = ascending edge id
    for (int64_t e = 0; e < E; e++) roff[col[e]]++;
    int32_t run = 0;
    for (int64_t v = 0; v < V; v++) { const int32_t c = roff[v]; roff[v] = run; run += c; }
    for (int64_t v = 0; v < V; v++) koff[v] = roff[v];               // fill cursor
    for (int64_t e = 0; e < E; e++) rev[koff[col[e]]++] = (int32_t)e;
    // Kahn FIFO of the reversed graph, seeded in index order; each vertex is relaxed when it leaves the queue, which is the
    // reference's separate pass over the finished order (a vertex's distance is final before it is popped)
    int64_t head = 0, tail = 0;
    for (int64_t v = 0; v < V; v++) if (deg[v] == 0) order[tail++] = (int32_t)v;
    d[t] = dist_zero();
    cnt[t] = 1;
    while (head < tail) {
        const int32_t v = order[head++];
        const int64_t r1 = v + 1 < V ? roff[v + 1] : E;
        const bool live = !dist_is_max(d[v]);
        for (int64_t r = roff[v]; r < r1; r++) {
            const int32_t e = rev[r], to = etail[e];
            if (live) {
                const Dist cand = dist_add(d[v], edge_w5(a.w5, eb + e));
                if (dist_lt<CALC_SUM_MODE>(cand, d[to])) { d[to] = cand; best[to] = v; bedge[to] = e; }   // d[to] > d[v] + w
                const int64_t c = cnt[to] + cnt[v];
                cnt[to] = c < a.k ? c : a.k;                          // walks to the sink, saturated at k
            }
            if (--deg[to] == 0) order[tail++] = to;
        }
    }
    if (tail < V) {                                                  // a cycle: topology_sort asserts (:144-147)
        a.status[g] = AASM_E_INVAL;
        for (int64_t v = 0; v < V; v++) { d[v] = dist_max(); best[v] = -1; bedge[v] = -1; }
        d[t] = dist_zero();
        a.nbfs[g] = 0; a.ins[g] = 0; a.walks[g] = 0;
        return;
    }
    a.status[g] = 0;
    a.walks[g] = dist_is_max(d[s]) ? 0 : cnt[s];
    ksw_tree_bfs(a, g);                                              // (the Kahn countdown deg[] is 0 everywhere now)
}

// What the two tree kernels for graphs with cycles share, on one lane.  ksw_cyc_prepare: every per-vertex array at its start value
// and the reversed lists, g_rev[v] as in kb_ksw_tree (ascending edge id within a head).  ksw_cyc_tail, after the tree is found: the
// tree guard, the BFS with the insert count, and the bound on the number of walks.
AASM_DEV void ksw_cyc_prepare(const KswArgs &a, int64_t g) {
    const int64_t vb = a.voff[g], V = a.voff[g + 1] - vb, eb = a.rowptr[vb], E = a.rowptr[vb + V] - eb;
    int32_t *roff = a.roff + vb, *deg = a.deg + vb, *best = a.best + vb, *bedge = a.bedge + vb, *koff = a.koff + vb, *depth = a.depth + vb;
    int32_t *rev = a.rev + eb, *etail = a.etail + eb;
    Dist *d = a.d + vb;
    int64_t *cnt = a.cnt + vb;
    const int64_t *rp = a.rowptr + vb;
    const int32_t *col = a.col + eb;
    for (int64_t v = 0; v < V; v++) {
        roff[v] = 0; d[v] = dist_max(); best[v] = -1; bedge[v] = -1; cnt[v] = 0; depth[v] = -1; deg[v] = 0;
        for (int64_t e = rp[v] - eb; e < rp[v + 1] - eb; e++) etail[e] = (int32_t)v;
    }
    for (int64_t e = 0; e < E; e++) roff[col[e]]++;
    int32_t run = 0;
    for (int64_t v = 0; v < V; v++) { const int32_t c = roff[v]; roff[v] = run; run += c; }
    for (int64_t v = 0; v < V; v++) koff[v] = roff[v];
    for (int64_t e = 0; e < E; e++) rev[koff[col[e]]++] = (int32_t)e;
    d[a.sink[g]] = dist_zero();                                      // IDENTITY_DISTANCE (:73)
}
AASM_DEV void ksw_cyc_tail(const KswArgs &a, int64_t g) {
    const int64_t vb = a.voff[g], V = a.voff[g + 1] - vb, eb = a.rowptr[vb], E = a.rowptr[vb + V] - eb;
    const int32_t s = a.src[g], t = a.sink[g];
    int32_t *roff = a.roff + vb, *deg = a.deg + vb, *order = a.order + vb;
    int32_t *koff = a.koff + vb, *kids = a.kids + vb;
    int32_t *rev = a.rev + eb, *etail = a.etail + eb;
    Dist *d = a.d + vb;
    int64_t *cnt = a.cnt + vb;
    const int64_t *rp = a.rowptr + vb;
    const int32_t *col = a.col + eb;
    // best[] must be a tree into the sink: the BFS from the sink over tree[] visits every vertex with a distance, once (where it
    // is none - the sink's own distance improved round a cycle - the reference's BFS does not end)
    int64_t fin = 0;
    for (int64_t v = 0; v < V; v++) fin += !dist_is_max(d[v]);
    if (!ksw_tree_bfs(a, g) || a.nbfs[g] != fin) {
        a.status[g] = AASM_E_INVAL;
        a.nbfs[g] = 0; a.ins[g] = 0;
        return;
    }
    a.status[g] = 0;
    if (dist_is_max(d[s])) return;                                   // no walk (:188-189)
    // An upper bound on distances.size(): the walks source -> sink stay on S, the vertices the source reaches among those with a
    // distance.  Kahn on the reversed graph of S; a vertex left over lies on or behind a cycle, then there is no bound but k;
    // otherwise the walks are the paths of a DAG, counted as in kb_ksw_tree.  (koff, kids, order, deg are free after the BFS.)
    int32_t *mark = koff, *queue = kids;
    for (int64_t v = 0; v < V; v++) { mark[v] = 0; deg[v] = 0; cnt[v] = 0; }
    int64_t head = 0, nS = 0;
    order[nS++] = s; mark[s] = 1;
    while (head < nS) {
        const int32_t u = order[head++];
        for (int64_t e = rp[u] - eb; e < rp[u + 1] - eb; e++) {
            const int32_t v = col[e];
            if (!mark[v] && !dist_is_max(d[v])) { mark[v] = 1; order[nS++] = v; }
        }
    }
    for (int64_t i = 0; i < nS; i++) {
        const int32_t u = order[i];
        for (int64_t e = rp[u] - eb; e < rp[u + 1] - eb; e++) deg[u] += mark[col[e]];
    }
    int64_t tail = 0;
    for (int64_t i = 0; i < nS; i++) if (deg[order[i]] == 0) queue[tail++] = order[i];
    cnt[t] = 1;
    for (head = 0; head < tail; head++) {
        const int32_t v = queue[head];
        const int64_t r1 = v + 1 < V ? roff[v + 1] : E;
        for (int64_t r = roff[v]; r < r1; r++) {
            const int32_t to = etail[rev[r]];
            if (!mark[to]) continue;
            const int64_t c = cnt[to] + cnt[v];
            cnt[to] = c < a.k ? c : a.k;
            if (--deg[to] == 0) queue[tail++] = to;
        }
    }
    a.walks[g] = tail < nS ? a.k : cnt[s];
}

// ---- stage 1-2 under AASM_KSW_CYCLES: the tree of dijkstra() from the sink over the reversed graph (:185, :69-87) ---------------
// kb_sssp_dijkstra's formulation on the reversed lists: wave-uniform control, lane 0 stores; bedge[to] is the edge whose
// relaxation last set best[to].  CALC_SUM's third key is not monotone under addition (a larger qnz / qtot ratio is "smaller"),
// so a cycle can improve a distance for ever while the heap holds a few entries: the pushes are counted and a graph that makes
// more than 64 * (E + 2) of them ends with AASM_E_OVERFLOW (the reference does not return on it).  A graph whose heap room
// runs out first is marked ins = -1 and run again by the host with more.  The rest runs on lane 0 as kb_ksw_tree.
AASM_DEV void kb_ksw_tree_cyc(const KCtx &k, const KswArgs &a) {
    const int64_t g = k.bid;
    if (g >= a.n_graphs || k.tid >= AASM_WAVE) return;
    const int64_t cap = a.hoff[g + 1] - a.hoff[g];
    if (cap <= 0) return;                                            // solved with less heap room
    const int lane = k.lane;
    const int64_t vb = a.voff[g], V = a.voff[g + 1] - vb, eb = a.rowptr[vb], E = a.rowptr[vb + V] - eb;
    const int32_t t = a.sink[g];
    int32_t *roff = a.roff + vb, *best = a.best + vb, *bedge = a.bedge + vb;
    int32_t *rev = a.rev + eb, *etail = a.etail + eb;
    Dist *d = a.d + vb;
    if (lane == 0) ksw_cyc_prepare(a, g);
    wave_fence();
    DjEnt *H = a.dheap + a.hoff[g];
    const int64_t push_lim = AASM_KSW_DJ_PUSHES * (E + 2);
    int64_t n = 0, pushes = 0;
    int over = 0;                                                    // 1: heap room, 2: the bound on pushes
    auto push = [&](const Dist &dd, int32_t v) {
        if (++pushes > push_lim) { over = 2; return; }
        if (n >= cap) { over = 1; return; }
        dj_heap_push(H, n, lane, dd, v);
    };
    push(dist_zero(), t);
    while (n > 0 && !over) {
        const DjEnt top = dj_heap_pop(H, n, lane);
        const int32_t v = uni(top.v);
        const Dist dv = uni(top.d);
        if (!uni(dist_eq(dv, d[v]))) continue;                       // :77 (operator!=)
        const int64_t r0 = uni((int64_t)roff[v]), r1 = v + 1 < V ? uni((int64_t)roff[v + 1]) : E;
        for (int64_t r = r0; r < r1 && !over; r++) {
            const int32_t e = uni(rev[r]), to = uni(etail[e]);
            const Dist cand = uni(dist_add(dv, edge_w5(a.w5, eb + e)));
            if (uni(dist_lt<CALC_SUM_MODE>(cand, d[to]))) {          // d_[to] > dv + w (:79)
                if (lane == 0) { d[to] = cand; best[to] = v; bedge[to] = e; }
                wave_fence();
                push(cand, to);
            }
        }
    }
    if (lane != 0) return;
    a.nbfs[g] = 0; a.ins[g] = 0; a.walks[g] = 0;
    if (over) {
        a.status[g] = AASM_E_OVERFLOW;
        if (over == 1) a.ins[g] = -1;
        for (int64_t v = 0; v < V; v++) { d[v] = dist_max(); best[v] = -1; bedge[v] = -1; }
        d[t] = dist_zero();
        return;
    }
    ksw_cyc_tail(a, g);
}

// ---- stage 1-2 under AASM_KSW_CYCLES | AASM_KSW_NEGATIVE: the tree of bellman_ford() from the sink over the reversed graph (:186) --
// bf_spfa (aasm_sssp.h) on the reversed lists, bedge[to] again the edge whose relaxation last set best[to].  The queue room is exact
// (2 * (E + 2) entries, from the driver), so there are no retry rounds, and the algorithm always ends: dijkstra's bound on pushes
// does not apply.  A graph with a negative cycle has no distance vector in the reference (k_shortest_walks would index an empty
// one): AASM_E_INVAL, no walks, d / best as max / -1.  The rest runs on lane 0 as kb_ksw_tree_cyc.
AASM_DEV void kb_ksw_tree_bf(const KCtx &k, const KswArgs &a) {
    const int64_t g = k.bid;
    if (g >= a.n_graphs || k.tid >= AASM_WAVE) return;
    const int lane = k.lane;
    const int64_t vb = a.voff[g], V = a.voff[g + 1] - vb, eb = a.rowptr[vb], E = a.rowptr[vb + V] - eb;
    int32_t *roff = a.roff + vb, *best = a.best + vb, *bedge = a.bedge + vb;
    int32_t *rev = a.rev + eb, *etail = a.etail + eb;
    Dist *d = a.d + vb;
    if (lane == 0) ksw_cyc_prepare(a, g);
    wave_fence();
    int32_t at = -1;
    int64_t high = 0;
    const int st = bf_spfa<AASM_BF_CHUNK>(lane, V, a.sink[g], d, a.w5, a.dheap + a.hoff[g], a.hoff[g + 1] - a.hoff[g],
        [&](int32_t x, int64_t &r0, int64_t &r1) { r0 = uni((int64_t)roff[x]); r1 = x + 1 < V ? uni((int64_t)roff[x + 1]) : E; },
        [&](int64_t r, int64_t &e, int32_t &nx) { const int32_t el = rev[r]; e = eb + el; nx = etail[el]; },
        [&](int32_t nx, int32_t x, int64_t e) { best[nx] = x; bedge[nx] = (int32_t)(e - eb); }, at, high);
    if (lane != 0) return;
    a.nbfs[g] = 0; a.ins[g] = 0; a.walks[g] = 0;
    if (st != BF_DONE) {
        a.status[g] = st == BF_CYCLE ? AASM_E_INVAL : AASM_E_INTERNAL;
        for (int64_t v = 0; v < V; v++) { d[v] = dist_max(); best[v] = -1; bedge[v] = -1; }
        return;
    }
    ksw_cyc_tail(a, g);
}

// heap_insert (leftist_heap.hpp:29-40) without recursion: the right spine below which the key goes is walked down first,
// then the new leaf and the copies of the walked nodes are allocated bottom-up - the recursion's allocation order
AASM_DEV int32_t ksw_insert(KswNode *A, int64_t &n, int64_t cap, int32_t a, const Dist &key, int32_t e, bool &over) {
    int32_t path[AASM_KSW_SPINE];
    int m = 0;
    while (a >= 0 && dist_lt<CALC_SUM_MODE>(A[a].key, key)) {
        if (m == AASM_KSW_SPINE) { over = true; return -1; }
        path[m++] = a;
        a = A[a].right;
    }
    if (n + m + 1 > cap) { over = true; return -1; }
    int32_t cur = (int32_t)n;
    KswNode leaf; leaf.key = key; leaf.rank = 1; leaf.left = a; leaf.right = -1; leaf.e = e;
    A[n++] = leaf;
    for (int j = m - 1; j >= 0; j--) {
        const KswNode p = A[path[j]];
        int32_t l = p.left, r = cur;
        if (l < 0 || A[l].rank < A[r].rank) { const int32_t x = l; l = r; r = x; }
        KswNode c; c.key = p.key; c.rank = r >= 0 ? A[r].rank + 1 : 0; c.left = l; c.right = r; c.e = p.e;
        cur = (int32_t)n;
        A[n++] = c;
    }
    return cur;
}

// ---- stage 3: sidetrack heaps, BFS order from the sink (:196-215) -----------------------------------------------------
AASM_DEV void kb_ksw_heap(const KCtx &k, const KswArgs &a) {
    const int64_t g = k.bid;
    if (g >= a.n_graphs || k.tid != 0) return;
    const int64_t vb = a.voff[g], V = a.voff[g + 1] - vb, eb = a.rowptr[vb];
    int32_t *hroot = a.hroot + vb;
    for (int64_t v = 0; v < V; v++) hroot[v] = -1;
    a.hcount[g] = 0;
    if (a.status[g] != 0 || a.acap[g] <= 0) return;
    const int32_t *best = a.best + vb, *bfs = a.bfs + vb, *col = a.col + eb;
    const Dist *d = a.d + vb;
    const int64_t *rp = a.rowptr + vb;
    KswNode *A = a.arena + a.aoff[g];
    const int64_t cap = a.acap[g], nb = a.nbfs[g];
    int64_t n = 0;
    bool over = false;
    for (int64_t i = 0; i < nb && !over; i++) {
        const int32_t u = bfs[i];
        int32_t hu = best[u] >= 0 ? hroot[best[u]] : -1;             // h[p] = h[u] of the parent (:213)
        bool seen_p = false;
        for (int64_t e = rp[u] - eb; e < rp[u + 1] - eb && !over; e++) {
            const int32_t v = col[e];
            if (dist_is_max(d[v])) continue;
            const Dist c = dist_sub(dist_add(edge_w5(a.w5, eb + e), d[v]), d[u]);
            if (!seen_p && v == best[u] && ksw_is_ident(c)) { seen_p = true; continue; }   // we can only skip once
            hu = ksw_insert(A, n, cap, hu, c, (int32_t)e, over);
        }
        hroot[u] = hu;
    }
    a.hcount[g] = n;
    if (over) {
        a.status[g] = AASM_E_OVERFLOW;
        for (int64_t v = 0; v < V; v++) hroot[v] = -1;
    }
}

// ---- stage 4: k pops (:217-249) ------------------------------------------------------------------------------------------
AASM_DEV bool ksw_qe_less(const KswQE &x, const KswQE &y) {        // std::tuple operator< (std::greater makes it a min-queue)
    if (dist_lt<CALC_SUM_MODE>(x.d, y.d)) return true;
    if (dist_lt<CALC_SUM_MODE>(y.d, x.d)) return false;
    if (x.hp != y.hp) return x.hp < y.hp;
    return x.cur < y.cur;
}
// a distance the next additions keep inside int64 / int32 (never outside on a DAG of <= 2^20 vertices)
AASM_DEV bool ksw_in_range(const Dist &x) {
    const int64_t S = AASM_KSW_SAFE_SCORE;
    const int32_t C = AASM_KSW_SAFE_COUNT;
    return x.qry > -S && x.qry < S && x.ref > -S && x.ref < S && x.anom > -C && x.anom < C && x.qnz > -C && x.qnz < C && x.qtot > -C && x.qtot < C;
}
AASM_DEV void kb_ksw_enum(const KCtx &k, const KswArgs &a) {
    const int64_t g = k.bid;
    if (g >= a.n_graphs || k.tid != 0) return;
    a.nfound[g] = 0;
    if (a.status[g] != 0 || a.walks[g] <= 0) return;                 // d[source] == MAX: no walk (:188-189)
    const int64_t vb = a.voff[g], eb = a.rowptr[vb];
    const int32_t s = a.src[g];
    const int32_t *hroot = a.hroot + vb, *col = a.col + eb;
    const KswNode *A = a.arena + a.aoff[g];
    KswQE *Q = a.q + a.qoff[g];
    int32_t *nodes = a.qnode + a.qoff[g], *prev = a.qprev + a.qoff[g], *last = a.rlast + a.rofs[g];
    Dist *dist = a.rdist + a.rofs[g];
    const int64_t qcap = a.qcap[g], kk = a.walks[g] < a.k ? a.walks[g] : a.k;
    int64_t nf = 0, qn = 0, nn = 0;
    dist[nf] = a.d[vb + s]; last[nf] = -1; nf++;
    const int32_t hs = hroot[s];
    bool over = false;
    auto emplace = [&](const Dist &dd, int32_t hp, int32_t pre) {
        if (nn >= qcap || !ksw_in_range(dd)) { over = true; return; }
        KswQE x; x.d = dd; x.hp = hp; x.cur = (int32_t)nn; x.pad = 0;
        nodes[nn] = hp; prev[nn] = pre; nn++;
        int64_t i = qn++;
        while (i > 0) {                                              // sift up
            const int64_t p = (i - 1) >> 1;
            const KswQE pe = Q[p];
            if (!ksw_qe_less(x, pe)) break;
            Q[i] = pe;
            i = p;
        }
        Q[i] = x;
    };
    if (hs >= 0) {                                                   // (made even when k == 1, as the reference does)
        emplace(dist_add(dist[0], A[hs].key), hs, -1);
        while (qn > 0 && nf < kk && !over) {
            const KswQE top = Q[0];
            const KswQE x = Q[--qn];
            if (qn > 0) {                                            // the last entry sinks from the root
                int64_t i = 0;
                while (true) {
                    int64_t c = 2 * i + 1;
                    if (c >= qn) break;
                    KswQE ce = Q[c];
                    if (c + 1 < qn) { const KswQE c2 = Q[c + 1]; if (ksw_qe_less(c2, ce)) { ce = c2; c++; } }
                    if (!ksw_qe_less(ce, x)) break;
                    Q[i] = ce;
                    i = c;
                }
                Q[i] = x;
            }
            dist[nf] = top.d; last[nf] = top.cur; nf++;
            const KswNode ch = A[top.hp];
            const int32_t hv = hroot[col[ch.e]];
            if (hv >= 0) emplace(dist_add(top.d, A[hv].key), hv, top.cur);                                  // add value
            if (ch.left >= 0) emplace(dist_sub(dist_add(top.d, A[ch.left].key), ch.key), ch.left, prev[top.cur]);    // same heap
            if (ch.right >= 0) emplace(dist_sub(dist_add(top.d, A[ch.right].key), ch.key), ch.right, prev[top.cur]);
        }
    }
    a.nfound[g] = nf;
    if (over) a.status[g] = AASM_E_OVERFLOW;
}

// ---- stage 5: walk recovery (:252-290) as caller edge ids --------------------------------------------------------------
// A walk is source ->tree-> u_1 -side-> v_1 ->tree-> u_2 ... v_m ->tree-> sink, the tree segment from x to y taking
// depth[x] - depth[y] edges (the reference takes a sidetrack the first time it stands on its tail: best[] is a tree into the
// sink, so a tree path visits a vertex once - with cycles too, where the sink, at depth 0, may be a sidetrack's tail).  The
// sidetracks come off the prev chain last first, so a walk is written back to front.  Walk i holds at most i sidetracks.
AASM_DEV int64_t ksw_walk_len(const KswArgs &a, int64_t g, int64_t i) {
    const int64_t vb = a.voff[g], nf = a.nfound[g], eb = a.rowptr[vb];
    const int32_t *depth = a.depth + vb, *etail = a.etail + eb, *col = a.col + eb;
    const KswNode *A = a.arena + a.aoff[g];
    const int32_t *nodes = a.qnode + a.qoff[g], *prev = a.qprev + a.qoff[g];
    int64_t len = 0, stop = 0, steps = 0;
    for (int32_t c = a.rlast[a.rofs[g] + i]; c >= 0 && steps < nf; c = prev[c], steps++) {
        const int32_t e = A[nodes[c]].e;
        len += depth[col[e]] - stop + 1;
        stop = depth[etail[e]];
    }
    return len + depth[a.src[g]] - stop;
}
AASM_DEV void kb_ksw_count(const KCtx &k, const KswArgs &a) {
    const int64_t g = k.bid;
    if (g >= a.n_graphs || k.tid >= AASM_WAVE) return;
    const int64_t nf = a.nfound[g], per = (nf + AASM_WAVE - 1) / AASM_WAVE;
    const int64_t i0 = k.lane * per < nf ? k.lane * per : nf, i1 = i0 + per < nf ? i0 + per : nf;
    // under AASM_KSW_CYCLES a lane's sum saturates just above the cap on a graph's walk edges (a walk through a cycle has any length)
    const int64_t sat = a.cycles ? AASM_KSW_MAX_WALK_EDGES + 1 : INT64_MAX;
    int64_t sum = 0;
    for (int64_t i = i0; i < i1; i++) { const int64_t len = ksw_walk_len(a, g, i); sum = len < sat - sum ? sum + len : sat; }
    const int64_t incl = wave_incl_add(sum);
    const int64_t tot = wave_bcast(incl, AASM_WAVE - 1);
    if (tot >= sat) {                                                // the distances stay, the walks come back empty
        for (int64_t i = i0; i < i1; i++) a.woff[a.rofs[g] + i] = 0;
        if (k.lane == 0) { a.wtot[g] = 0; a.status[g] = AASM_E_OVERFLOW; }
        return;
    }
    int64_t at = incl - sum;
    for (int64_t i = i0; i < i1; i++) { a.woff[a.rofs[g] + i] = at; at += ksw_walk_len(a, g, i); }
    if (k.lane == 0) a.wtot[g] = tot;
}
AASM_DEV void kb_ksw_fill(const KCtx &k, const KswArgs &a) {
    const int64_t g = k.bid;
    if (g >= a.n_graphs || k.tid >= AASM_WAVE) return;
    const int64_t vb = a.voff[g], eb = a.rowptr[vb], nf = a.nfound[g];
    const int32_t *depth = a.depth + vb, *bedge = a.bedge + vb, *etail = a.etail + eb, *col = a.col + eb;
    const KswNode *A = a.arena + a.aoff[g];
    const int32_t *nodes = a.qnode + a.qoff[g], *prev = a.qprev + a.qoff[g];
    int64_t *out = a.wedges + a.wbase[g];
    const int64_t lim = a.wtot[g];
    if (lim <= 0) return;                                            // no edge to write (or the walks were capped)
    auto tree_seg = [&](int32_t x, int64_t from, int64_t n) {        // n tree edges from x into out[from, from + n)
        for (int64_t j = 0; j < n; j++) {
            const int32_t e = bedge[x];
            if (e < 0 || from + j < 0 || from + j >= lim) return;
            out[from + j] = eb + e;
            x = col[e];
        }
    };
    for (int64_t i = k.lane; i < nf; i += AASM_WAVE) {
        int64_t p = a.woff[a.rofs[g] + i] + ksw_walk_len(a, g, i);   // one past the walk's last edge
        int64_t stop = 0, steps = 0;
        for (int32_t c = a.rlast[a.rofs[g] + i]; c >= 0 && steps < nf; c = prev[c], steps++) {
            const int32_t e = A[nodes[c]].e, v = col[e];
            const int64_t n = depth[v] - stop;
            tree_seg(v, p - n, n);
            p -= n + 1;
            if (p >= 0 && p < lim) out[p] = eb + e;
            stop = depth[etail[e]];
        }
        const int32_t s = a.src[g];
        tree_seg(s, p - (depth[s] - stop), depth[s] - stop);
    }
}

// ---- host side: argument checks and the driver, shared by the product (aasm_gpu.hip) and the host emulation -----------
// Returns AASM_OK or the code, with a message in why: the graph-batch layout and the w5 weight domain of aasm_sssp.h, and k-walks' own
// bounds.
static inline int ksw_check_args(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5,
                                 const int32_t *source, const int32_t *sink, int64_t k, int flags, const aasm_ksw_out *out, const char **why) {
    int rc = check_graph_batch(n_graphs, g_voff, rowptr, col, source, {w5, sink, out}, why);
    if (rc != AASM_OK) return rc;
    if (k < 1 || k > AASM_KSW_MAX_K) return check_fail(why, AASM_E_INVAL, "k outside 1 .. 2^24");
    if (flags & ~(AASM_KSW_WALKS | AASM_KSW_TREE | AASM_KSW_CYCLES | AASM_KSW_NEGATIVE | AASM_KSW_HOOK_ARENA)) return check_fail(why, AASM_E_INVAL, "unknown flag");
    for (int64_t g = 0; g < n_graphs; g++) {
        const int64_t v0 = g_voff[g], v1 = g_voff[g + 1];
        if (sink[g] < 0 || sink[g] >= v1 - v0) return check_fail(why, AASM_E_INVAL, "graph " + std::to_string(g) + ": sink outside it");
        if (v1 - v0 > AASM_KSW_MAX_V) return check_fail(why, AASM_E_OVERFLOW, "graph " + std::to_string(g) + ": more than 2^20 vertices");
        if (rowptr[v1] - rowptr[v0] > INT32_MAX) return check_fail(why, AASM_E_OVERFLOW, "graph " + std::to_string(g) + ": 2^31 edges or more");
    }
    return check_w5(w5, rowptr[g_voff[n_graphs]], (flags & AASM_KSW_NEGATIVE) != 0, why);
}

static inline void ksw_free_out(aasm_ksw_out *o) {
    if (!o) return;
    free(o->n_found); free(o->dist5); free(o->walk_off); free(o->walk_edges); free(o->d5); free(o->best);
    free(o->heap_nodes); free(o->status); free(o->hook_arena); free(o->hook_hroot);
    memset(o, 0, sizeof(*o));
}

// The k-walk kernels, one 64-lane workgroup per graph of [g0, g1) (row shapes: aasm_dev.h); body(k, a)
#define AASM_KSW_KERNELS(K, ...)                    \
    K(KSW_K_TREE, aasm_ksw_tree, 64, 1, kb_ksw_tree)   \
    K(KSW_K_TREE_CYC, aasm_ksw_tree_cyc, 64, 1, kb_ksw_tree_cyc) \
    K(KSW_K_HEAP, aasm_ksw_heap, 64, 1, kb_ksw_heap)   \
    K(KSW_K_ENUM, aasm_ksw_enum, 64, 1, kb_ksw_enum)   \
    K(KSW_K_COUNT, aasm_ksw_count, 64, 1, kb_ksw_count) \
    K(KSW_K_FILL, aasm_ksw_fill, 64, 1, kb_ksw_fill)   \
    K(KSW_K_TREE_BF, aasm_ksw_tree_bf, 64, 1, kb_ksw_tree_bf)
enum { AASM_KSW_KERNELS(AASM_ROW_ID, AASM_ROW_ID) };
constexpr int ksw_block[] = {AASM_KSW_KERNELS(AASM_ROW_BLOCK, AASM_ROW_BLOCK)};
AASM_KERNEL_BODY(run_ksw_body, AASM_KSW_KERNELS, KswArgs)

// Backend BE: void *alloc(size_t) (nullptr = out of memory; freed with the backend), size_t mark() / release(mark) (free what
// was allocated since), bool h2d(dst, src, n), bool d2h(dst, src, n), bool launch_from(kernel, g0, g1, args) (blocks for the
// graphs [g0, g1), ordered on one stream), bool sync(), int err() (the code after a failure).
// Device memory per chunk of graphs stays under `budget` bytes unless one graph alone needs more.
template <class BE>
int ksw_run(BE &be, int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5,
            const int32_t *source, const int32_t *sink, int64_t k, int flags, aasm_ksw_out *out, int64_t budget) {
    const int64_t G = n_graphs, VT = g_voff[G], ET = rowptr[VT];
    KswArgs a;
    memset(&a, 0, sizeof(a));
    a.n_graphs = G; a.k = k;
    DevMem<BE> m{be};
    a.voff = (const int64_t *)m.up(g_voff, (size_t)(G + 1) * 8);
    a.rowptr = (const int64_t *)m.up(rowptr, (size_t)(VT + 1) * 8);
    a.col = (const int32_t *)m.up(col, (size_t)ET * 4);
    a.w5 = (const int64_t *)m.up(w5, (size_t)ET * 40);
    a.src = (const int32_t *)m.up(source, (size_t)G * 4);
    a.sink = (const int32_t *)m.up(sink, (size_t)G * 4);
    int32_t **v32[] = {&a.roff, &a.deg, &a.order, &a.best, &a.bedge, &a.koff, &a.kids, &a.bfs, &a.depth, &a.hroot};
    for (int32_t **p : v32) *p = (int32_t *)m.alloc((size_t)VT * 4);
    a.d = (Dist *)m.alloc((size_t)VT * sizeof(Dist));
    a.cnt = (int64_t *)m.alloc((size_t)VT * 8);
    a.rev = (int32_t *)m.alloc((size_t)ET * 4);
    a.etail = (int32_t *)m.alloc((size_t)ET * 4);
    a.status = (int32_t *)m.alloc((size_t)G * 4);
    int64_t **g64[] = {&a.nbfs, &a.ins, &a.walks, &a.hcount, &a.nfound, &a.wtot};
    for (int64_t **p : g64) *p = (int64_t *)m.alloc((size_t)G * 8);
    int64_t *d_aoff = (int64_t *)m.alloc((size_t)G * 8), *d_acap = (int64_t *)m.alloc((size_t)G * 8), *d_qoff = (int64_t *)m.alloc((size_t)G * 8);
    int64_t *d_qcap = (int64_t *)m.alloc((size_t)G * 8), *d_rofs = (int64_t *)m.alloc((size_t)G * 8), *d_wbase = (int64_t *)m.alloc((size_t)G * 8);
    a.aoff = d_aoff; a.acap = d_acap; a.qoff = d_qoff; a.qcap = d_qcap; a.rofs = d_rofs; a.wbase = d_wbase;
    if (!m.ok) return be.err();
    std::vector<int32_t> status((size_t)G);
    std::vector<int64_t> ins((size_t)G), walks((size_t)G);
    const bool cycles = flags & AASM_KSW_CYCLES;
    a.cycles = cycles;
    if (!cycles) {                                                   // (AASM_KSW_NEGATIVE: the DAG relaxation assumes no sign)
        if (!be.launch_from(KSW_K_TREE, 0, G, a)) return be.err();
    } else if (flags & AASM_KSW_NEGATIVE) {                          // bellman_ford_run's queue room (aasm_sssp.h): exact, one round
        const std::vector<int64_t> qo = bf_queue_offsets(G, g_voff, rowptr);
        const size_t mark = be.mark();
        a.hoff = (const int64_t *)m.up(qo.data(), (size_t)(G + 1) * 8);
        a.dheap = (DjEnt *)m.alloc((size_t)qo[(size_t)G] * sizeof(DjEnt));
        if (!m.ok || !be.launch_from(KSW_K_TREE_BF, 0, G, a) || !be.sync()) return be.err();
        be.release(mark);
        a.hoff = nullptr; a.dheap = nullptr;
    } else {
        // dijkstra_run's heap room (aasm_sssp.h): E + 2 entries, then 4x, 16x, 64x for the graphs that ran out of it; at 64x
        // the kernel's bound on pushes ends a graph first
        std::vector<char> todo((size_t)G, 1);
        for (int64_t mult = 1; mult <= AASM_KSW_DJ_PUSHES; mult *= 4) {
            std::vector<int64_t> ho((size_t)G + 1, 0);
            for (int64_t g = 0; g < G; g++)
                ho[(size_t)g + 1] = ho[(size_t)g] + (todo[(size_t)g] ? mult * (rowptr[g_voff[g + 1]] - rowptr[g_voff[g]] + 2) : 0);
            const size_t mark = be.mark();
            a.hoff = (const int64_t *)m.up(ho.data(), (size_t)(G + 1) * 8);
            a.dheap = (DjEnt *)m.alloc((size_t)ho[(size_t)G] * sizeof(DjEnt));
            if (!m.ok || !be.launch_from(KSW_K_TREE_CYC, 0, G, a) || !be.sync() || !be.d2h(status.data(), a.status, (size_t)G * 4) ||
                !be.d2h(ins.data(), a.ins, (size_t)G * 8)) return be.err();
            be.release(mark);
            a.hoff = nullptr; a.dheap = nullptr;
            bool again = false;
            for (int64_t g = 0; g < G; g++) again |= (todo[(size_t)g] = status[(size_t)g] == AASM_E_OVERFLOW && ins[(size_t)g] < 0);
            if (!again) break;
        }
    }
    if (!be.sync() || !be.d2h(status.data(), a.status, (size_t)G * 4) || !be.d2h(ins.data(), a.ins, (size_t)G * 8) ||
        !be.d2h(walks.data(), a.walks, (size_t)G * 8)) return be.err();
    for (int64_t g = 0; g < G; g++) if (ins[(size_t)g] < 0) ins[(size_t)g] = 0;
    // bounds from the device's counts: an insert copies at most the right spine of a version of <= ins keys
    // (<= floor(log2(ins + 1)) + 1 nodes) and adds a leaf; a pop emplaces at most three entries
    std::vector<int64_t> acap((size_t)G), qcap((size_t)G), per((size_t)G);
    for (int64_t g = 0; g < G; g++) {
        int64_t lg = 0;
        while (((int64_t)1 << (lg + 1)) <= ins[g] + 1) lg++;
        const int64_t bound = ins[g] * (lg + 2);
        acap[g] = status[g] == 0 && walks[g] > 0 ? (bound < INT32_MAX ? bound : INT32_MAX) : 0;   // no walk: no heaps (:188-189)
        qcap[g] = status[g] == 0 && walks[g] > 0 ? 3 * walks[g] - 2 : 0;
        per[g] = acap[g] * (int64_t)sizeof(KswNode) + qcap[g] * (int64_t)(sizeof(KswQE) + 8) + walks[g] * (int64_t)(sizeof(Dist) + 4 + 8);
    }
    // outputs
    const bool want_walks = flags & AASM_KSW_WALKS, want_tree = flags & AASM_KSW_TREE, want_arena = flags & AASM_KSW_HOOK_ARENA;
    memset(out, 0, sizeof(*out));
    out->n_graphs = G; out->k = k;
    out->n_found = (int64_t *)calloc((size_t)G, 8);
    out->dist5 = (int64_t *)calloc((size_t)(G * k * 5), 8);
    out->heap_nodes = (int64_t *)calloc((size_t)G, 8);
    out->status = (int32_t *)calloc((size_t)G, 4);
    if (want_walks) out->walk_off = (int64_t *)calloc((size_t)(G * k + 1), 8);
    if (want_tree) { out->d5 = (int64_t *)calloc((size_t)VT * 5, 8); out->best = (int32_t *)calloc((size_t)VT, 4); }
    if (want_arena) out->hook_hroot = (int32_t *)calloc((size_t)VT, 4);
    if (!out->n_found || !out->dist5 || !out->heap_nodes || !out->status || (want_walks && !out->walk_off) ||
        (want_tree && (!out->d5 || !out->best)) || (want_arena && !out->hook_hroot)) { ksw_free_out(out); return AASM_E_NOMEM; }
    std::vector<int64_t> wedges, arena_words;
    int64_t wdone = 0;
    std::vector<int64_t> aoff((size_t)G, 0), qoff((size_t)G, 0), rofs((size_t)G, 0), wbase((size_t)G, 0);
    auto fail = [&](int rc) { ksw_free_out(out); return rc; };
    auto down = [&](void *h, const void *d, size_t n) { return n == 0 || be.d2h(h, d, n); };   // (an empty vector's data() may be null)
    for (int64_t g0 = 0; g0 < G;) {
        int64_t g1 = g0, bytes = 0, na = 0, nq = 0, nr = 0;
        while (g1 < G && (g1 == g0 || bytes + per[g1] <= budget)) {
            aoff[g1] = na; qoff[g1] = nq; rofs[g1] = nr;
            na += acap[g1]; nq += qcap[g1]; nr += walks[g1]; bytes += per[g1]; g1++;
        }
        // graphs outside the chunk get no room: the kernels leave them alone
        std::vector<int64_t> cap_c((size_t)G, 0), qcap_c((size_t)G, 0);
        for (int64_t g = g0; g < g1; g++) { cap_c[g] = acap[g]; qcap_c[g] = qcap[g]; }
        const size_t mark = be.mark();
        KswArgs c = a;
        c.arena = (KswNode *)m.alloc((size_t)na * sizeof(KswNode));
        c.q = (KswQE *)m.alloc((size_t)nq * sizeof(KswQE));
        c.qnode = (int32_t *)m.alloc((size_t)nq * 4); c.qprev = (int32_t *)m.alloc((size_t)nq * 4);
        c.rdist = (Dist *)m.alloc((size_t)nr * sizeof(Dist)); c.rlast = (int32_t *)m.alloc((size_t)nr * 4);
        c.woff = (int64_t *)m.alloc((size_t)nr * 8);
        if (!m.ok) return fail(be.err());
        if (!be.h2d(d_aoff, aoff.data(), (size_t)G * 8) || !be.h2d(d_acap, cap_c.data(), (size_t)G * 8) || !be.h2d(d_qoff, qoff.data(), (size_t)G * 8) ||
            !be.h2d(d_qcap, qcap_c.data(), (size_t)G * 8) || !be.h2d(d_rofs, rofs.data(), (size_t)G * 8)) return fail(be.err());
        KswArgs cc = c;
        if (!be.launch_from(KSW_K_HEAP, g0, g1, cc) || !be.launch_from(KSW_K_ENUM, g0, g1, cc)) return fail(be.err());
        const int64_t ng = g1 - g0;
        std::vector<int64_t> nfound((size_t)ng), hcount((size_t)ng);
        std::vector<int32_t> st((size_t)ng);
        std::vector<Dist> rd((size_t)nr);
        if (!be.sync() || !be.d2h(nfound.data(), a.nfound + g0, (size_t)ng * 8) || !be.d2h(hcount.data(), a.hcount + g0, (size_t)ng * 8) ||
            !be.d2h(st.data(), a.status + g0, (size_t)ng * 4) || !down(rd.data(), c.rdist, (size_t)nr * sizeof(Dist))) return fail(be.err());
        for (int64_t g = g0; g < g1; g++) {
            const int64_t j = g - g0;
            out->n_found[g] = nfound[j]; out->heap_nodes[g] = hcount[j]; out->status[g] = st[j];
            for (int64_t i = 0; i < nfound[j]; i++) put_d5(out->dist5 + (g * k + i) * 5, rd[(size_t)(rofs[g] + i)]);
        }
        if (want_walks) {
            if (!be.launch_from(KSW_K_COUNT, g0, g1, cc)) return fail(be.err());
            std::vector<int64_t> wtot((size_t)ng);
            if (!be.sync() || !be.d2h(wtot.data(), a.wtot + g0, (size_t)ng * 8)) return fail(be.err());
            if (cycles) {                                            // a graph over the cap on walk edges: status from kb_ksw_count
                if (!be.d2h(st.data(), a.status + g0, (size_t)ng * 4)) return fail(be.err());
                for (int64_t g = g0; g < g1; g++) out->status[g] = st[(size_t)(g - g0)];
            }
            int64_t nw = 0;
            for (int64_t g = g0; g < g1; g++) { wbase[g] = nw; nw += wtot[g - g0]; }
            cc.wedges = (int64_t *)m.alloc((size_t)nw * 8);
            if (!m.ok) return fail(be.err());
            if (!be.h2d(d_wbase, wbase.data(), (size_t)G * 8) || !be.launch_from(KSW_K_FILL, g0, g1, cc)) return fail(be.err());
            std::vector<int64_t> wo((size_t)nr);
            wedges.resize((size_t)(wdone + nw));
            if (!be.sync() || !down(wo.data(), cc.woff, (size_t)nr * 8) || !down(wedges.data() + wdone, cc.wedges, (size_t)nw * 8)) return fail(be.err());
            for (int64_t g = g0; g < g1; g++) {
                const int64_t j = g - g0, base = wdone + wbase[g];
                for (int64_t i = 0; i < k; i++) out->walk_off[g * k + i] = base + (i < nfound[j] ? wo[(size_t)(rofs[g] + i)] : wtot[j]);
            }
            wdone += nw;
        }
        if (want_arena) {                                            // test hook: {rank, key[5], u, v, left, right} per node
            std::vector<KswNode> nodes((size_t)na);
            std::vector<int32_t> et((size_t)ET), cl((size_t)ET);
            if (!down(nodes.data(), c.arena, (size_t)na * sizeof(KswNode)) || !down(et.data(), a.etail, (size_t)ET * 4) ||
                !be.d2h(out->hook_hroot + g_voff[g0], a.hroot + g_voff[g0], (size_t)(g_voff[g1] - g_voff[g0]) * 4)) return fail(be.err());
            for (int64_t g = g0; g < g1; g++) {
                const int64_t eb = rowptr[g_voff[g]];
                for (int64_t i = 0; i < hcount[g - g0]; i++) {
                    const KswNode &nd = nodes[(size_t)(aoff[g] + i)];
                    const int64_t w[10] = {nd.rank, nd.key.qry, nd.key.ref, nd.key.anom, nd.key.qnz, nd.key.qtot, et[(size_t)(eb + nd.e)], col[eb + nd.e], nd.left, nd.right};
                    arena_words.insert(arena_words.end(), w, w + 10);
                }
            }
        }
        be.release(mark);
        g0 = g1;
    }
    if (want_walks) {
        out->walk_off[G * k] = wdone;
        out->walk_edges = (int64_t *)malloc((size_t)(wdone ? wdone : 1) * 8);
        if (!out->walk_edges) return fail(AASM_E_NOMEM);
        if (wdone) memcpy(out->walk_edges, wedges.data(), (size_t)wdone * 8);
    }
    if (want_arena) {
        out->hook_arena = (int64_t *)malloc((arena_words.size() ? arena_words.size() : 1) * 8);
        if (!out->hook_arena) return fail(AASM_E_NOMEM);
        if (!arena_words.empty()) memcpy(out->hook_arena, arena_words.data(), arena_words.size() * 8);
    }
    if (want_tree) {
        std::vector<Dist> hd((size_t)VT);
        if (!be.d2h(hd.data(), a.d, (size_t)VT * sizeof(Dist)) || !be.d2h(out->best, a.best, (size_t)VT * 4)) return fail(be.err());
        for (int64_t v = 0; v < VT; v++) put_d5(out->d5 + 5 * v, hd[(size_t)v]);
    }
    return AASM_OK;
}

}  // namespace aasm
