// aasm_sssp.h -- single-source shortest paths over a batch of caller graphs, and the checks of the layout that aasm_sssp_dijkstra,
// aasm_sssp_dial and aasm_k_shortest_walks share (include/alignasm_amd.h), run on the host before a device is touched.
// Kernel bodies in KCtx style, so tests/host_emul/graphs_emul.cpp compiles them for one lane on the host: kb_sssp_dijkstra, the solver's
// dijkstra() (row ★J), kb_sssp_bellman_ford, its bellman_ford() (row ★L), kb_sssp_dag, its topology_sort() and shortest_path_dag()
// (row ★M), and kb_sssp_dial, Dial's bucketed BFS (row K5); host drivers dijkstra_run / bellman_ford_run / dag_run / dial_run as
// ksw_run (aasm_ksw.h).
#pragma once
#include "aasm_dev.h"
#include "../../include/alignasm_amd.h"

namespace aasm {

struct DjEnt { Dist d; int32_t v, p0, p1, p2; };
#define DIAL_WIN 256
#define DIAL_MAXB 8
struct DialLds { int32_t ring[DIAL_MAXB][DIAL_WIN]; };

struct SsspArgs {
    int64_t n_graphs;
    const int64_t *voff, *rowptr;                       // caller layout (global vertex / edge ids)
    const int32_t *col, *src;
    const int64_t *w5, *hoff; Dist *d; int32_t *prv; DjEnt *heap;            // dijkstra: graph g's heap is [hoff[g], hoff[g + 1])
    const int32_t *cost; int32_t nb; int64_t *dist, *pre; int32_t *spill;    // dial: nb = lim + 1 stacks in graph g's spill,
    const int64_t *soff;                                                     //       [soff[g], soff[g + 1])
    // bellman_ford: graph g's queue ring is [hoff[g], hoff[g + 1]) of heap; its cycle goes to cyc[voff[g] + g ...], clen[g] entries
    int32_t *status, *cyc, *mark; int64_t *clen, *qhigh;
    // dag: in-degrees in mark, the Kahn order (and FIFO) in order, the first improving lane of a head in claim; w5 == nullptr is the
    // sort alone (no src, d, prv, claim)
    int32_t *order, *claim;
};

AASM_DEV Dist edge_w5(const int64_t *w5, int64_t e) {
    Dist r; r.qry = w5[5 * e]; r.ref = w5[5 * e + 1]; r.anom = (int32_t)w5[5 * e + 2]; r.qnz = (int32_t)w5[5 * e + 3];
    r.qtot = (int32_t)w5[5 * e + 4]; r.pad = 0; return r;
}

// ---- generic SSSP: the solver's dijkstra() (k_shortest_walks.hpp:69-87) ------------------------------
// The reference's CLI never reaches it (is_dag = true, paf_data.cpp:728: the shortest-path tree is the DAG
// relaxation, K6), but the solver class offers it for graphs with cycles and BASELINE.json's north_star names it.
// One wave per graph, wave-uniform control: a binary min-heap of (Distance, vertex) in global memory with the
// reference's order (std::greater on std::pair: PafDistance operator< in CALC_SUM mode, then the vertex), lazy
// deletion by `dv != d[v]` (operator==), strict `d[to] > dv + w` relaxation of the popped vertex's list in list
// order (sequential: a list may name a vertex twice).  Results equal the reference's d[] and prev[] exactly.
AASM_DEV bool dj_ent_less(const DjEnt &a, const DjEnt &b) {         // std::pair<Distance, int64_t> operator<
    if (dist_lt<CALC_SUM_MODE>(a.d, b.d)) return true;
    if (dist_lt<CALC_SUM_MODE>(b.d, a.d)) return false;
    return a.v < b.v;
}
// The binary min-heap of dijkstra(), shared with k-walks' tree kernel (aasm_ksw.h): all lanes hold the same n and entry, lane 0 stores.
// dj_heap_push: the caller has checked n < capacity.  dj_heap_pop: n > 0; returns the top.
AASM_DEV void dj_heap_push(DjEnt *H, int64_t &n, int lane, const Dist &dd, int32_t v) {
    DjEnt x; x.d = dd; x.v = v; x.p0 = x.p1 = x.p2 = 0;
    int64_t i = n++;
    while (i > 0) {
        const int64_t p = (i - 1) >> 1;
        const DjEnt pe = H[p];
        if (!uni(dj_ent_less(x, pe))) break;
        if (lane == 0) H[i] = pe;
        wave_fence();
        i = p;
    }
    if (lane == 0) H[i] = x;
    wave_fence();
}
AASM_DEV DjEnt dj_heap_pop(DjEnt *H, int64_t &n, int lane) {
    const DjEnt top = H[0];
    const DjEnt x = H[--n];
    if (n > 0) {                                                     // the last entry sinks from the root
        int64_t i = 0;
        while (true) {
            int64_t c = 2 * i + 1;
            if (c >= n) break;
            DjEnt ce = H[c];
            if (c + 1 < n) { const DjEnt ce2 = H[c + 1]; if (uni(dj_ent_less(ce2, ce))) { ce = ce2; c++; } }
            if (!uni(dj_ent_less(ce, x))) break;
            if (lane == 0) H[i] = ce;
            wave_fence();
            i = c;
        }
        if (lane == 0) H[i] = x;
        wave_fence();
    }
    return top;
}
AASM_DEV void kb_sssp_dijkstra(const KCtx &k, const SsspArgs &a) {
    const int64_t g = k.bid;
    if (g >= a.n_graphs) return;
    const int lane = k.lane;
    const int64_t vb = a.voff[g], V = a.voff[g + 1] - vb;
    Dist *dg = a.d + vb;
    int32_t *pg = a.prv + vb;
    DjEnt *H = a.heap + a.hoff[g];
    for (int64_t v = lane; v < V; v += AASM_WAVE) { dg[v] = dist_max(); pg[v] = -1; }
    wave_fence();
    int64_t n = 0;
    const int64_t cap = a.hoff[g + 1] - a.hoff[g];
    bool over = false;
    auto push = [&](const Dist &dd, int32_t v) {
        if (n >= cap) { over = true; return; }                       // more relaxations than edges: a cycle keeps improving the order (the reference would not return)
        dj_heap_push(H, n, lane, dd, v);
    };
    const int32_t s = a.src[g];
    if (lane == 0) dg[s] = dist_zero();                              // IDENTITY_DISTANCE (:74)
    wave_fence();
    push(dist_zero(), s);
    while (n > 0 && !over) {
        const DjEnt top = dj_heap_pop(H, n, lane);
        const int32_t v = uni(top.v);
        const Dist dv = uni(top.d);
        if (!uni(dist_eq(dv, dg[v]))) continue;                      // :79 (operator!=)
        for (int64_t e = a.rowptr[vb + v]; e < a.rowptr[vb + v + 1]; e++) {
            const int32_t to = uni(a.col[e]);
            const Dist cand = uni(dist_add(dv, edge_w5(a.w5, e)));
            if (uni(dist_lt<CALC_SUM_MODE>(cand, dg[to]))) {         // d_[to] > dv + w (:81)
                if (lane == 0) { dg[to] = cand; pg[to] = v; }
                wave_fence();
                push(cand, to);
            }
        }
    }
    if (over && lane == 0) pg[s] = -2;                               // reported by the host driver
}

// ---- generic SSSP with negative weights: the solver's bellman_ford() (k_shortest_walks.hpp:91-129) --------------------------------
// The reference's round-counted SPFA restated exactly, because prv[] depends on the order of the relaxations: a FIFO queue of
// (Distance, vertex) that starts with (IDENTITY, src); rounds i = 1 .. n, each popping exactly the entries present at its start; an
// entry is skipped when cur_dis > dis[x] (:114; an equal one is not); the edges of x in list order under the strict test
// `dis[nx] > dis[x] + w` (:116) with dis[x] as it stands at that moment (a self-loop may have improved it), the stored value being
// dis[x] + w; a relaxation in round n ends the graph as "negative cycle" after dis / prv are stored (:119-122), any other pushes
// (dis[nx], nx).  Unlike dijkstra() it always ends: the mapq-ratio key is not monotone under addition, so a graph can keep improving
// round a cycle whose score sum is not negative; the reference reports a cycle there at round n, and so does this.
//
// One wave per graph, wave-uniform control, lane 0 stores.  The popped vertex's list is taken AASM_BF_CHUNK edges at a time: each
// lane loads its edge's head, its weight and dis[head] and forms the strict predicate with dis[x]; one ballot decides the chunk (no
// improving lane: one step, the common case after the first rounds).  The improving lanes are committed in lane order, each
// re-tested against the current dis[head] and dis[x], because heads repeat inside a chunk and an edge can lead back to x.  A lane
// that did not improve at the chunk's start cannot improve later in it - dis[] only falls in the order, which is a strict weak
// order inside the w5 domain - unless dis[x] itself fell: after a commit to x the rest of the chunk is evaluated again from the next
// edge.  So the result is bit for bit what one lane walking the list leaves; with one lane (the host emulation) a chunk is one edge,
// which is that walk.  -DAASM_BF_EDGEWISE (tools/bf_probe.py's comparison build) takes one edge per step on the device too.
//
// Queue room.  An entry of x is live (not skipped) only while its distance is still dis[x], and the pushes of one vertex fall
// strictly, so at any moment at most one queued entry per vertex is live - but stale ones remain queued.  A round pops what its
// start holds and relaxes each live vertex's list once: at most one push per edge, E per round.  The queue therefore holds at
// most the E entries of the previous round (1 in the first) plus the E of this one: <= 2E + 1 < 2 * (E + 2), the room the drivers
// give.  The room is still checked before every write; a graph that runs out of it ends as BF_QUEUE_FULL (AASM_E_INTERNAL).
#if defined(AASM_BF_EDGEWISE)
#define AASM_BF_CHUNK 1
#else
#define AASM_BF_CHUNK AASM_WAVE
#endif
enum { BF_DONE = 0, BF_CYCLE = 1, BF_QUEUE_FULL = 2 };
// row(x, r0, r1): x's list as positions; edge(r, e, nx): position r's edge id in w5 and its head; commit(nx, x, e): lane 0's stores
// beside dis[nx] (prv, and the edge for k-walks).  cyc_at: the vertex relaxed in round n; high: the queue's high-water mark.
template <int W, class Row, class Edge, class Commit>
AASM_DEV int bf_spfa(int lane, int64_t n, int32_t s, Dist *dis, const int64_t *w5, DjEnt *Q, int64_t cap, Row row, Edge edge, Commit commit,
                     int32_t &cyc_at, int64_t &high) {
    int64_t qh = 0, cnt = 0;
    high = 0;
    auto push = [&](const Dist &dd, int32_t v) {
        if (cnt >= cap) return false;
        int64_t at = qh + cnt;
        if (at >= cap) at -= cap;
        if (lane == 0) { DjEnt x; x.d = dd; x.v = v; x.p0 = x.p1 = x.p2 = 0; Q[at] = x; }
        wave_fence();
        if (++cnt > high) high = cnt;
        return true;
    };
    if (lane == 0) dis[s] = dist_zero();                             // IDENTITY_DISTANCE (:109)
    wave_fence();
    if (!push(dist_zero(), s)) return BF_QUEUE_FULL;
    for (int64_t i = 1; i <= n && cnt > 0; i++) {
        const int64_t sz = cnt;
        for (int64_t j = 0; j < sz; j++) {
            const DjEnt ent = Q[qh];
            if (++qh == cap) qh = 0;
            cnt--;
            const int32_t x = uni(ent.v);
            const Dist cur = uni(ent.d);
            Dist dx = uni(dis[x]);
            if (uni(dist_lt<CALC_SUM_MODE>(dx, cur))) continue;      // cur_dis > dis[x] (:114)
            int64_t r0, r1;
            row(x, r0, r1);
            while (r0 < r1) {
                const int64_t r = r0 + (W > 1 ? lane : 0);
                bool imp = false;
                if (r < r1) {
                    int64_t e; int32_t nx;
                    edge(r, e, nx);
                    imp = dist_lt<CALC_SUM_MODE>(dist_add(dx, edge_w5(w5, e)), dis[nx]);
                }
                uint64_t m = wave_ballot(imp);
                if (W == 1) m &= 1;                                  // every lane holds the same edge
                int64_t next = r0 + W;
                while (m) {
                    const int jl = ffs64(m) - 1;                     // the improving lanes in lane order = list order
                    m &= m - 1;
                    int64_t e; int32_t nx;
                    edge(r0 + jl, e, nx);
                    e = uni(e); nx = uni(nx);
                    const Dist cand = uni(dist_add(dx, edge_w5(w5, e)));
                    if (!uni(dist_lt<CALC_SUM_MODE>(cand, dis[nx]))) continue;   // dis[nx] > dis[x] + w (:116), as they stand now
                    if (lane == 0) { dis[nx] = cand; commit(nx, x, e); }
                    wave_fence();
                    if (i == n) { cyc_at = nx; return BF_CYCLE; }    // :119-122
                    if (!push(cand, nx)) return BF_QUEUE_FULL;
                    if (nx == x) { dx = cand; next = r0 + jl + 1; break; }       // dis[x] fell: the rest of the chunk again
                }
                r0 = next;
            }
        }
    }
    return BF_DONE;
}
// detect_cycle(x) (:94-107) on one lane: follow prv from x until a vertex repeats; the list is closed (first entry == last entry)
// and runs in edge direction.  mark[] is 0 on entry; out has room for n + 1.  Returns the length, or 0 when the chain meets -1
// before it repeats a vertex (the reference would index out of bounds there).
AASM_DEV int64_t bf_cycle(int64_t n, const int32_t *prv, int32_t *mark, int32_t x, int32_t *out) {
    int64_t m = 0;
    while (true) {
        if (x < 0 || m > n) return 0;
        out[m] = x;
        if (mark[x]) break;
        mark[x] = (int32_t)m + 1;
        m++;
        x = prv[x];
    }
    const int64_t first = mark[x] - 1, len = m - first + 1;          // out[first] == out[m]: reversed, [m .. first] is the answer
    for (int64_t i = first, j = m; i < j; i++, j--) { const int32_t t = out[i]; out[i] = out[j]; out[j] = t; }
    for (int64_t i = 0; i < len; i++) out[i] = out[first + i];
    return len;
}
AASM_DEV void kb_sssp_bellman_ford(const KCtx &k, const SsspArgs &a) {
    const int64_t g = k.bid;
    if (g >= a.n_graphs) return;
    const int lane = k.lane;
    const int64_t vb = a.voff[g], V = a.voff[g + 1] - vb;
    Dist *dg = a.d + vb;
    int32_t *pg = a.prv + vb, *mark = a.mark + vb;
    for (int64_t v = lane; v < V; v += AASM_WAVE) { dg[v] = dist_max(); pg[v] = -1; mark[v] = 0; }
    wave_fence();
    int32_t at = -1;
    int64_t high = 0;
    const int st = bf_spfa<AASM_BF_CHUNK>(lane, V, a.src[g], dg, a.w5, a.heap + a.hoff[g], a.hoff[g + 1] - a.hoff[g],
        [&](int32_t x, int64_t &r0, int64_t &r1) { r0 = uni(a.rowptr[vb + x]); r1 = uni(a.rowptr[vb + x + 1]); },
        [&](int64_t r, int64_t &e, int32_t &nx) { e = r; nx = a.col[r]; },
        [&](int32_t nx, int32_t x, int64_t) { pg[nx] = x; }, at, high);
    if (st == BF_DONE) {
        if (lane == 0) { a.status[g] = 0; a.clen[g] = 0; a.qhigh[g] = high; }
        return;
    }
    if (lane == 0) {
        const int64_t len = st == BF_CYCLE ? bf_cycle(V, pg, mark, at, a.cyc + vb + g) : 0;
        a.status[g] = st == BF_QUEUE_FULL ? AASM_E_INTERNAL : len ? 1 : AASM_E_INVAL;
        a.clen[g] = len; a.qhigh[g] = high;
    }
    wave_fence();
    for (int64_t v = lane; v < V; v += AASM_WAVE) { dg[v] = dist_max(); pg[v] = -1; }   // the reference returns no distance vector
}

// ---- the solver's topology_sort() and shortest_path_dag() (k_shortest_walks.hpp:132-156, :160-175) ------------------------------
// The two the reference's command line reaches (is_dag = true, paf_data.cpp:728), as an entry from a SOURCE over the caller's own
// lists; kb_ksw_tree (aasm_ksw.h) keeps its own copy on lane 0, from the sink over the reversed graph, and is not routed through
// this.  Kahn's algorithm with a FIFO: the vertices of in-degree 0 in ascending id, then a vertex when its last in-edge is
// processed, "last" in (queue position of the tail, list position); parallel edges count once each.  The relaxation walks the
// finished order, skips a vertex whose distance == max() (:166) and takes each list in list order under the strict test
// `d[to] > d[v] + w` (:168), so the first candidate in (Kahn position of the tail, list position) among equals stays, with its own
// five numbers.  A vertex's distance is final when it leaves the queue (every in-edge's tail left before it), so the two passes are
// fused: a vertex is relaxed when it is popped.  On a cycle the reference asserts (:144-147); built with NDEBUG it returns an empty
// order and relaxes nothing, which is what status 1 gives back: order -1, d max() but IDENTITY at src, prv -1.
//
// One wave per graph, wave-uniform control, order[] itself the FIFO (head, tail), every loop bounded by V or E, and every cell of
// working memory (in-degrees, claim, d, prv, order) written here before it is read.  In-degrees: a lane per edge, atomic adds.
// Sources: 64 vertices at a time, a ballot and a prefix count keep ascending id.  The popped vertex's list, AASM_DAG_CHUNK edges at
// a time (as bf_spfa's):
//  1. every lane takes its edge's head off the in-degree (atomically: heads repeat) and reads it back; the lanes that read 0 hold
//     the heads that became ready in this chunk - an in-degree reaches 0 once, with the vertex's last in-edge, so a head that
//     repeats across chunks of the list is ready only in the chunk of its last edge.  They are appended in lane order = list order,
//     a head that repeats inside the chunk by its LAST lane only.
//  2. d[u] is fixed for the whole list (the graph is acyclic, or the results are reset), so every lane forms d[u] + w and the strict
//     predicate at once.  The improving lanes take the minimum of their lane ids on claim[head]: a lane that does not read its own
//     id back shares its head with an earlier improving lane.  Heads named by one improving lane are stored in parallel; the lanes
//     of a shared head are settled in lane order by lane 0, each re-tested against the value as it then stands, so the first of
//     equals stays.  (A lane that did not improve at the chunk's start cannot improve later in it: d[] only falls.)
//  3. a popped vertex at max() relaxes nothing and still counts down its heads.
// With one lane (the host emulation) a chunk is one edge, the reference's own walk.  -DAASM_DAG_EDGEWISE (tools/dag_probe.py's
// comparison build) takes one edge per step on the device too: lane 0 alone holds an edge.
#if defined(AASM_DAG_EDGEWISE)
#define AASM_DAG_CHUNK 1
#else
#define AASM_DAG_CHUNK AASM_WAVE
#endif
enum { DAG_DONE = 0, DAG_CYCLE = 1 };
template <int W>
AASM_DEV void dag_sort_relax(const KCtx &k, const SsspArgs &a) {
    const int64_t g = k.bid;
    if (g >= a.n_graphs) return;
    const int lane = k.lane;
    const bool relax = a.w5 != nullptr;                              // false: topology_sort() alone
    const int64_t vb = a.voff[g], V = a.voff[g + 1] - vb, e0 = a.rowptr[vb], e1 = a.rowptr[vb + V];
    const int64_t *rp = a.rowptr + vb;
    int32_t *deg = a.mark + vb, *order = a.order + vb;
    Dist *dg = relax ? a.d + vb : nullptr;
    int32_t *pg = relax ? a.prv + vb : nullptr, *claim = relax ? a.claim + vb : nullptr;
    const int32_t s = relax ? a.src[g] : 0;
    for (int64_t v = lane; v < V; v += AASM_WAVE) {
        deg[v] = 0; order[v] = -1;
        if (relax) { dg[v] = dist_max(); pg[v] = -1; claim[v] = INT32_MAX; }
    }
    wave_fence();
    for (int64_t e = e0 + lane; e < e1; e += AASM_WAVE) atomic_add(&deg[a.col[e]], (int32_t)1);   // :135-137
    if (relax && lane == 0) dg[s] = dist_zero();                     // IDENTITY_DISTANCE (:163)
    wave_fence();
    int64_t head = 0, tail = 0;
    for (int64_t v0 = 0; v0 < V; v0 += AASM_WAVE) {                  // :139-141, ascending id
        const int64_t v = v0 + lane;
        const bool src0 = v < V && ld_shared_i32(&deg[v]) == 0;
        const uint64_t m = wave_ballot(src0);
        if (src0) order[tail + popc64(m & lanemask_lt(lane))] = (int32_t)v;
        tail += popc64(m);
    }
    wave_fence();
    while (head < tail) {                                            // at most V pops: a vertex is appended once
        const int32_t u = uni(order[head++]);
        Dist du = dist_max();
        if (relax) du = uni(dg[u]);
        const bool live = relax && !dist_is_max(du);                 // :166
        const int64_t r1 = uni(rp[u + 1]);
        for (int64_t r0 = uni(rp[u]); r0 < r1; r0 += W) {
            const int64_t r = r0 + (W > 1 ? lane : 0);
            const bool act = r < r1 && (W > 1 || lane == 0);
            const int32_t to = act ? a.col[r] : -1;
            // 1. the countdown (:151-153)
            if (act) atomic_add(&deg[to], (int32_t)-1);
            wave_fence();
            const bool ready = act && ld_shared_i32(&deg[to]) == 0;
            for (uint64_t m = wave_ballot(ready); m; m &= m - 1) {
                const int j = ffs64(m) - 1;
                const int32_t h = wave_readlane(to, j);
                if ((wave_ballot(ready && to == h) >> j) >> 1) continue;   // a later lane names h again: that one appends it
                if (tail < V) { if (lane == 0) order[tail] = h; tail++; }
            }
            // 2. the relaxation (:167-172)
            if (live) {
                Dist cand = du;
                bool imp = false;
                if (act) { cand = dist_add(du, edge_w5(a.w5, r)); imp = dist_lt<CALC_SUM_MODE>(cand, dg[to]); }
                if (wave_ballot(imp)) {
                    if (imp) atomic_min_i32(&claim[to], (int32_t)lane);
                    wave_fence();
                    const bool first = imp && ld_shared_i32(&claim[to]) == lane;
                    bool shared = false;
                    for (uint64_t f = wave_ballot(imp && !first); f;) {          // the heads that several improving lanes name
                        const int32_t h = wave_readlane(to, ffs64(f) - 1);
                        shared |= imp && to == h;
                        f &= ~wave_ballot(to == h);
                    }
                    if (imp && !shared) { dg[to] = cand; pg[to] = u; }
                    if (first) claim[to] = INT32_MAX;
                    wave_fence();
                    for (uint64_t m = wave_ballot(shared); m; m &= m - 1) {      // in lane order = list order
                        const int j = ffs64(m) - 1;
                        const int32_t h = wave_readlane(to, j);
                        const Dist c = uni(dist_add(du, edge_w5(a.w5, r0 + j)));
                        if (!uni(dist_lt<CALC_SUM_MODE>(c, dg[h]))) continue;    // d[to] > d[v] + w, as it stands now
                        if (lane == 0) { dg[h] = c; pg[h] = u; }
                        wave_fence();
                    }
                }
            }
        }
        wave_fence();                                                // order[] written by lane 0, read by every lane
    }
    if (tail < V) {                                                  // a cycle: the empty order, nothing relaxed (:144-147)
        for (int64_t v = lane; v < V; v += AASM_WAVE) {
            order[v] = -1;
            if (relax) { dg[v] = v == s ? dist_zero() : dist_max(); pg[v] = -1; }
        }
    }
    if (lane == 0) a.status[g] = tail < V ? DAG_CYCLE : DAG_DONE;
}
AASM_DEV void kb_sssp_dag(const KCtx &k, const SsspArgs &a) { dag_sort_relax<AASM_DAG_CHUNK>(k, a); }

// ---- Dial's bucketed BFS (k_weighted_bfs.hpp:16-37), one wave per graph -------------------------------------------------
// The reference keeps lim + 1 circular buckets, each a LIFO stack, and walks d = 0, 1, ...: pop the top of bucket d mod (lim + 1),
// skip it when its distance is stale, relax its out-edges in list order; a successful relaxation (dist[nxt] == -1 or > d + cost)
// sets dist / pre and pushes nxt onto bucket (d + cost) mod (lim + 1).  dist is order-independent, pre is not: it names the FIRST
// vertex, in the reference's pop order, that reached the final distance - so the pops stay sequential and the relaxations of ONE
// popped row run on the lanes:
//  * buckets staged in LDS (k.lds, a DialLds): every stack's top DIAL_WIN entries live in an LDS ring (ring slot = stack position
//    mod DIAL_WIN); a full ring spills its lower half to the stack's slice of global memory in one coalesced store, an empty one
//    refills from it;
//  * a row is relaxed a wave of edges at a time; the lanes that succeed are compacted PER BUCKET by ballot + prefix count, so a
//    chunk's pushes land on every stack in list order (what the LIFO pops then reverse, as in the reference);
//  * a chunk that names a head twice (parallel edges) is relaxed edge by edge - the second edge must see the first one's result.
//    With one lane (the host emulation) a chunk is one edge, the reference's own order.
// The solver drives it with lim = 2 on the anomaly weights and keeps one scalar (paf_data.cpp:704-715), which the pipeline folds
// into its forward sweep; this entry is the algorithm itself, for any digraph (cycles allowed) and weights 0 .. lim <= 7.
AASM_DEV void kb_sssp_dial(const KCtx &k, const SsspArgs &a) {
    AASM_LDS_VIEW DialLds &L = *(AASM_LDS_VIEW DialLds *)k.lds;
    const int64_t g = k.bid;
    if (g >= a.n_graphs) return;
    const int lane = k.lane;
    const int32_t nb = a.nb;
    const int64_t vb = a.voff[g], V = a.voff[g + 1] - vb;
    int64_t *dg = a.dist + vb, *pg = a.pre + vb;
    const int64_t cap = (a.soff[g + 1] - a.soff[g]) / nb;            // per bucket
    int32_t *sp = a.spill + a.soff[g];
    for (int64_t v = lane; v < V; v += AASM_WAVE) { dg[v] = -1; pg[v] = -1; }
    wave_fence();
    int32_t base[DIAL_MAXB], cnt[DIAL_MAXB];                        // stack b = global [0, base) + ring [base, base + cnt)
    AASM_UNROLL
    for (int b = 0; b < DIAL_MAXB; b++) { base[b] = 0; cnt[b] = 0; }
    bool over = false;
    // room for m more entries on stack b (m <= AASM_WAVE): spill the lower half of a ring that would overflow
    auto make_room = [&](int b, int32_t m) {
        AASM_UNROLL
        for (int bb = 0; bb < DIAL_MAXB; bb++) if (bb == b && cnt[bb] + m > DIAL_WIN) {
            const int32_t n = DIAL_WIN / 2;
            if ((int64_t)base[bb] + n > cap) { over = true; return; }
            for (int32_t t = lane; t < n; t += AASM_WAVE) sp[(int64_t)bb * cap + base[bb] + t] = L.ring[bb][(base[bb] + t) & (DIAL_WIN - 1)];
            base[bb] += n; cnt[bb] -= n;
        }
    };
    auto push_lanes = [&](int b, bool mine, int32_t v) {             // the lanes with `mine` push v onto stack b, in lane order
        const uint64_t m = wave_ballot(mine);
        if (!m) return;
        make_room(b, popc64(m));
        if (over) return;
        AASM_UNROLL
        for (int bb = 0; bb < DIAL_MAXB; bb++) if (bb == b) {
            if (mine) L.ring[bb][(base[bb] + cnt[bb] + popc64(m & lanemask_lt(lane))) & (DIAL_WIN - 1)] = v;
            cnt[bb] += popc64(m);
        }
        wave_fence();
    };
    const int32_t s0 = a.src[g];
    if (lane == 0) dg[s0] = 0;
    push_lanes(0, lane == 0, s0);
    int64_t maxd = 0;
    for (int64_t d = 0; d <= maxd && !over; d++) {
        const int b = (int)(d % nb);
        while (!over) {
            int32_t c_b = 0, b_b = 0;
            AASM_UNROLL
            for (int bb = 0; bb < DIAL_MAXB; bb++) if (bb == b) { c_b = cnt[bb]; b_b = base[bb]; }
            if (c_b == 0) {
                if (b_b == 0) break;                                 // the bucket is empty
                const int32_t n = b_b < DIAL_WIN / 2 ? b_b : DIAL_WIN / 2;   // refill the ring from the stack's global part
                for (int32_t t = lane; t < n; t += AASM_WAVE) L.ring[b][(b_b - n + t) & (DIAL_WIN - 1)] = sp[(int64_t)b * cap + b_b - n + t];
                wave_fence();
                AASM_UNROLL
                for (int bb = 0; bb < DIAL_MAXB; bb++) if (bb == b) { base[bb] -= n; cnt[bb] += n; }
                continue;
            }
            const int32_t cur = uni(L.ring[b][(b_b + c_b - 1) & (DIAL_WIN - 1)]);   // q.back(); q.pop_back()
            AASM_UNROLL
            for (int bb = 0; bb < DIAL_MAXB; bb++) if (bb == b) cnt[bb]--;
            const int64_t dc = dg[cur];
            if (uni((int32_t)(dc != d))) continue;                   // stale (:24)
            const int64_t r0 = a.rowptr[vb + cur], r1 = a.rowptr[vb + cur + 1];
            for (int64_t e0 = r0; e0 < r1 && !over; e0 += AASM_WAVE) {
                const int64_t e = e0 + lane;
                const bool act = e < r1;
                const int32_t nxt = act ? a.col[e] : -1 - lane;
                const int32_t cs = act ? a.cost[e] : 0;
                // a head named twice in this chunk?  (lane i looks at the lanes below it)
                bool dup = false;
                const int32_t nlan = (int32_t)((r1 - e0 < AASM_WAVE) ? (r1 - e0) : AASM_WAVE);
                for (int32_t j = 0; j + 1 < nlan; j++) dup |= (lane > j) && (wave_readlane(nxt, j) == nxt);
                if (wave_ballot(dup)) {                              // edge by edge, as the reference (:25-32)
                    for (int32_t j = 0; j < nlan && !over; j++) {
                        const int32_t nj = wave_readlane(nxt, j), cj = wave_readlane(cs, j);
                        const int64_t nd = d + cj, dn = dg[nj];
                        const bool ok = uni((int32_t)(dn == -1 || dn > nd)) != 0;
                        if (!ok) continue;
                        if (lane == 0) { dg[nj] = nd; pg[nj] = cur; }
                        wave_fence();
                        push_lanes((int)(nd % nb), lane == 0, nj);
                        if (nd > maxd) maxd = nd;
                    }
                    continue;
                }
                const int64_t nd = d + cs;
                bool ok = false;
                if (act) { const int64_t dn = dg[nxt]; ok = dn == -1 || dn > nd; if (ok) { dg[nxt] = nd; pg[nxt] = cur; } }
                wave_fence();
                const int bk = (int)(nd % nb);
                for (int bb = 0; bb < nb && !over; bb++) push_lanes(bb, ok && bk == bb, nxt);
                int64_t mx = ok ? nd : 0;
                for (int o = AASM_WAVE / 2; o >= 1; o >>= 1) { const int64_t y = wave_shfl_xor(mx, o); mx = y > mx ? y : mx; }
                if (mx > maxd) maxd = mx;
            }
        }
    }
    if (over && lane == 0) pg[s0] = -2;                              // reported by the host driver
}

// ---- host side: argument checks and the drivers, shared by the product (aasm_gpu.hip) and the host emulation -----------
}  // namespace aasm
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>
namespace aasm {

// A failed check or driver run: code rc, and *why = msg (kept until this thread's next failure).
static inline int check_fail(const char **why, int rc, const std::string &msg) {
    static thread_local std::string last;
    last = msg;
    *why = last.c_str();
    return rc;
}

// The common layout of a graph batch.  Returns AASM_OK, or AASM_E_INVAL with a message in *why.  The offsets are checked first
// (g_voff from 0 and strictly increasing, then rowptr from 0 and non-decreasing), and only then is anything read through them.
// more: the entry's other pointers, which must not be NULL either.  has_src = false: an entry without sources (aasm_topology_sort);
// src is then neither required nor read.  n_vertices / n_edges >= 0: the arrays' lengths as the caller of a resident batch states them
// (aasm_graphs.h), which the offsets must end at; each is asked before anything is read through the offsets it closes.
static inline int check_graph_batch(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int32_t *src,
                                    std::initializer_list<const void *> more, const char **why, bool has_src = true, int64_t n_vertices = -1,
                                    int64_t n_edges = -1) {
    bool null = !g_voff || !rowptr || !col || (has_src && !src);
    for (const void *p : more) null |= !p;
    if (n_graphs <= 0 || null) return check_fail(why, AASM_E_INVAL, "empty batch or NULL pointer");
    if (g_voff[0] != 0) return check_fail(why, AASM_E_INVAL, "graph offsets do not start at 0");
    for (int64_t g = 0; g < n_graphs; g++)
        if (g_voff[g + 1] <= g_voff[g]) return check_fail(why, AASM_E_INVAL, "graph " + std::to_string(g) + ": empty, or graph offsets not increasing");
    const int64_t VT = g_voff[n_graphs];
    if (n_vertices >= 0 && VT != n_vertices) return check_fail(why, AASM_E_INVAL, "graph offsets do not end at n_vertices");
    if (rowptr[0] != 0) return check_fail(why, AASM_E_INVAL, "row pointers do not start at 0");
    for (int64_t v = 0; v < VT; v++)
        if (rowptr[v + 1] < rowptr[v]) return check_fail(why, AASM_E_INVAL, "row pointers decrease at vertex " + std::to_string(v));
    if (n_edges >= 0 && rowptr[VT] != n_edges) return check_fail(why, AASM_E_INVAL, "row pointers do not end at n_edges");
    for (int64_t g = 0; g < n_graphs; g++) {
        const int64_t v0 = g_voff[g], v1 = g_voff[g + 1];
        if (has_src && (src[g] < 0 || src[g] >= v1 - v0)) return check_fail(why, AASM_E_INVAL, "graph " + std::to_string(g) + ": source outside it");
        for (int64_t e = rowptr[v0]; e < rowptr[v1]; e++)
            if (col[e] < 0 || col[e] >= v1 - v0) return check_fail(why, AASM_E_INVAL, "graph " + std::to_string(g) + ": edge head outside the graph");
    }
    return AASM_OK;
}

// a distance as the C-ABI's five int64 {qry, ref, anom, qnz, qtot}
static inline void put_d5(int64_t *o, const Dist &x) { o[0] = x.qry; o[1] = x.ref; o[2] = x.anom; o[3] = x.qnz; o[4] = x.qtot; }

// The w5 weight domain of dijkstra and k-walks; with `negative` (bellman_ford, AASM_KSW_NEGATIVE) without the clause on the score
// sum's sign.  AASM_OK, or AASM_E_OVERFLOW.
static inline int w5_fail(int64_t e, bool negative, const char **why) {
    return check_fail(why, AASM_E_OVERFLOW, "edge " + std::to_string(e) + ": weight outside the supported range (" + (negative ? "" : "score sum >= 0, ") + "|scores| < 2^39, anom 0..2, mapq counts 0..1)");
}
static inline int check_w5(const int64_t *w5, int64_t n_edges, bool negative, const char **why) {
    const int64_t lim = (int64_t)1 << 39;
    for (int64_t e = 0; e < n_edges; e++) {
        const int64_t *w = w5 + 5 * e;
        if (w[0] < -lim || w[0] >= lim || w[1] < -lim || w[1] >= lim || (!negative && w[0] + w[1] < 0) || w[2] < 0 || w[2] > 2 || w[3] < 0 || w[3] > 1 || w[4] < 0 || w[4] > 1)
            return w5_fail(e, negative, why);
    }
    return AASM_OK;
}

// The entries' argument checks (shared by the product and the host emulation): AASM_OK, or the code with a message in why.
static inline int dijkstra_check_args(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5,
                                      const int32_t *src, const int64_t *d5, const int32_t *prev, const char **why) {
    const int rc = check_graph_batch(n_graphs, g_voff, rowptr, col, src, {w5, d5, prev}, why);
    return rc != AASM_OK ? rc : check_w5(w5, rowptr[g_voff[n_graphs]], false, why);
}
static inline int bellman_ford_check_args(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5,
                                          const int32_t *src, const int64_t *d5, const int32_t *prev, const int32_t *status, const int64_t *cycle_off,
                                          const int32_t *cycle, const char **why) {
    const int rc = check_graph_batch(n_graphs, g_voff, rowptr, col, src, {w5, d5, prev, status, cycle_off, cycle}, why);
    return rc != AASM_OK ? rc : check_w5(w5, rowptr[g_voff[n_graphs]], true, why);
}
// aasm_sssp_dag (w5, src, d5, prev given; order may be NULL) and aasm_topology_sort (sort_only: none of the four, order required).
// A graph's in-degrees and edge positions are int32: fewer than 2^31 edges per graph; the relaxation sums up to V - 1 weights of
// |w| < 2^39 in int64: at most 2^20 vertices per graph (AASM_KSW_MAX_V, aasm_ksw.h, for the same reason).
#define AASM_DAG_MAX_V ((int64_t)1 << 20)
static inline int dag_check_args(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5,
                                 const int32_t *src, const int64_t *d5, const int32_t *prev, const int32_t *order, const int32_t *status,
                                 bool sort_only, const char **why) {
    const int rc = sort_only ? check_graph_batch(n_graphs, g_voff, rowptr, col, nullptr, {order, status}, why, false)
                             : check_graph_batch(n_graphs, g_voff, rowptr, col, src, {w5, d5, prev, status}, why);
    if (rc != AASM_OK) return rc;
    for (int64_t g = 0; g < n_graphs; g++) {
        const int64_t V = g_voff[g + 1] - g_voff[g], E = rowptr[g_voff[g + 1]] - rowptr[g_voff[g]];
        if (!sort_only && V > AASM_DAG_MAX_V) return check_fail(why, AASM_E_OVERFLOW, "graph " + std::to_string(g) + ": more than 2^20 vertices");
        if (V > INT32_MAX || E > INT32_MAX) return check_fail(why, AASM_E_OVERFLOW, "graph " + std::to_string(g) + ": 2^31 vertices or edges, or more");
    }
    return sort_only ? AASM_OK : check_w5(w5, rowptr[g_voff[n_graphs]], true, why);
}
// Dial's lim and the cost range
static inline int dial_lim_fail(const char **why) { return check_fail(why, AASM_E_INVAL, "lim outside 0 .. 7"); }
static inline int dial_cost_fail(int64_t e, const char **why) {
    return check_fail(why, AASM_E_INVAL, "edge " + std::to_string(e) + ": cost outside 0 .. lim (the reference asserts it, k_weighted_bfs.hpp:27)");
}
static inline int check_dial_costs(const int32_t *cost, int64_t n_edges, int lim, const char **why) {
    if (lim < 0 || lim >= DIAL_MAXB) return dial_lim_fail(why);
    for (int64_t e = 0; e < n_edges; e++)
        if (cost[e] < 0 || cost[e] > lim) return dial_cost_fail(e, why);
    return AASM_OK;
}
static inline int dial_check_args(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int32_t *cost,
                                  const int32_t *src, int lim, const int64_t *dist, const int64_t *pre, const char **why) {
    const int rc = check_graph_batch(n_graphs, g_voff, rowptr, col, src, {cost, dist, pre}, why);
    return rc != AASM_OK ? rc : check_dial_costs(cost, rowptr[g_voff[n_graphs]], lim, why);
}

// Device memory of one driver run through backend BE: after the first failure `ok` stays false and every later call returns
// nullptr, so a driver allocates everything and tests once.
template <class BE> struct DevMem {
    BE &be;
    bool ok = true;
    void *alloc(size_t bytes) {
        if (!ok) return nullptr;
        void *p = be.alloc(bytes ? bytes : 16);
        if (!p) ok = false;
        return p;
    }
    void *up(const void *h, size_t bytes) {
        void *p = alloc(bytes);
        if (ok && bytes && !be.h2d(p, h, bytes)) ok = false;
        return p;
    }
};

// The SSSP kernels, one 64-lane workgroup per graph (row shapes: aasm_dev.h); body(k, a).  Dial's keeps its buckets in LDS, with no
// register budget.
#define AASM_SSSP_KERNELS(K, KL)                                     \
    K(SSSP_K_DIJKSTRA, aasm_sssp_dijkstra_kernel, 64, 1, kb_sssp_dijkstra) \
    KL(SSSP_K_DIAL, aasm_sssp_dial_kernel, 64, 1, sizeof(DialLds), 0, kb_sssp_dial) \
    K(SSSP_K_BELLMAN_FORD, aasm_sssp_bellman_ford_kernel, 64, 1, kb_sssp_bellman_ford) \
    K(SSSP_K_DAG, aasm_sssp_dag_kernel, 64, 1, kb_sssp_dag)
enum { AASM_SSSP_KERNELS(AASM_ROW_ID, AASM_ROW_ID) };
constexpr int sssp_block[] = {AASM_SSSP_KERNELS(AASM_ROW_BLOCK, AASM_ROW_BLOCK)};
AASM_KERNEL_BODY(run_sssp_body, AASM_SSSP_KERNELS, SsspArgs)

// Backend BE: ksw_run's contract (aasm_ksw.h), with bool launch(kernel, n_graphs, SsspArgs) for the SSSP kernels (one block
// per graph of the whole batch).  why: the message of a failure the driver itself finds.
template <class BE>
int dijkstra_run(BE &be, int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5,
                 const int32_t *src, int64_t *d5, int32_t *prev, const char **why) {
    const int64_t G = n_graphs, VT = g_voff[G], ET = rowptr[VT];
    DevMem<BE> m{be};
    SsspArgs a;
    memset(&a, 0, sizeof(a));
    a.n_graphs = G;
    a.voff = (const int64_t *)m.up(g_voff, (size_t)(G + 1) * 8);
    a.rowptr = (const int64_t *)m.up(rowptr, (size_t)(VT + 1) * 8);
    a.col = (const int32_t *)m.up(col, (size_t)ET * 4);
    a.src = (const int32_t *)m.up(src, (size_t)G * 4);
    a.w5 = (const int64_t *)m.up(w5, (size_t)ET * 40);
    a.d = (Dist *)m.alloc((size_t)VT * sizeof(Dist));
    a.prv = (int32_t *)m.alloc((size_t)VT * 4);
    if (!m.ok) return be.err();
    std::vector<Dist> hd((size_t)VT);
    // Heap capacity.  With a monotone order every successful relaxation pushes once (<= E + 1 entries), but CALC_SUM's third
    // key (the mapq ratio) is not monotone under addition and the reference re-expands a vertex whenever its distance
    // improves, so stale entries of one edge can pile up: a graph whose heap overflows is run again with 4x, 16x, 64x the room.
    int64_t overflowed = -1;
    for (int64_t mult = 1; mult <= 64; mult *= 4) {
        std::vector<int64_t> ho((size_t)G + 1, 0);
        for (int64_t g = 0; g < G; g++) ho[(size_t)g + 1] = ho[(size_t)g] + mult * (rowptr[g_voff[g + 1]] - rowptr[g_voff[g]] + 2);
        const size_t mark = be.mark();
        a.hoff = (const int64_t *)m.up(ho.data(), (size_t)(G + 1) * 8);
        a.heap = (DjEnt *)m.alloc((size_t)ho[(size_t)G] * sizeof(DjEnt));
        if (!m.ok || !be.launch(SSSP_K_DIJKSTRA, G, a) || !be.sync() || !be.d2h(hd.data(), a.d, (size_t)VT * sizeof(Dist)) ||
            !be.d2h(prev, a.prv, (size_t)VT * 4)) return be.err();
        be.release(mark);
        overflowed = -1;
        for (int64_t g = 0; g < G; g++) if (prev[g_voff[g] + src[g]] == -2) { overflowed = g; break; }
        if (overflowed < 0) break;
    }
    if (overflowed >= 0) return check_fail(why, AASM_E_OVERFLOW, "graph " + std::to_string(overflowed) + ": dijkstra heap capacity exceeded at 64 x (E + 2) entries");
    for (int64_t v = 0; v < VT; v++) put_d5(d5 + 5 * v, hd[(size_t)v]);
    return AASM_OK;
}

// graph g's queue ring of bellman_ford: 2 * (E + 2) entries (the bound: bf_spfa's comment), as offsets into one allocation
static inline std::vector<int64_t> bf_queue_offsets(int64_t G, const int64_t *g_voff, const int64_t *rowptr) {
    std::vector<int64_t> qo((size_t)G + 1, 0);
    for (int64_t g = 0; g < G; g++) qo[(size_t)g + 1] = qo[(size_t)g] + 2 * (rowptr[g_voff[g + 1]] - rowptr[g_voff[g]] + 2);
    return qo;
}

// status[g]: 0 with d5 / prev the reference's vectors; 1 for a negative cycle, cycle[cycle_off[g] .. cycle_off[g + 1]) holding it and
// d5 / prev max / -1; a negative AASM_E_* otherwise.  A graph's status never fails the call.  qhigh: nullptr, or G cells for the
// queues' high-water marks (the emulation's debug return).
template <class BE>
int bellman_ford_run(BE &be, int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5,
                     const int32_t *src, int64_t *d5, int32_t *prev, int32_t *status, int64_t *cycle_off, int32_t *cycle, int64_t *qhigh,
                     const char **why) {
    (void)why;
    const int64_t G = n_graphs, VT = g_voff[G], ET = rowptr[VT];
    const std::vector<int64_t> qo = bf_queue_offsets(G, g_voff, rowptr);
    DevMem<BE> m{be};
    SsspArgs a;
    memset(&a, 0, sizeof(a));
    a.n_graphs = G;
    a.voff = (const int64_t *)m.up(g_voff, (size_t)(G + 1) * 8);
    a.rowptr = (const int64_t *)m.up(rowptr, (size_t)(VT + 1) * 8);
    a.col = (const int32_t *)m.up(col, (size_t)ET * 4);
    a.src = (const int32_t *)m.up(src, (size_t)G * 4);
    a.w5 = (const int64_t *)m.up(w5, (size_t)ET * 40);
    a.hoff = (const int64_t *)m.up(qo.data(), (size_t)(G + 1) * 8);
    a.d = (Dist *)m.alloc((size_t)VT * sizeof(Dist));
    a.prv = (int32_t *)m.alloc((size_t)VT * 4);
    a.mark = (int32_t *)m.alloc((size_t)VT * 4);
    a.heap = (DjEnt *)m.alloc((size_t)qo[(size_t)G] * sizeof(DjEnt));
    a.status = (int32_t *)m.alloc((size_t)G * 4);
    a.clen = (int64_t *)m.alloc((size_t)G * 8);
    a.qhigh = (int64_t *)m.alloc((size_t)G * 8);
    a.cyc = (int32_t *)m.alloc((size_t)(VT + G) * 4);
    if (!m.ok) return be.err();
    std::vector<Dist> hd((size_t)VT);
    std::vector<int64_t> clen((size_t)G);
    if (!be.launch(SSSP_K_BELLMAN_FORD, G, a) || !be.sync() || !be.d2h(hd.data(), a.d, (size_t)VT * sizeof(Dist)) ||
        !be.d2h(prev, a.prv, (size_t)VT * 4) || !be.d2h(status, a.status, (size_t)G * 4) || !be.d2h(clen.data(), a.clen, (size_t)G * 8) ||
        (qhigh && !be.d2h(qhigh, a.qhigh, (size_t)G * 8))) return be.err();
    for (int64_t v = 0; v < VT; v++) put_d5(d5 + 5 * v, hd[(size_t)v]);
    cycle_off[0] = 0;
    for (int64_t g = 0; g < G; g++) {
        const int64_t len = clen[(size_t)g] < 0 || clen[(size_t)g] > g_voff[g + 1] - g_voff[g] + 1 ? 0 : clen[(size_t)g];
        if (len && !be.d2h(cycle + cycle_off[g], a.cyc + g_voff[g] + g, (size_t)len * 4)) return be.err();
        cycle_off[g + 1] = cycle_off[g] + len;
    }
    return AASM_OK;
}

// topology_sort() and shortest_path_dag() of every graph in one launch.  status[g]: 0 with order / d5 / prev the reference's vectors;
// 1 for a cycle, with order -1, d5 max() but IDENTITY at src, prev -1.  w5 == nullptr: the sort alone (src, d5, prev unused).
// order == nullptr: not wanted.  A graph's status never fails the call.
template <class BE>
int dag_run(BE &be, int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5,
            const int32_t *src, int64_t *d5, int32_t *prev, int32_t *order, int32_t *status, const char **why) {
    (void)why;
    const int64_t G = n_graphs, VT = g_voff[G], ET = rowptr[VT];
    DevMem<BE> m{be};
    SsspArgs a;
    memset(&a, 0, sizeof(a));
    a.n_graphs = G;
    a.voff = (const int64_t *)m.up(g_voff, (size_t)(G + 1) * 8);
    a.rowptr = (const int64_t *)m.up(rowptr, (size_t)(VT + 1) * 8);
    a.col = (const int32_t *)m.up(col, (size_t)ET * 4);
    a.mark = (int32_t *)m.alloc((size_t)VT * 4);
    a.order = (int32_t *)m.alloc((size_t)VT * 4);
    a.status = (int32_t *)m.alloc((size_t)G * 4);
    if (w5) {
        a.src = (const int32_t *)m.up(src, (size_t)G * 4);
        a.w5 = (const int64_t *)m.up(w5, (size_t)ET * 40);
        a.d = (Dist *)m.alloc((size_t)VT * sizeof(Dist));
        a.prv = (int32_t *)m.alloc((size_t)VT * 4);
        a.claim = (int32_t *)m.alloc((size_t)VT * 4);
    }
    if (!m.ok || !be.launch(SSSP_K_DAG, G, a) || !be.sync() || !be.d2h(status, a.status, (size_t)G * 4) ||
        (order && !be.d2h(order, a.order, (size_t)VT * 4))) return be.err();
    if (w5) {
        std::vector<Dist> hd((size_t)VT);
        if (!be.d2h(hd.data(), a.d, (size_t)VT * sizeof(Dist)) || !be.d2h(prev, a.prv, (size_t)VT * 4)) return be.err();
        for (int64_t v = 0; v < VT; v++) put_d5(d5 + 5 * v, hd[(size_t)v]);
    }
    return AASM_OK;
}

template <class BE>
int dial_run(BE &be, int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int32_t *cost,
             const int32_t *src, int lim, int64_t *dist, int64_t *pre, const char **why) {
    const int64_t G = n_graphs, VT = g_voff[G], ET = rowptr[VT];
    const int nb = lim + 1;
    std::vector<int64_t> soff((size_t)G + 1, 0);
    for (int64_t g = 0; g < G; g++) {
        // a vertex is pushed once per successful relaxation: its distance falls by at least one each time and by at most lim in all
        // after the first (a later pop has d' >= d), so <= lim + 1 pushes per vertex - and never more than one per edge, plus the source
        const int64_t v0 = g_voff[g], v1 = g_voff[g + 1];
        const int64_t E = rowptr[v1] - rowptr[v0], by_v = (v1 - v0) * (int64_t)nb;
        const int64_t per = ((E + 1 < by_v ? E + 1 : by_v) + DIAL_WIN + 63) / 64 * 64;
        soff[(size_t)g + 1] = soff[(size_t)g] + per * nb;
    }
    DevMem<BE> m{be};
    SsspArgs a;
    memset(&a, 0, sizeof(a));
    a.n_graphs = G; a.nb = nb;
    a.voff = (const int64_t *)m.up(g_voff, (size_t)(G + 1) * 8);
    a.rowptr = (const int64_t *)m.up(rowptr, (size_t)(VT + 1) * 8);
    a.col = (const int32_t *)m.up(col, (size_t)ET * 4);
    a.cost = (const int32_t *)m.up(cost, (size_t)ET * 4);
    a.src = (const int32_t *)m.up(src, (size_t)G * 4);
    a.soff = (const int64_t *)m.up(soff.data(), (size_t)(G + 1) * 8);
    a.dist = (int64_t *)m.alloc((size_t)VT * 8);
    a.pre = (int64_t *)m.alloc((size_t)VT * 8);
    a.spill = (int32_t *)m.alloc((size_t)soff[(size_t)G] * 4);
    if (!m.ok || !be.launch(SSSP_K_DIAL, G, a) || !be.sync() || !be.d2h(dist, a.dist, (size_t)VT * 8) || !be.d2h(pre, a.pre, (size_t)VT * 8))
        return be.err();
    for (int64_t g = 0; g < G; g++)
        if (pre[g_voff[g] + src[g]] == -2) return check_fail(why, AASM_E_INTERNAL, "graph " + std::to_string(g) + ": bucket capacity exceeded (must not happen)");
    return AASM_OK;
}

}  // namespace aasm
