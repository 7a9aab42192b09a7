// aasm_graphs.h -- resident graph batches (include/alignasm_amd.h: aasm_graphs_upload / aasm_graphs_wrap_device and the five
// *_device entries): a checked batch that lives on one device, aasm_sssp.h's kernels run over it with device pointers in and out.
// Here: the thread-per-item kernels around those solves (table AASM_GRAPHS_KERNELS, bodies in KCtx style: the layout checks of a
// batch that is already on the device, the per-graph counts, the source check, Dist -> five int64, the one-word reductions, the
// packing of bellman_ford's cycles), the handle, and the drivers, shared by the product (aasm_gpu.hip) and the host emulation
// (tests/host_emul/graphs_resident_emul.cpp).  Also here: k shortest walks on a resident batch (aasm_k_shortest_walks_device /
// aasm_ksw_export_device) - aasm_ksw.h's kernels as they are, the small kernels that size, place and pack around them, and the
// driver pair graphs_ksw / graphs_ksw_export (tests/host_emul/ksw_resident_emul.cpp).
#pragma once
#include "aasm_ksw.h"

namespace aasm {

struct GraphsArgs {
    int64_t n_graphs, n_vertices, n_edges;                           // the lengths the caller stated
    const int64_t *voff, *rowptr; const int32_t *col; const int64_t *w5; const int32_t *cost; int32_t lim, pad;
    const int32_t *src;
    int64_t *words;                                                  // GR_W_*: verdicts, by 64-bit atomic min
    int64_t *gcount;                                                 // [2 * (G + 1)]: voff[g], then rowptr[voff[g]]
    const Dist *d; int64_t *d5;                                      // Dist -> five int64
    const int32_t *prv; const int64_t *pre; int32_t *status;         // the overflow markers of dijkstra (prv) and dial (pre)
    const int64_t *clen; int64_t *cycle_off; const int32_t *cyc; int32_t *cycle;   // bellman_ford's cycles
    // k shortest walks (graphs_ksw): kb_ksw_*'s per-graph counts in, the graphs' shares of arena / queue / results and their scans out
    const int32_t *sink;
    const int64_t *ins, *walks, *nfound, *wtot, *hcount;
    int64_t *acap, *qcap, *aoff, *qoff, *rofs;
    int64_t *hoff; int64_t mult;                                     // a retry round of the cyclic tree: [G + 1] heap offsets at mult x (E + 2)
    int64_t *foff, *wbase;                                           // [G + 1] scan of nfound, [G] scan of wtot
    int64_t *ktot;                                                   // GR_KT_N totals, the words the host reads
    // ... and the export: walk i of graph g is result rofs[g] + i of the solve and walk foff[g] + i of the caller
    const Dist *rdist; const int64_t *woff; int64_t n_walks, n_walk_edges;
    int64_t *o_nfound, *o_foff, *o_dist5, *o_woff, *o_heap; int32_t *o_status;
};
#define GR_KT_N 4
enum { GR_W_VERDICT = 0, GR_W_NEG = 1, GR_W_N = 2 };
// A verdict: (reason << GR_POS_BITS) | position, the smallest one wins - reasons in the order the host checks ask them, positions in
// array order, so the message is the host's ("first in array order").  A word nobody lowered (filled with 0x7f bytes) is a pass.
#define GR_POS_BITS 56
#define GR_PASS ((int64_t)0x7f7f7f7f7f7f7f7fll)
enum { GR_START = 0, GR_ORDER = 1, GR_END = 2 };                     // stages 1 and 2 (position: graph / vertex)
enum { GR_HEAD = 0, GR_W5 = 1, GR_COST = 2 };                        // stage 3 (position: graph for a head, else edge)
#define GR_MAX_BLOCKS 4096                                           // 256-thread blocks: beyond 16 per CU the items are taken grid-stride

AASM_DEV void gr_fail(const GraphsArgs &a, int reason, int64_t pos) { atomic_min_i64(a.words + GR_W_VERDICT, ((int64_t)reason << GR_POS_BITS) | pos); }
#define GR_FOR_ITEMS(i, n) for (int64_t i = k.bid * k.nthreads + k.tid; i < (n); i += k.nblocks * k.nthreads)

// ---- the layout checks of a batch that is already on the device, in three stages -------------------------------------------------
// What keeps a hostile batch from becoming an address: in stages 1 and 2 a thread reads only the cells whose index is its own id and
// id + 1, below a length the caller stated - the pointer check asks of an array its device, its alignment and that it is not NULL, not
// its size: a caller who overstates a length has the kernels read past the array, as with any entry that takes a length -; nothing is
// read THROUGH an offset until the stage that validated that offset has passed - the host reads the verdict between stages and launches
// the next one only after a pass.
// 1. g_voff: from 0, strictly increasing, ends at n_vertices.  A thread per graph.
AASM_DEV void kb_gr_check_voff(const KCtx &k, const GraphsArgs &a) {
    GR_FOR_ITEMS(g, a.n_graphs) {
        const int64_t lo = a.voff[g], hi = a.voff[g + 1];
        if (g == 0 && lo != 0) gr_fail(a, GR_START, 0);
        if (hi <= lo) gr_fail(a, GR_ORDER, g);
        if (g == a.n_graphs - 1 && hi != a.n_vertices) gr_fail(a, GR_END, 0);
    }
}
// 2. rowptr: from 0, non-decreasing, ends at n_edges.  A thread per vertex (n_vertices is g_voff's end: stage 1).
AASM_DEV void kb_gr_check_rowptr(const KCtx &k, const GraphsArgs &a) {
    GR_FOR_ITEMS(v, a.n_vertices) {
        const int64_t lo = a.rowptr[v], hi = a.rowptr[v + 1];
        if (v == 0 && lo != 0) gr_fail(a, GR_START, 0);
        if (hi < lo) gr_fail(a, GR_ORDER, v);
        if (v == a.n_vertices - 1 && hi != a.n_edges) gr_fail(a, GR_END, 0);
    }
}
// the last index i in [0, n) with off[i] <= x; off is non-decreasing with off[0] <= x < off[n] (stages 1 and 2)
AASM_DEV int64_t gr_owner(const int64_t *off, int64_t n, int64_t x) {
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) { const int64_t mid = lo + ((hi - lo) >> 1); if (off[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}
// 3. every edge head inside ITS graph, the w5 clauses (check_w5 with negative = true), the cost range; and the first edge whose score
// sum is negative, for dijkstra.  A thread per edge, so a row of hundreds of edges is hundreds of threads and col / w5 / cost stream
// in coalesced; the edge's vertex and the vertex's graph are found by bisection in the two validated offset arrays (cached: the
// threads of a wave look for neighbouring edges).  Hundreds of tiny graphs cost the same two bisections.
AASM_DEV void kb_gr_check_edges(const KCtx &k, const GraphsArgs &a) {
    const int64_t lim = (int64_t)1 << 39;
    GR_FOR_ITEMS(e, a.n_edges) {
        const int64_t v = gr_owner(a.rowptr, a.n_vertices, e), g = gr_owner(a.voff, a.n_graphs, v);
        const int64_t V = a.voff[g + 1] - a.voff[g];
        const int32_t h = a.col[e];
        if (h < 0 || h >= V) gr_fail(a, GR_HEAD, g);
        bool neg = false;
        if (a.w5) {
            const int64_t *w = a.w5 + 5 * e;
            const int64_t w0 = w[0], w1 = w[1];
            if (w0 < -lim || w0 >= lim || w1 < -lim || w1 >= lim || w[2] < 0 || w[2] > 2 || w[3] < 0 || w[3] > 1 || w[4] < 0 || w[4] > 1) gr_fail(a, GR_W5, e);
            else neg = w0 + w1 < 0;
        }
        if (a.cost) { const int32_t c = a.cost[e]; if (c < 0 || c > a.lim) gr_fail(a, GR_COST, e); }
        // one atomic per wave: its lanes hold consecutive edges, so the lowest lane with a negative sum holds the wave's first
        const uint64_t m = wave_ballot(neg);
        if (neg && (m & lanemask_lt(k.lane)) == 0) atomic_min_i64(a.words + GR_W_NEG, e);
    }
}
// the per-graph vertex and edge counts for the host's sizing, as offsets: voff[g] and rowptr[voff[g]], g = 0 .. G (after stage 2)
AASM_DEV void kb_gr_counts(const KCtx &k, const GraphsArgs &a) {
    GR_FOR_ITEMS(g, a.n_graphs + 1) { const int64_t v = a.voff[g]; a.gcount[g] = v; a.gcount[a.n_graphs + 1 + g] = a.rowptr[v]; }
}

// ---- per call ------------------------------------------------------------------------------------------------------------------------
// the first graph with a source outside it
AASM_DEV void kb_gr_check_src(const KCtx &k, const GraphsArgs &a) {
    GR_FOR_ITEMS(g, a.n_graphs) { const int32_t s = a.src[g]; if (s < 0 || s >= a.voff[g + 1] - a.voff[g]) atomic_min_i64(a.words + GR_W_VERDICT, g); }
}
// Dist -> {qry, ref, anom, qnz, qtot} as int64: a thread per OUTPUT word, so the stores of a wave are 512 contiguous bytes; the loads
// are one word of a 32-byte Dist each, five threads per Dist
AASM_DEV void kb_gr_d5(const KCtx &k, const GraphsArgs &a) {
    GR_FOR_ITEMS(i, 5 * a.n_vertices) {
        const int64_t v = i / 5;
        const int c = (int)(i - 5 * v);
        const Dist &x = a.d[v];
        a.d5[i] = c == 0 ? x.qry : c == 1 ? x.ref : c == 2 ? (int64_t)x.anom : c == 3 ? (int64_t)x.qnz : (int64_t)x.qtot;
    }
}
// dijkstra's "some graph ran out of heap room" (kb_sssp_dijkstra leaves prv[src] = -2) as one word: the first such graph
AASM_DEV void kb_gr_dj_over(const KCtx &k, const GraphsArgs &a) {
    GR_FOR_ITEMS(g, a.n_graphs) if (a.prv[a.voff[g] + a.src[g]] == -2) atomic_min_i64(a.words + GR_W_VERDICT, g);
}
// dial's bucket-overflow marker (pre[src] = -2) as the graph's status
AASM_DEV void kb_gr_dial_status(const KCtx &k, const GraphsArgs &a) {
    GR_FOR_ITEMS(g, a.n_graphs) a.status[g] = a.pre[a.voff[g] + a.src[g]] == -2 ? AASM_E_INTERNAL : 0;
}
// bellman_ford's cycles: the length the host driver would take (0 for a count outside 0 .. V + 1)
AASM_DEV int64_t gr_cycle_len(const GraphsArgs &a, int64_t g) {
    const int64_t c = a.clen[g];
    return c < 0 || c > a.voff[g + 1] - a.voff[g] + 1 ? 0 : c;
}
// cycle_off = the exclusive scan of the lengths over the graphs: ONE wave, 64 graphs per step with a running carry (the batch's
// graphs, not its vertices: a few thousand words at most beside a solve that took a workgroup per graph)
AASM_DEV void kb_gr_cycle_scan(const KCtx &k, const GraphsArgs &a) {
    if (k.bid != 0) return;
    int64_t carry = 0;
    for (int64_t g0 = 0; g0 < a.n_graphs; g0 += AASM_WAVE) {
        const int64_t g = g0 + k.lane;
        const int64_t len = g < a.n_graphs ? gr_cycle_len(a, g) : 0;
        const int64_t incl = wave_incl_add(len);
        if (g < a.n_graphs) a.cycle_off[g] = carry + incl - len;
        carry += wave_bcast(incl, AASM_WAVE - 1);
    }
    if (k.lane == 0) a.cycle_off[a.n_graphs] = carry;
}
// ... and the copy from cyc[voff[g] + g ...] to the packed list, a workgroup per graph
AASM_DEV void kb_gr_cycle_copy(const KCtx &k, const GraphsArgs &a) {
    const int64_t g = k.bid;
    if (g >= a.n_graphs) return;
    const int64_t len = gr_cycle_len(a, g), from = a.voff[g] + g, to = a.cycle_off[g];
    for (int64_t i = k.tid; i < len; i += k.nthreads) a.cycle[to + i] = a.cyc[from + i];
}

// ---- k shortest walks on a resident batch: the kernels around aasm_ksw.h's ---------------------------------------------------------------
// the first graph with a source or a sink outside it: verdict 2 * g for the source, 2 * g + 1 for the sink (ksw_check_args' order as
// the entry states it: the lowest graph, its source before its sink)
AASM_DEV void kb_gr_ksw_check(const KCtx &k, const GraphsArgs &a) {
    GR_FOR_ITEMS(g, a.n_graphs) {
        const int64_t V = a.voff[g + 1] - a.voff[g];
        const int32_t s = a.src[g], t = a.sink[g];
        if (s < 0 || s >= V) atomic_min_i64(a.words + GR_W_VERDICT, 2 * g);
        if (t < 0 || t >= V) atomic_min_i64(a.words + GR_W_VERDICT, 2 * g + 1);
    }
}
// N exclusive scans over the graphs at once, by ONE wave as kb_gr_cycle_scan: a TILE of AASM_WAVE = 64 graphs per step, a graph per
// lane, running carries between the steps - right for any G, G / 64 steps long (a few thousand graphs beside solves that took a
// workgroup each).  val(g, x): graph g's N terms; put(g, x, ex): its terms and the sums before it; tot: the N totals.
template <int N, class Val, class Put> AASM_DEV void gr_wave_scans(const KCtx &k, int64_t G, Val val, Put put, int64_t *tot) {
    int64_t carry[N];
    AASM_UNROLL
    for (int j = 0; j < N; j++) carry[j] = 0;
    for (int64_t g0 = 0; g0 < G; g0 += AASM_WAVE) {
        const int64_t g = g0 + k.lane;
        int64_t x[N], ex[N];
        AASM_UNROLL
        for (int j = 0; j < N; j++) x[j] = 0;
        if (g < G) val(g, x);
        AASM_UNROLL
        for (int j = 0; j < N; j++) {
            const int64_t incl = wave_incl_add(x[j]);
            ex[j] = carry[j] + incl - x[j];
            carry[j] += wave_bcast(incl, AASM_WAVE - 1);
        }
        if (g < G) put(g, x, ex);
    }
    AASM_UNROLL
    for (int j = 0; j < N; j++) tot[j] = carry[j];
}
// After the tree stage: ksw_run's bounds from the device's counts - an insert copies at most the right spine of a version of <= ins
// keys (<= floor(log2(ins + 1)) + 1 nodes) and adds a leaf: ins * (floor(log2(ins + 1)) + 2) nodes, capped at INT32_MAX; a pop
// emplaces at most three queue entries: 3 * walks - 2; nothing for a graph with a status or without a walk - and the scans that place
// every graph's share: aoff (arena), qoff (queue), rofs (results, walks[g] each).  ktot[0 .. 2]: the three totals.
AASM_DEV void kb_gr_ksw_bounds(const KCtx &k, const GraphsArgs &a) {
    if (k.bid != 0 || k.tid >= AASM_WAVE) return;
    int64_t tot[3];
    gr_wave_scans<3>(k, a.n_graphs,
        [&](int64_t g, int64_t *x) {
            const int64_t in = a.ins[g] < 0 ? 0 : a.ins[g], w = a.walks[g];
            int64_t lg = 0;
            while (lg < 40 && ((int64_t)1 << (lg + 1)) <= in + 1) lg++;      // (ins <= E < 2^31)
            const int64_t bound = in * (lg + 2);
            const bool live = a.status[g] == 0 && w > 0;
            x[0] = live ? (bound < INT32_MAX ? bound : INT32_MAX) : 0;
            x[1] = live ? 3 * w - 2 : 0;
            x[2] = w;
        },
        [&](int64_t g, const int64_t *x, const int64_t *ex) {
            a.acap[g] = x[0]; a.qcap[g] = x[1];
            a.aoff[g] = ex[0]; a.qoff[g] = ex[1]; a.rofs[g] = ex[2];
        }, tot);
    if (k.lane == 0) { a.ktot[0] = tot[0]; a.ktot[1] = tot[1]; a.ktot[2] = tot[2]; }
}
// Between two rounds of kb_ksw_tree_cyc: the graphs that ran out of heap room (status AASM_E_OVERFLOW with ins = -1) get
// mult * (E + 2) entries in the next round, the others none (the kernel leaves a graph without room as it is).  ktot[0]: the room
// of the round together, 0 when no graph runs again - the one word the host reads.
AASM_DEV void kb_gr_ksw_retry(const KCtx &k, const GraphsArgs &a) {
    if (k.bid != 0 || k.tid >= AASM_WAVE) return;
    int64_t tot[1];
    gr_wave_scans<1>(k, a.n_graphs,
        [&](int64_t g, int64_t *x) {
            const bool todo = a.status[g] == AASM_E_OVERFLOW && a.ins[g] < 0;
            x[0] = todo ? a.mult * (a.rowptr[a.voff[g + 1]] - a.rowptr[a.voff[g]] + 2) : 0;
        },
        [&](int64_t g, const int64_t *, const int64_t *ex) { a.hoff[g] = ex[0]; }, tot);
    if (k.lane == 0) { a.hoff[a.n_graphs] = tot[0]; a.ktot[0] = tot[0]; }
}
// After the enumeration (and kb_ksw_count where walks are asked for: wtot, else nullptr): foff, the scan of n_found that packs the
// result, and wbase, the scan of the graphs' walk edges.  ktot[0 .. 1]: n_walks, n_walk_edges.
AASM_DEV void kb_gr_ksw_totals(const KCtx &k, const GraphsArgs &a) {
    if (k.bid != 0 || k.tid >= AASM_WAVE) return;
    int64_t tot[2];
    gr_wave_scans<2>(k, a.n_graphs,
        [&](int64_t g, int64_t *x) { x[0] = a.nfound[g]; x[1] = a.wtot ? a.wtot[g] : 0; },
        [&](int64_t g, const int64_t *, const int64_t *ex) { a.foff[g] = ex[0]; a.wbase[g] = ex[1]; }, tot);
    if (k.lane == 0) { a.foff[a.n_graphs] = tot[0]; a.ktot[0] = tot[0]; a.ktot[1] = tot[1]; }
}
// the export, a thread per output word: the per-graph arrays ...
AASM_DEV void kb_gr_ksw_pack_graphs(const KCtx &k, const GraphsArgs &a) {
    GR_FOR_ITEMS(g, a.n_graphs + 1) {
        a.o_foff[g] = a.foff[g];
        if (g < a.n_graphs) { a.o_nfound[g] = a.nfound[g]; a.o_heap[g] = a.hcount[g]; a.o_status[g] = a.status[g]; }
    }
}
// ... the walks' distances, packed by n_found (kb_gr_d5's form: five threads per Dist, the stores of a wave contiguous; the walk's
// graph by bisection in foff, where a graph without walks owns nothing) ...
AASM_DEV void kb_gr_ksw_pack_dist(const KCtx &k, const GraphsArgs &a) {
    GR_FOR_ITEMS(i, 5 * a.n_walks) {
        const int64_t w = i / 5, g = gr_owner(a.foff, a.n_graphs, w);
        const int c = (int)(i - 5 * w);
        const Dist &x = a.rdist[a.rofs[g] + (w - a.foff[g])];
        a.o_dist5[i] = c == 0 ? x.qry : c == 1 ? x.ref : c == 2 ? (int64_t)x.anom : c == 3 ? (int64_t)x.qnz : (int64_t)x.qtot;
    }
}
// ... and the walks' offsets into walk_edges, [n_walks + 1] (a graph whose walks were capped has wtot = 0 and woff = 0: empty ranges)
AASM_DEV void kb_gr_ksw_pack_woff(const KCtx &k, const GraphsArgs &a) {
    GR_FOR_ITEMS(w, a.n_walks + 1) {
        if (w == a.n_walks) { a.o_woff[w] = a.n_walk_edges; continue; }
        const int64_t g = gr_owner(a.foff, a.n_graphs, w);
        a.o_woff[w] = a.wbase[g] + a.woff[a.rofs[g] + (w - a.foff[g])];
    }
}

#define AASM_GRAPHS_KERNELS(K, ...)                                  \
    K(GR_K_CHECK_VOFF, aasm_graphs_check_voff, 256, ALL_LANES, kb_gr_check_voff) \
    K(GR_K_CHECK_ROWPTR, aasm_graphs_check_rowptr, 256, ALL_LANES, kb_gr_check_rowptr) \
    K(GR_K_CHECK_EDGES, aasm_graphs_check_edges, 256, ALL_LANES, kb_gr_check_edges) \
    K(GR_K_COUNTS, aasm_graphs_counts, 256, ALL_LANES, kb_gr_counts) \
    K(GR_K_CHECK_SRC, aasm_graphs_check_src, 256, ALL_LANES, kb_gr_check_src) \
    K(GR_K_D5, aasm_graphs_d5, 256, ALL_LANES, kb_gr_d5) \
    K(GR_K_DJ_OVER, aasm_graphs_dijkstra_over, 256, ALL_LANES, kb_gr_dj_over) \
    K(GR_K_DIAL_STATUS, aasm_graphs_dial_status, 256, ALL_LANES, kb_gr_dial_status) \
    K(GR_K_CYCLE_SCAN, aasm_graphs_cycle_scan, 64, 1, kb_gr_cycle_scan) \
    K(GR_K_CYCLE_COPY, aasm_graphs_cycle_copy, 64, ALL_LANES, kb_gr_cycle_copy) \
    K(GR_K_KSW_CHECK, aasm_graphs_ksw_check, 256, ALL_LANES, kb_gr_ksw_check) \
    K(GR_K_KSW_BOUNDS, aasm_graphs_ksw_bounds, 64, 1, kb_gr_ksw_bounds) \
    K(GR_K_KSW_RETRY, aasm_graphs_ksw_retry, 64, 1, kb_gr_ksw_retry) \
    K(GR_K_KSW_TOTALS, aasm_graphs_ksw_totals, 64, 1, kb_gr_ksw_totals) \
    K(GR_K_KSW_PACK_GRAPHS, aasm_graphs_ksw_pack_graphs, 256, ALL_LANES, kb_gr_ksw_pack_graphs) \
    K(GR_K_KSW_PACK_DIST, aasm_graphs_ksw_pack_dist, 256, ALL_LANES, kb_gr_ksw_pack_dist) \
    K(GR_K_KSW_PACK_WOFF, aasm_graphs_ksw_pack_woff, 256, ALL_LANES, kb_gr_ksw_pack_woff)
enum { AASM_GRAPHS_KERNELS(AASM_ROW_ID, AASM_ROW_ID) };
constexpr int graphs_block[] = {AASM_GRAPHS_KERNELS(AASM_ROW_BLOCK, AASM_ROW_BLOCK)};
AASM_KERNEL_BODY(run_graphs_body, AASM_GRAPHS_KERNELS, GraphsArgs)

// ---- host side: the handle and the drivers -----------------------------------------------------------------------------------------
// Backend BE (a fresh one per call: the device, the call's stream):
//   void *alloc(size_t) / void free_dev(void *)   device memory that outlives the backend (nullptr: out of memory)
//   bool h2d(d, h, n), bool fill(d, byte, n)      enqueued;  bool read(h, d, n)  enqueued, then waits for the stream;  bool sync()
//   void poison(d, n)                             aasm_debug_poison's fill of working memory about to be used
//   void quiesce()                                waits for the handle's work in flight (before working memory is replaced)
//   bool dev_ok(p, n, align)                      a non-empty array is memory of the device, aligned
//   bool launch_gr(kernel, n_blocks, GraphsArgs), bool launch(kernel, n_graphs, SsspArgs);  int err()
struct GraphsCore {
    aasm_graphs_in view;                                             // device pointers
    std::vector<void *> own;                                         // what the handle frees: an upload's arrays, the words, the offsets
    std::vector<int64_t> gv, ge;                                     // [G + 1] on the host: voff[g], rowptr[voff[g]]
    int64_t first_neg = -1, max_v = 0, max_e = 0;                    // first edge with a negative score sum; the largest graph
    int64_t *words = nullptr;                                        // GR_W_N verdict words
    std::vector<int64_t> ho[4], qo, so;                              // dijkstra's heap offsets at 1x .. 64x, bellman_ford's queues, dial's spill
    int64_t *d_ho[4] = {nullptr, nullptr, nullptr, nullptr}, *d_qo = nullptr, *d_so = nullptr;
    char *work = nullptr; size_t work_cap = 0;                       // working memory: grown on demand, kept between calls
    // the latest k-walk solve, which lives in the working memory until the next call takes it: what graphs_ksw_export packs
    struct { bool valid = false; int64_t serial = 0; aasm_ksw_sizes sz; KswArgs a; int64_t *foff; } ksw;
};
static const char *const GR_BAD_POINTER = "an array is NULL, not device memory of the batch's device, or misaligned";

// working memory of one call, carved from the handle's block in 256-byte steps; sizing: the same calls with base = nullptr
struct GrCarve {
    char *base; size_t at = 0;
    template <class T> T *take(size_t n) { T *p = base ? (T *)(base + at) : nullptr; at += (n * sizeof(T) + 255) / 256 * 256; return p; }
};
template <class BE> bool graphs_work(BE &be, GraphsCore &h, size_t bytes) {
    h.ksw.valid = false;                                             // (a k-walk result lived there)
    if (bytes > h.work_cap) {
        be.quiesce();
        if (h.work) be.free_dev(h.work);
        h.work = nullptr; h.work_cap = 0;
        if (!(h.work = (char *)be.alloc(bytes))) return false;
        h.work_cap = bytes;
    }
    be.poison(h.work, bytes);
    return true;
}
// ... and more of it in the middle of a call (k-walks size their arenas from the tree stage's counts): the first `keep` bytes stay -
// copied where the block has to be replaced, after which every pointer into it is stale -, the rest is poisoned.  A block that cannot
// be had leaves the old one in place.
template <class BE> bool graphs_work_more(BE &be, GraphsCore &h, size_t keep, size_t bytes) {
    if (bytes > h.work_cap) {
        char *p = (char *)be.alloc(bytes);
        if (!p) return false;
        const bool ok = be.d2d(p, h.work, keep) && be.sync();
        be.free_dev(ok ? h.work : p);
        if (!ok) return false;
        h.work = p; h.work_cap = bytes;
    }
    be.poison(h.work + keep, bytes - keep);
    return true;
}
template <class BE> int64_t *graphs_up(BE &be, GraphsCore &h, const std::vector<int64_t> &x) {
    int64_t *p = (int64_t *)be.alloc(x.size() * 8);
    if (p) { h.own.push_back(p); if (!be.h2d(p, x.data(), x.size() * 8)) return nullptr; }
    return p;
}
static inline int64_t gr_blocks(int64_t items) { const int64_t b = (items + 255) / 256; return b < 1 ? 1 : b > GR_MAX_BLOCKS ? GR_MAX_BLOCKS : b; }
static inline GraphsArgs gr_args(const GraphsCore &h) {
    GraphsArgs a;
    memset(&a, 0, sizeof(a));
    a.n_graphs = h.view.n_graphs; a.n_vertices = h.view.n_vertices; a.n_edges = h.view.n_edges;
    a.voff = h.view.g_voff; a.rowptr = h.view.rowptr; a.col = h.view.col; a.w5 = h.view.w5; a.cost = h.view.cost; a.lim = h.view.lim;
    a.words = h.words;
    return a;
}
static inline SsspArgs gr_sssp_args(const GraphsCore &h, const int32_t *src) {
    SsspArgs a;
    memset(&a, 0, sizeof(a));
    a.n_graphs = h.view.n_graphs; a.voff = h.view.g_voff; a.rowptr = h.view.rowptr; a.col = h.view.col; a.src = src;
    return a;
}
// one verdict word of a launch: filled, lowered by the kernel, read back (the call's host wait)
template <class BE> bool graphs_verdict(BE &be, GraphsCore &h, int kid, int64_t items, const GraphsArgs &a, int64_t *out, int n_words = 1) {
    return be.fill(h.words, 0x7f, GR_W_N * 8) && be.launch_gr(kid, gr_blocks(items), a) && be.read(out, h.words, (size_t)n_words * 8);
}

template <class BE> void graphs_destroy(BE &be, GraphsCore *h) {
    if (!h) return;
    for (void *p : h->own) be.free_dev(p);
    if (h->work) be.free_dev(h->work);
    delete h;
}

// The host checks of a resident batch, in the order the stages ask them on the device: layout, the two ends, heads, w5, lim, cost.
static inline int graphs_check_host(const aasm_graphs_in &in, const char **why) {
    int rc = check_graph_batch(in.n_graphs, in.g_voff, in.rowptr, in.col, nullptr, {}, why, false, in.n_vertices < 0 ? INT64_MAX : in.n_vertices,
                               in.n_edges < 0 ? INT64_MAX : in.n_edges);
    if (rc == AASM_OK && in.w5) rc = check_w5(in.w5, in.n_edges, true, why);
    if (rc == AASM_OK && in.cost) rc = check_dial_costs(in.cost, in.n_edges, in.lim, why);
    return rc;
}
// A verdict of stage 1 / 2 / 3 as the host checks' code and message; lim: dial's, asked between the w5 clauses and the costs.
static inline int graphs_verdict_fail(int stage, int64_t word, const aasm_graphs_in &in, const char **why) {
    const int reason = (int)(word >> GR_POS_BITS);
    const int64_t pos = word & (((int64_t)1 << GR_POS_BITS) - 1);
    const bool bad_lim = in.cost && (in.lim < 0 || in.lim >= DIAL_MAXB);
    if (stage == 3) {
        if (word != GR_PASS && reason == GR_HEAD) return check_fail(why, AASM_E_INVAL, "graph " + std::to_string(pos) + ": edge head outside the graph");
        if (word != GR_PASS && reason == GR_W5) return w5_fail(pos, true, why);
        if (bad_lim) return dial_lim_fail(why);
        return word == GR_PASS ? AASM_OK : dial_cost_fail(pos, why);
    }
    if (word == GR_PASS) return AASM_OK;
    if (stage == 1)
        return check_fail(why, AASM_E_INVAL, reason == GR_START ? std::string("graph offsets do not start at 0") :
                          reason == GR_ORDER ? "graph " + std::to_string(pos) + ": empty, or graph offsets not increasing" : std::string("graph offsets do not end at n_vertices"));
    return check_fail(why, AASM_E_INVAL, reason == GR_START ? std::string("row pointers do not start at 0") :
                      reason == GR_ORDER ? "row pointers decrease at vertex " + std::to_string(pos) : std::string("row pointers do not end at n_edges"));
}

// what both creation paths share once the batch is checked and h.view / h.gv / h.ge / h.first_neg are set: the largest graph, the
// entries' offsets, the verdict words
template <class BE> int graphs_finish(BE &be, GraphsCore &h) {
    const int64_t G = h.view.n_graphs;
    for (int i = 0; i < 4; i++) h.ho[i].assign((size_t)G + 1, 0);
    h.qo.assign((size_t)G + 1, 0); h.so.assign((size_t)G + 1, 0);
    const int nb = h.view.lim + 1;
    for (int64_t g = 0; g < G; g++) {
        const int64_t V = h.gv[(size_t)g + 1] - h.gv[(size_t)g], E = h.ge[(size_t)g + 1] - h.ge[(size_t)g];
        if (V > h.max_v) h.max_v = V;
        if (E > h.max_e) h.max_e = E;
        int64_t mult = 1;
        for (int i = 0; i < 4; i++, mult *= 4) h.ho[i][(size_t)g + 1] = h.ho[i][(size_t)g] + mult * (E + 2);   // dijkstra_run's
        h.qo[(size_t)g + 1] = h.qo[(size_t)g] + 2 * (E + 2);                                                   // bf_queue_offsets'
        if (h.view.cost) {                                                                                     // dial_run's
            const int64_t by_v = V * (int64_t)nb, per = ((E + 1 < by_v ? E + 1 : by_v) + DIAL_WIN + 63) / 64 * 64;
            h.so[(size_t)g + 1] = h.so[(size_t)g] + per * nb;
        }
    }
    if (!h.words) {
        if (!(h.words = (int64_t *)be.alloc(GR_W_N * 8))) return be.err();
        h.own.push_back(h.words);
    }
    if (h.view.w5 && (!(h.d_ho[0] = graphs_up(be, h, h.ho[0])) || !(h.d_qo = graphs_up(be, h, h.qo)))) return be.err();
    if (h.view.cost && !(h.d_so = graphs_up(be, h, h.so))) return be.err();
    return be.sync() ? AASM_OK : be.err();
}

// aasm_graphs_upload after graphs_check_host has passed: copies of the arrays, owned by the handle
template <class BE> int graphs_upload(BE &be, const aasm_graphs_in &in, GraphsCore **out) {
    GraphsCore *h = new GraphsCore;
    const int64_t G = in.n_graphs, VT = in.n_vertices, ET = in.n_edges;
    h->view = in;
    auto up = [&](const void *src, size_t bytes) -> void * {
        void *p = be.alloc(bytes ? bytes : 16);
        if (p) { h->own.push_back(p); if (bytes && !be.h2d(p, src, bytes)) return nullptr; }
        return p;
    };
    bool ok = (h->view.g_voff = (const int64_t *)up(in.g_voff, (size_t)(G + 1) * 8)) && (h->view.rowptr = (const int64_t *)up(in.rowptr, (size_t)(VT + 1) * 8)) &&
              (h->view.col = (const int32_t *)up(in.col, (size_t)ET * 4));
    if (ok && in.w5) ok = (h->view.w5 = (const int64_t *)up(in.w5, (size_t)ET * 40)) != nullptr;
    if (ok && in.cost) ok = (h->view.cost = (const int32_t *)up(in.cost, (size_t)ET * 4)) != nullptr;
    if (!ok) { const int rc = be.err(); graphs_destroy(be, h); return rc; }
    h->gv.assign(in.g_voff, in.g_voff + G + 1);
    h->ge.resize((size_t)G + 1);
    for (int64_t g = 0; g <= G; g++) h->ge[(size_t)g] = in.rowptr[in.g_voff[g]];
    if (in.w5) for (int64_t e = 0; e < ET; e++) if (in.w5[5 * e] + in.w5[5 * e + 1] < 0) { h->first_neg = e; break; }
    const int rc = graphs_finish(be, *h);
    if (rc != AASM_OK) { graphs_destroy(be, h); return rc; }
    *out = h;
    return AASM_OK;
}

// aasm_graphs_wrap_device: the arrays are borrowed, and checked where they are
template <class BE> int graphs_wrap(BE &be, const aasm_graphs_in &in, GraphsCore **out, const char **why) {
    if (in.n_graphs <= 0 || !in.g_voff || !in.rowptr || !in.col) return check_fail(why, AASM_E_INVAL, "empty batch or NULL pointer");
    if (!be.dev_ok(in.g_voff, in.n_graphs + 1, 8) || !be.dev_ok(in.rowptr, in.n_vertices + 1, 8) || !be.dev_ok(in.col, in.n_edges, 4) ||
        !be.dev_ok(in.w5, in.w5 ? in.n_edges : 0, 8) || !be.dev_ok(in.cost, in.cost ? in.n_edges : 0, 4)) return check_fail(why, AASM_E_INVAL, GR_BAD_POINTER);
    GraphsCore *h = new GraphsCore;
    h->view = in;
    const int64_t G = in.n_graphs;
    int rc = AASM_OK;
    int64_t *counts = nullptr;
    if (!(h->words = (int64_t *)be.alloc(GR_W_N * 8))) rc = be.err();
    else h->own.push_back(h->words);
    GraphsArgs a = gr_args(*h);
    int64_t word[GR_W_N] = {GR_PASS, GR_PASS};
    // stage 1, stage 2: one verdict each, the next launch only after a pass
    if (rc == AASM_OK && !graphs_verdict(be, *h, GR_K_CHECK_VOFF, G, a, word)) rc = be.err();
    if (rc == AASM_OK) rc = graphs_verdict_fail(1, word[0], in, why);
    if (rc == AASM_OK && !graphs_verdict(be, *h, GR_K_CHECK_ROWPTR, in.n_vertices, a, word)) rc = be.err();
    if (rc == AASM_OK) rc = graphs_verdict_fail(2, word[0], in, why);
    // stage 3 with the counts behind it: one wait for both
    if (rc == AASM_OK) {
        std::vector<int64_t> gc(2 * ((size_t)G + 1));
        a.gcount = counts = (int64_t *)be.alloc(gc.size() * 8);
        if (!counts || !be.launch_gr(GR_K_COUNTS, gr_blocks(G + 1), a) || !graphs_verdict(be, *h, GR_K_CHECK_EDGES, in.n_edges, a, word, GR_W_N) ||
            !be.read(gc.data(), counts, gc.size() * 8)) rc = be.err();
        else rc = graphs_verdict_fail(3, word[0], in, why);
        h->gv.assign(gc.begin(), gc.begin() + G + 1);
        h->ge.assign(gc.begin() + G + 1, gc.end());
        if (word[GR_W_NEG] != GR_PASS) h->first_neg = word[GR_W_NEG];
    }
    if (counts) be.free_dev(counts);
    if (rc == AASM_OK) rc = graphs_finish(be, *h);
    if (rc != AASM_OK) { graphs_destroy(be, h); return rc; }
    *out = h;
    return AASM_OK;
}

// ---- the entries ---------------------------------------------------------------------------------------------------------------------
// What every entry asks before anything is enqueued: the pointers, the batch's arrays, the size limits.
template <class BE> int graphs_call_checks(BE &be, const GraphsCore &h, bool need_w5, bool need_cost, bool dag_limit,
                                           std::initializer_list<std::pair<const void *, std::pair<int64_t, int>>> arrays, const char **why) {
    for (const auto &x : arrays)
        if (x.second.first > 0 && (!x.first || !be.dev_ok(x.first, x.second.first, (size_t)x.second.second))) return check_fail(why, AASM_E_INVAL, GR_BAD_POINTER);
    if (need_w5 && !h.view.w5) return check_fail(why, AASM_E_INVAL, "the batch carries no w5 weights");
    if (need_cost && !h.view.cost) return check_fail(why, AASM_E_INVAL, "the batch carries no costs");
    const bool big = h.max_v > INT32_MAX || h.max_e > INT32_MAX || (dag_limit && h.max_v > AASM_DAG_MAX_V);   // (else no graph can fail)
    for (int64_t g = 0; big && g < h.view.n_graphs; g++) {
        const int64_t V = h.gv[(size_t)g + 1] - h.gv[(size_t)g], E = h.ge[(size_t)g + 1] - h.ge[(size_t)g];
        if (dag_limit && V > AASM_DAG_MAX_V) return check_fail(why, AASM_E_OVERFLOW, "graph " + std::to_string(g) + ": more than 2^20 vertices");
        if (V > INT32_MAX || E > INT32_MAX) return check_fail(why, AASM_E_OVERFLOW, "graph " + std::to_string(g) + ": 2^31 vertices or edges, or more");
    }
    return AASM_OK;
}
#define GR_ARR(p, n, align) std::pair<const void *, std::pair<int64_t, int>>{(const void *)(p), {(int64_t)(n), (int)(align)}}
// the sources, by the kernel: the call's one host wait
template <class BE> int graphs_check_src(BE &be, GraphsCore &h, const int32_t *src, const char **why) {
    GraphsArgs a = gr_args(h);
    a.src = src;
    int64_t word = GR_PASS;
    if (!graphs_verdict(be, h, GR_K_CHECK_SRC, h.view.n_graphs, a, &word)) return be.err();
    return word == GR_PASS ? AASM_OK : check_fail(why, AASM_E_INVAL, "graph " + std::to_string(word) + ": source outside it");
}
template <class BE> bool graphs_d5(BE &be, GraphsCore &h, const Dist *d, int64_t *d5) {
    GraphsArgs a = gr_args(h);
    a.d = d; a.d5 = d5;
    return be.launch_gr(GR_K_D5, gr_blocks(5 * h.view.n_vertices), a);
}

template <class BE> int graphs_dijkstra(BE &be, GraphsCore &h, const int32_t *src, int64_t *d5, int32_t *prev, const char **why) {
    const int64_t G = h.view.n_graphs, VT = h.view.n_vertices;
    int rc = graphs_call_checks(be, h, true, false, false, {GR_ARR(src, G, 4), GR_ARR(d5, 5 * VT, 8), GR_ARR(prev, VT, 4)}, why);
    if (rc != AASM_OK) return rc;
    if (h.first_neg >= 0) return w5_fail(h.first_neg, false, why);
    if ((rc = graphs_check_src(be, h, src, why)) != AASM_OK) return rc;
    SsspArgs a = gr_sssp_args(h, src);
    a.w5 = h.view.w5; a.prv = prev;
    int64_t over = GR_PASS;
    for (int i = 0; i < 4; i++) {                                    // heap room 1x, 4x, 16x, 64x (dijkstra_run's comment)
        if (!h.d_ho[i] && !(h.d_ho[i] = graphs_up(be, h, h.ho[i]))) return be.err();
        GrCarve c{nullptr};
        for (int pass = 0; pass < 2; pass++) {
            c.at = 0;
            a.d = c.take<Dist>((size_t)VT); a.heap = c.take<DjEnt>((size_t)h.ho[i][(size_t)G]);
            if (pass == 0) { if (!graphs_work(be, h, c.at)) return be.err(); c.base = h.work; }
        }
        a.hoff = h.d_ho[i];
        GraphsArgs r = gr_args(h);
        r.src = src; r.prv = prev;
        if (!be.launch(SSSP_K_DIJKSTRA, G, a) || !graphs_verdict(be, h, GR_K_DJ_OVER, G, r, &over)) return be.err();
        if (over == GR_PASS) break;
    }
    if (over != GR_PASS) return check_fail(why, AASM_E_OVERFLOW, "graph " + std::to_string(over) + ": dijkstra heap capacity exceeded at 64 x (E + 2) entries");
    return graphs_d5(be, h, a.d, d5) && be.sync() ? AASM_OK : be.err();
}

template <class BE> int graphs_bellman_ford(BE &be, GraphsCore &h, const int32_t *src, int64_t *d5, int32_t *prev, int32_t *status, int64_t *cycle_off,
                                            int32_t *cycle, const char **why) {
    const int64_t G = h.view.n_graphs, VT = h.view.n_vertices;
    int rc = graphs_call_checks(be, h, true, false, false, {GR_ARR(src, G, 4), GR_ARR(d5, 5 * VT, 8), GR_ARR(prev, VT, 4), GR_ARR(status, G, 4),
                                                              GR_ARR(cycle_off, G + 1, 8), GR_ARR(cycle, VT + G, 4)}, why);
    if (rc != AASM_OK || (rc = graphs_check_src(be, h, src, why)) != AASM_OK) return rc;
    SsspArgs a = gr_sssp_args(h, src);
    a.w5 = h.view.w5; a.prv = prev; a.status = status; a.hoff = h.d_qo;
    GrCarve c{nullptr};
    for (int pass = 0; pass < 2; pass++) {
        c.at = 0;
        a.d = c.take<Dist>((size_t)VT); a.mark = c.take<int32_t>((size_t)VT); a.heap = c.take<DjEnt>((size_t)h.qo[(size_t)G]);
        a.clen = c.take<int64_t>((size_t)G); a.qhigh = c.take<int64_t>((size_t)G); a.cyc = c.take<int32_t>((size_t)(VT + G));
        if (pass == 0) { if (!graphs_work(be, h, c.at)) return be.err(); c.base = h.work; }
    }
    GraphsArgs r = gr_args(h);
    r.clen = a.clen; r.cyc = a.cyc; r.cycle_off = cycle_off; r.cycle = cycle;
    return be.launch(SSSP_K_BELLMAN_FORD, G, a) && graphs_d5(be, h, a.d, d5) && be.launch_gr(GR_K_CYCLE_SCAN, 1, r) && be.launch_gr(GR_K_CYCLE_COPY, G, r) ? AASM_OK : be.err();
}

// aasm_sssp_dag_device, and with sort_only aasm_topology_sort_device (no src, d5, prev)
template <class BE> int graphs_dag(BE &be, GraphsCore &h, const int32_t *src, int64_t *d5, int32_t *prev, int32_t *order, int32_t *status, bool sort_only,
                                   const char **why) {
    const int64_t G = h.view.n_graphs, VT = h.view.n_vertices;
    int rc = sort_only ? graphs_call_checks(be, h, false, false, false, {GR_ARR(order, VT, 4), GR_ARR(status, G, 4)}, why)
                       : graphs_call_checks(be, h, true, false, true, {GR_ARR(src, G, 4), GR_ARR(d5, 5 * VT, 8), GR_ARR(prev, VT, 4), GR_ARR(status, G, 4),
                                                                        GR_ARR(order ? order : status, order ? VT : G, 4)}, why);
    if (rc != AASM_OK || (!sort_only && (rc = graphs_check_src(be, h, src, why)) != AASM_OK)) return rc;
    SsspArgs a = gr_sssp_args(h, sort_only ? nullptr : src);
    a.status = status;
    if (!sort_only) { a.w5 = h.view.w5; a.prv = prev; }
    GrCarve c{nullptr};
    for (int pass = 0; pass < 2; pass++) {
        c.at = 0;
        a.mark = c.take<int32_t>((size_t)VT);
        a.order = order ? order : c.take<int32_t>((size_t)VT);
        if (!sort_only) { a.d = c.take<Dist>((size_t)VT); a.claim = c.take<int32_t>((size_t)VT); }
        if (pass == 0) { if (!graphs_work(be, h, c.at)) return be.err(); c.base = h.work; }
    }
    return be.launch(SSSP_K_DAG, G, a) && (sort_only || graphs_d5(be, h, a.d, d5)) ? AASM_OK : be.err();
}

template <class BE> int graphs_dial(BE &be, GraphsCore &h, const int32_t *src, int64_t *dist, int64_t *pre, int32_t *status, const char **why) {
    const int64_t G = h.view.n_graphs, VT = h.view.n_vertices;
    int rc = graphs_call_checks(be, h, false, true, false, {GR_ARR(src, G, 4), GR_ARR(dist, VT, 8), GR_ARR(pre, VT, 8), GR_ARR(status, G, 4)}, why);
    if (rc != AASM_OK || (rc = graphs_check_src(be, h, src, why)) != AASM_OK) return rc;
    SsspArgs a = gr_sssp_args(h, src);
    a.cost = h.view.cost; a.nb = h.view.lim + 1; a.soff = h.d_so; a.dist = dist; a.pre = pre;
    if (!graphs_work(be, h, (size_t)h.so[(size_t)G] * 4)) return be.err();
    a.spill = (int32_t *)h.work;
    GraphsArgs r = gr_args(h);
    r.src = src; r.pre = pre; r.status = status;
    return be.launch(SSSP_K_DIAL, G, a) && be.launch_gr(GR_K_DIAL_STATUS, gr_blocks(G), r) ? AASM_OK : be.err();
}

// ---- k shortest walks: aasm_k_shortest_walks_device / aasm_ksw_export_device -----------------------------------------------------------
// ksw_run (aasm_ksw.h) on a resident batch, the whole batch in one piece of the handle's working memory: what ksw_run's host loops
// size per chunk of graphs, kb_gr_ksw_bounds sizes and places on the device, and the host reads totals.  Of the backend, beside the
// above: bool d2d(dst, src, n) (enqueued), bool launch_ksw(kernel, n_graphs, KswArgs).
// The working memory's fixed part: everything ksw_run allocates before its chunks, copies of the sources and sinks (the export runs
// kb_ksw_fill after the caller's arrays may be gone), the shares' offsets and the scans.  The kernel bodies ask nothing of fresh
// memory - every tree kernel starts by writing its graph's per-vertex arrays (deg 0 / the out-degree, depth -1, ...), kb_ksw_heap
// writes hroot and hcount of every graph, kb_ksw_enum nfound, kb_ksw_count wtot -, so the block is used as the poison fill left it.
struct KswLay {
    KswArgs a;
    int32_t *src, *sink;
    int64_t *aoff, *acap, *qoff, *qcap, *rofs, *wbase, *foff, *hoff, *ktot;
    GrCarve c;                                                       // c.at: the fixed part's end, where the stages' tails begin
};
static inline KswLay ksw_lay(const GraphsCore &h, char *base, int64_t k, int flags) {
    const size_t G = (size_t)h.view.n_graphs, VT = (size_t)h.view.n_vertices, ET = (size_t)h.view.n_edges;
    KswLay l;
    memset(&l.a, 0, sizeof(l.a));
    l.c = GrCarve{base};
    GrCarve &c = l.c;
    KswArgs &a = l.a;
    a.n_graphs = h.view.n_graphs; a.k = k; a.cycles = (flags & AASM_KSW_CYCLES) != 0;
    a.voff = h.view.g_voff; a.rowptr = h.view.rowptr; a.col = h.view.col; a.w5 = h.view.w5;
    a.src = l.src = c.take<int32_t>(G); a.sink = l.sink = c.take<int32_t>(G);
    int32_t **v32[] = {&a.roff, &a.deg, &a.order, &a.best, &a.bedge, &a.koff, &a.kids, &a.bfs, &a.depth, &a.hroot};
    for (int32_t **p : v32) *p = c.take<int32_t>(VT);
    a.d = c.take<Dist>(VT); a.cnt = c.take<int64_t>(VT);
    a.rev = c.take<int32_t>(ET); a.etail = c.take<int32_t>(ET);
    a.status = c.take<int32_t>(G);
    int64_t **g64[] = {&a.nbfs, &a.ins, &a.walks, &a.hcount, &a.nfound, &a.wtot, &l.aoff, &l.acap, &l.qoff, &l.qcap, &l.rofs, &l.wbase};
    for (int64_t **p : g64) *p = c.take<int64_t>(G);
    a.aoff = l.aoff; a.acap = l.acap; a.qoff = l.qoff; a.qcap = l.qcap; a.rofs = l.rofs; a.wbase = l.wbase;
    l.foff = c.take<int64_t>(G + 1); l.hoff = c.take<int64_t>(G + 1); l.ktot = c.take<int64_t>(GR_KT_N);
    return l;
}
static inline GraphsArgs ksw_gr_args(const GraphsCore &h, const KswLay &l) {
    GraphsArgs r = gr_args(h);
    r.src = l.src; r.sink = l.sink; r.status = l.a.status;
    r.ins = l.a.ins; r.walks = l.a.walks; r.nfound = l.a.nfound; r.wtot = l.a.wtot; r.hcount = l.a.hcount;
    r.acap = l.acap; r.qcap = l.qcap; r.aoff = l.aoff; r.qoff = l.qoff; r.rofs = l.rofs;
    r.hoff = l.hoff; r.foff = l.foff; r.wbase = l.wbase; r.ktot = l.ktot;
    return r;
}

template <class BE> int graphs_ksw(BE &be, GraphsCore &h, const int32_t *source, const int32_t *sink, int64_t k, int flags, aasm_ksw_sizes *sz,
                                   const char **why) {
    const int64_t G = h.view.n_graphs, VT = h.view.n_vertices;
    if (!sz) return check_fail(why, AASM_E_INVAL, "empty batch or NULL pointer");
    for (const int32_t *p : {source, sink}) if (!p || !be.dev_ok(p, G, 4)) return check_fail(why, AASM_E_INVAL, GR_BAD_POINTER);
    if (!h.view.w5) return check_fail(why, AASM_E_INVAL, "the batch carries no w5 weights");
    const bool big = h.max_v > AASM_KSW_MAX_V || h.max_e > INT32_MAX;  // (else no graph can fail; ksw_check_args' messages)
    for (int64_t g = 0; big && g < G; g++) {
        if (h.gv[(size_t)g + 1] - h.gv[(size_t)g] > AASM_KSW_MAX_V) return check_fail(why, AASM_E_OVERFLOW, "graph " + std::to_string(g) + ": more than 2^20 vertices");
        if (h.ge[(size_t)g + 1] - h.ge[(size_t)g] > INT32_MAX) return check_fail(why, AASM_E_OVERFLOW, "graph " + std::to_string(g) + ": 2^31 edges or more");
    }
    if (k < 1 || k > AASM_KSW_MAX_K) return check_fail(why, AASM_E_INVAL, "k outside 1 .. 2^24");
    if (flags & ~(AASM_KSW_WALKS | AASM_KSW_TREE | AASM_KSW_CYCLES | AASM_KSW_NEGATIVE)) return check_fail(why, AASM_E_INVAL, "unknown flag");
    if (!(flags & AASM_KSW_NEGATIVE) && h.first_neg >= 0) return w5_fail(h.first_neg, false, why);
    {   // the sources and sinks, by the kernel: the call's first host wait
        GraphsArgs r = gr_args(h);
        r.src = source; r.sink = sink;
        int64_t word = GR_PASS;
        if (!graphs_verdict(be, h, GR_K_KSW_CHECK, G, r, &word)) return be.err();
        if (word != GR_PASS) return check_fail(why, AASM_E_INVAL, "graph " + std::to_string(word >> 1) + ((word & 1) ? ": sink outside it" : ": source outside it"));
    }
    const bool cycles = flags & AASM_KSW_CYCLES, negative = flags & AASM_KSW_NEGATIVE, want_walks = flags & AASM_KSW_WALKS;
    // the tree stage: the fixed part, behind it the heap room of dijkstra's first round (E + 2 entries per graph) or bellman_ford's
    // queue rings (exact: 2 * (E + 2))
    const size_t fixed = ksw_lay(h, nullptr, k, flags).c.at;
    const int64_t room0 = !cycles ? 0 : negative ? h.qo[(size_t)G] : h.ho[0][(size_t)G];
    if (!graphs_work(be, h, fixed + (size_t)room0 * sizeof(DjEnt))) return be.err();
    KswLay l = ksw_lay(h, h.work, k, flags);
    if (!be.d2d(l.src, source, (size_t)G * 4) || !be.d2d(l.sink, sink, (size_t)G * 4)) return be.err();
    int64_t tot[GR_KT_N] = {0, 0, 0, 0};
    if (!cycles) {                                                   // (AASM_KSW_NEGATIVE: the DAG relaxation assumes no sign)
        if (!be.launch_ksw(KSW_K_TREE, G, l.a)) return be.err();
    } else if (negative) {
        KswArgs a = l.a;
        a.hoff = h.d_qo; a.dheap = l.c.take<DjEnt>((size_t)room0);
        if (!be.launch_ksw(KSW_K_TREE_BF, G, a)) return be.err();
    } else {
        // heap room as ksw_run gives it: E + 2 entries, then 4x, 16x, 64x for the graphs that ran out of it, chosen by
        // kb_gr_ksw_retry; at 64x the kernel's bound on pushes ends a graph first, so nobody asks for a fifth round
        KswArgs a = l.a;
        a.hoff = h.d_ho[0]; a.dheap = l.c.take<DjEnt>((size_t)room0);
        if (!be.launch_ksw(KSW_K_TREE_CYC, G, a)) return be.err();
        for (int64_t mult = 4; mult <= AASM_KSW_DJ_PUSHES; mult *= 4) {
            GraphsArgs r = ksw_gr_args(h, l);
            r.mult = mult;
            if (!be.launch_gr(GR_K_KSW_RETRY, 1, r) || !be.read(tot, l.ktot, 8)) return be.err();
            if (tot[0] == 0) break;
            if (!graphs_work_more(be, h, fixed, fixed + (size_t)tot[0] * sizeof(DjEnt))) return be.err();
            l = ksw_lay(h, h.work, k, flags);
            a = l.a;
            a.hoff = l.hoff; a.dheap = l.c.take<DjEnt>((size_t)tot[0]);
            if (!be.launch_ksw(KSW_K_TREE_CYC, G, a)) return be.err();
        }
    }
    // the enumeration's room from the tree stage's counts: three totals
    GraphsArgs r = ksw_gr_args(h, l);
    if (!be.launch_gr(GR_K_KSW_BOUNDS, 1, r) || !be.read(tot, l.ktot, 3 * 8)) return be.err();
    const size_t na = (size_t)tot[0], nq = (size_t)tot[1], nr = (size_t)tot[2];
    KswArgs a;
    for (int pass = 0; pass < 2; pass++) {
        l = ksw_lay(h, pass ? h.work : nullptr, k, flags);
        a = l.a;
        a.arena = l.c.take<KswNode>(na); a.q = l.c.take<KswQE>(nq); a.qnode = l.c.take<int32_t>(nq); a.qprev = l.c.take<int32_t>(nq);
        a.rdist = l.c.take<Dist>(nr); a.rlast = l.c.take<int32_t>(nr); a.woff = l.c.take<int64_t>(nr);
        if (pass == 0 && !graphs_work_more(be, h, fixed, l.c.at)) return be.err();
    }
    r = ksw_gr_args(h, l);
    if (!want_walks) r.wtot = nullptr;
    if (!be.launch_ksw(KSW_K_HEAP, G, a) || !be.launch_ksw(KSW_K_ENUM, G, a) || (want_walks && !be.launch_ksw(KSW_K_COUNT, G, a)) ||
        !be.launch_gr(GR_K_KSW_TOTALS, 1, r) || !be.read(tot, l.ktot, 2 * 8)) return be.err();
    memset(sz, 0, sizeof(*sz));
    sz->n_graphs = G; sz->n_vertices = VT; sz->k = k; sz->n_walks = tot[0]; sz->n_walk_edges = tot[1]; sz->flags = flags;
    sz->serial = ++h.ksw.serial;
    h.ksw.sz = *sz; h.ksw.a = a; h.ksw.foff = l.foff; h.ksw.valid = true;
    return AASM_OK;
}

// The export of the handle's latest k-walk solve: every check before the first enqueue, then launches only.
template <class BE> int graphs_ksw_export(BE &be, GraphsCore &h, const aasm_ksw_sizes *sz, const aasm_ksw_dev_out *dst, const char **why) {
    if (!sz || !dst) return check_fail(why, AASM_E_INVAL, "empty batch or NULL pointer");
    if (!h.ksw.valid || memcmp(sz, &h.ksw.sz, sizeof(*sz)) != 0)
        return check_fail(why, AASM_E_INVAL, "the sizes are not those of the handle's latest k-walk solve, or a later call has reused its working memory");
    const int64_t G = sz->n_graphs, VT = sz->n_vertices, NW = sz->n_walks, NE = sz->n_walk_edges;
    const bool want_walks = sz->flags & AASM_KSW_WALKS, want_tree = sz->flags & AASM_KSW_TREE;
    const int rc = graphs_call_checks(be, h, true, false, false, {GR_ARR(dst->n_found, G, 8), GR_ARR(dst->found_off, G + 1, 8), GR_ARR(dst->dist5, 5 * NW, 8),
        GR_ARR(dst->heap_nodes, G, 8), GR_ARR(dst->status, G, 4), GR_ARR(dst->walk_off, want_walks ? NW + 1 : 0, 8), GR_ARR(dst->walk_edges, want_walks ? NE : 0, 8),
        GR_ARR(dst->d5, want_tree ? 5 * VT : 0, 8), GR_ARR(dst->best, want_tree ? VT : 0, 4)}, why);
    if (rc != AASM_OK) return rc;
    const KswArgs &a = h.ksw.a;
    GraphsArgs r = gr_args(h);
    r.status = a.status; r.nfound = a.nfound; r.hcount = a.hcount; r.rofs = (int64_t *)a.rofs; r.foff = h.ksw.foff; r.wbase = (int64_t *)a.wbase;
    r.rdist = a.rdist; r.woff = a.woff; r.n_walks = NW; r.n_walk_edges = NE;
    r.o_nfound = dst->n_found; r.o_foff = dst->found_off; r.o_dist5 = dst->dist5; r.o_woff = dst->walk_off; r.o_heap = dst->heap_nodes; r.o_status = dst->status;
    if (!be.launch_gr(GR_K_KSW_PACK_GRAPHS, gr_blocks(G + 1), r) || (NW > 0 && !be.launch_gr(GR_K_KSW_PACK_DIST, gr_blocks(5 * NW), r))) return be.err();
    if (want_walks) {
        KswArgs f = a;                                               // kb_ksw_fill, straight into the caller's array
        f.wedges = dst->walk_edges;
        if (!be.launch_gr(GR_K_KSW_PACK_WOFF, gr_blocks(NW + 1), r) || (NE > 0 && !be.launch_ksw(KSW_K_FILL, G, f))) return be.err();
    }
    if (want_tree && (!graphs_d5(be, h, a.d, dst->d5) || !be.d2d(dst->best, a.best, (size_t)VT * 4))) return be.err();
    return AASM_OK;
}

}  // namespace aasm
