// tests/host_emul/graphs_emul.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The graph family, compiled for the HOST: a workgroup runs as its one working lane (nthreads = 1), so a chunk of a list is one edge
// and a kernel is the reference's own walk; device memory and LDS are poisoned host memory.  The product library never links this
// file; its entries need a HIP device.  Two backends, because the drivers under test expect different contracts:
//  * GraphEmu, the host entries (emk_*): dijkstra, Dial, bellman_ford, topology_sort and shortest_path_dag
//    (alignasm_amd/csrc/aasm_sssp.h) and k shortest walks (aasm_ksw.h) with the product's argument checks and host drivers.
//  * ResidentEmu, resident graph batches (emr_*; aasm_graphs.h: the kernel table AASM_GRAPHS_KERNELS, both creation paths, the five
//    *_device drivers): "device" memory is host memory, so the pointer-attribute checks are skipped (NULL and alignment are still
//    asked), and fresh working memory is poisoned with 0xA5 before every call.  KswResidentEmu over it, k shortest walks on a
//    resident batch (emw_*; graphs_ksw / graphs_ksw_export), counts the bytes a call reads back and can refuse allocations above a
//    size.
// libaasm_emul_graphs.so holds all of them; with AASM_EMUL_SAN_MAIN the same in a program for the host address sanitizer,
// graphs_emul_san MODE IN OUT (at the end of this file).
#define AASM_HOST_EMUL 1
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../alignasm_amd/csrc/aasm_graphs.h"
#include "emul_launch.h"

using namespace aasm;

namespace {
AASM_EMUL_ROWS(ksw_rows, AASM_KSW_KERNELS);
AASM_EMUL_ROWS(sssp_rows, AASM_SSSP_KERNELS);
AASM_EMUL_ROWS(graphs_rows, AASM_GRAPHS_KERNELS);
struct GraphEmu {
    std::vector<void *> blocks;
    ~GraphEmu() { for (void *p : blocks) free(p); }
    void *alloc(size_t n) {
        void *p = malloc(n);
        if (!p) return nullptr;
        memset(p, 0xA5, n);                        // poison: catches reads of never-written cells
        blocks.push_back(p);
        return p;
    }
    size_t mark() const { return blocks.size(); }
    void release(size_t m) { while (blocks.size() > m) { free(blocks.back()); blocks.pop_back(); } }
    bool h2d(void *d, const void *h, size_t n) { memcpy(d, h, n); return true; }
    bool d2h(void *h, const void *d, size_t n) { memcpy(h, d, n); return true; }
    bool sync() { return true; }
    bool launch_from(int kid, int64_t g0, int64_t g1, const KswArgs &a) {
        emul_launch(ksw_rows, kid, ksw_block[kid], g0, g1 - g0, 0, [&](const KCtx &k) { run_ksw_body(kid, k, a); });
        return true;
    }
    bool launch(int kid, int64_t n_graphs, const SsspArgs &a) {
        emul_launch(sssp_rows, kid, sssp_block[kid], 0, n_graphs, 0, [&](const KCtx &k) { run_sssp_body(kid, k, a); });
        return true;
    }
    int err() { return AASM_E_NOMEM; }
};
struct ResidentEmu : GraphEmu {
    void *alloc(size_t n) {                                          // (outlives the backend: the handle frees it)
        void *p = malloc(n ? n : 16);
        if (p) memset(p, 0xA5, n ? n : 16);
        return p;
    }
    void free_dev(void *p) { free(p); }
    bool fill(void *d, int byte, size_t n) { memset(d, byte, n); return true; }
    bool read(void *h, const void *d, size_t n) { memcpy(h, d, n); return true; }
    void poison(void *d, size_t n) { memset(d, 0xA5, n); }
    void quiesce() {}
    bool dev_ok(const void *p, int64_t n, size_t align) { return n <= 0 || (p && (uintptr_t)p % align == 0); }
    bool launch_gr(int kid, int64_t nblocks, const GraphsArgs &a) {
        emul_launch(graphs_rows, kid, graphs_block[kid], 0, nblocks, 0, [&](const KCtx &k) { run_graphs_body(kid, k, a); });
        return true;
    }
};
int64_t emw_read = 0, emw_limit = 0;
struct KswResidentEmu : ResidentEmu {
    void *alloc(size_t n) { return emw_limit > 0 && (int64_t)n > emw_limit ? nullptr : ResidentEmu::alloc(n); }
    bool read(void *h, const void *d, size_t n) { emw_read += (int64_t)n; memcpy(h, d, n); return true; }
    bool d2d(void *d, const void *s, size_t n) { if (n) memcpy(d, s, n); return true; }
    bool launch_ksw(int kid, int64_t n_graphs, const KswArgs &a) {
        emul_launch(ksw_rows, kid, ksw_block[kid], 0, n_graphs, 0, [&](const KCtx &k) { run_ksw_body(kid, k, a); });
        return true;
    }
};
thread_local std::string emr_error;                                  // the latest emr_* / emw_* call's message, of this thread
int emr_done(int rc, const char *why) { emr_error = why; return rc; }
}  // namespace

extern "C" {
// ---- the host entries, without a device ----------------------------------------------------------------------------------------
// aasm_k_shortest_walks(); budget: bytes of "device" memory per chunk of graphs (<= 0: the product's 4 GiB)
int emk_k_shortest_walks(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5,
                         const int32_t *source, const int32_t *sink, int64_t k, int flags, aasm_ksw_out *out, int64_t budget) {
    const char *why = "";
    const int rc = ksw_check_args(n_graphs, g_voff, rowptr, col, w5, source, sink, k, flags, out, &why);
    if (rc != AASM_OK) return rc;
    GraphEmu be;
    return ksw_run(be, n_graphs, g_voff, rowptr, col, w5, source, sink, k, flags, out, budget > 0 ? budget : (int64_t)4 << 30);
}
void emk_free(aasm_ksw_out *out) { ksw_free_out(out); }

// aasm_sssp_dijkstra()
int emk_sssp_dijkstra(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5,
                      const int32_t *src, int64_t *d5, int32_t *prev) {
    const char *why = "";
    const int rc = dijkstra_check_args(n_graphs, g_voff, rowptr, col, w5, src, d5, prev, &why);
    if (rc != AASM_OK) return rc;
    GraphEmu be;
    return dijkstra_run(be, n_graphs, g_voff, rowptr, col, w5, src, d5, prev, &why);
}

// aasm_sssp_dial()
int emk_sssp_dial(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int32_t *cost,
                  const int32_t *src, int lim, int64_t *dist, int64_t *pre) {
    const char *why = "";
    const int rc = dial_check_args(n_graphs, g_voff, rowptr, col, cost, src, lim, dist, pre, &why);
    if (rc != AASM_OK) return rc;
    GraphEmu be;
    return dial_run(be, n_graphs, g_voff, rowptr, col, cost, src, lim, dist, pre, &why);
}

// aasm_sssp_bellman_ford().  qhigh: NULL, or n_graphs cells for the high-water marks of the graphs' queues (a debug return: the room
// is 2 * (E + 2) entries, emk_bf_queue_room).
int emk_sssp_bellman_ford(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5,
                          const int32_t *src, int64_t *d5, int32_t *prev, int32_t *status, int64_t *cycle_off, int32_t *cycle, int64_t *qhigh) {
    const char *why = "";
    const int rc = bellman_ford_check_args(n_graphs, g_voff, rowptr, col, w5, src, d5, prev, status, cycle_off, cycle, &why);
    if (rc != AASM_OK) return rc;
    GraphEmu be;
    return bellman_ford_run(be, n_graphs, g_voff, rowptr, col, w5, src, d5, prev, status, cycle_off, cycle, qhigh, &why);
}
int64_t emk_bf_queue_room(int64_t n_edges) {
    const int64_t voff[2] = {0, 1}, rp[2] = {0, n_edges};
    return bf_queue_offsets(1, voff, rp)[1];
}

// aasm_topology_sort()
int emk_topology_sort(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, int32_t *order, int32_t *status) {
    const char *why = "";
    const int rc = dag_check_args(n_graphs, g_voff, rowptr, col, nullptr, nullptr, nullptr, nullptr, order, status, true, &why);
    if (rc != AASM_OK) return rc;
    GraphEmu be;
    return dag_run(be, n_graphs, g_voff, rowptr, col, nullptr, nullptr, nullptr, nullptr, order, status, &why);
}
// aasm_sssp_dag(); order may be NULL
int emk_sssp_dag(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5, const int32_t *src,
                 int64_t *d5, int32_t *prev, int32_t *order, int32_t *status) {
    const char *why = "";
    const int rc = dag_check_args(n_graphs, g_voff, rowptr, col, w5, src, d5, prev, order, status, false, &why);
    if (rc != AASM_OK) return rc;
    GraphEmu be;
    return dag_run(be, n_graphs, g_voff, rowptr, col, w5, src, d5, prev, order, status, &why);
}

// ---- resident graph batches ----------------------------------------------------------------------------------------------------
const char *emr_last_error() { return emr_error.c_str(); }
// graphs_check_host alone: what aasm_graphs_upload answers before it touches a device
int emr_host_check(const aasm_graphs_in *in) {
    const char *why = "";
    const int rc = graphs_check_host(*in, &why);
    return emr_done(rc, why);
}
// aasm_graphs_upload (wrap = 0: the host checks, then copies) / aasm_graphs_wrap_device (wrap = 1: the check kernels, the arrays borrowed)
int emr_graphs_make(const aasm_graphs_in *in, int wrap, void **gb) {
    const char *why = "";
    ResidentEmu be;
    GraphsCore *core = nullptr;
    int rc = wrap ? graphs_wrap(be, *in, &core, &why) : graphs_check_host(*in, &why);
    if (rc == AASM_OK && !wrap) rc = graphs_upload(be, *in, &core);
    *gb = core;
    return emr_done(rc, why);
}
void emr_graphs_free(void *gb) { ResidentEmu be; graphs_destroy(be, (GraphsCore *)gb); }
int64_t emr_first_negative(void *gb) { return ((GraphsCore *)gb)->first_neg; }
int64_t emr_work_bytes(void *gb) { return (int64_t)((GraphsCore *)gb)->work_cap; }
int emr_dijkstra(void *gb, const int32_t *src, int64_t *d5, int32_t *prev) {
    const char *why = "";
    ResidentEmu be;
    const int rc = graphs_dijkstra(be, *(GraphsCore *)gb, src, d5, prev, &why);
    return emr_done(rc, why);
}
int emr_bellman_ford(void *gb, const int32_t *src, int64_t *d5, int32_t *prev, int32_t *status, int64_t *cycle_off, int32_t *cycle) {
    const char *why = "";
    ResidentEmu be;
    const int rc = graphs_bellman_ford(be, *(GraphsCore *)gb, src, d5, prev, status, cycle_off, cycle, &why);
    return emr_done(rc, why);
}
int emr_topology_sort(void *gb, int32_t *order, int32_t *status) {
    const char *why = "";
    ResidentEmu be;
    const int rc = graphs_dag(be, *(GraphsCore *)gb, nullptr, nullptr, nullptr, order, status, true, &why);
    return emr_done(rc, why);
}
int emr_dag(void *gb, const int32_t *src, int64_t *d5, int32_t *prev, int32_t *order, int32_t *status) {
    const char *why = "";
    ResidentEmu be;
    const int rc = graphs_dag(be, *(GraphsCore *)gb, src, d5, prev, order, status, false, &why);
    return emr_done(rc, why);
}
int emr_dial(void *gb, const int32_t *src, int64_t *dist, int64_t *pre, int32_t *status) {
    const char *why = "";
    ResidentEmu be;
    const int rc = graphs_dial(be, *(GraphsCore *)gb, src, dist, pre, status, &why);
    return emr_done(rc, why);
}

// ---- k shortest walks on a resident batch --------------------------------------------------------------------------------------
int emw_solve(void *gb, const int32_t *source, const int32_t *sink, int64_t k, int flags, aasm_ksw_sizes *sz) {
    const char *why = "";
    KswResidentEmu be;
    emw_read = 0;
    const int rc = graphs_ksw(be, *(GraphsCore *)gb, source, sink, k, flags, sz, &why);
    return emr_done(rc, why);
}
int emw_export(void *gb, const aasm_ksw_sizes *sz, const aasm_ksw_dev_out *dst) {
    const char *why = "";
    KswResidentEmu be;
    emw_read = 0;
    const int rc = graphs_ksw_export(be, *(GraphsCore *)gb, sz, dst, &why);
    return emr_done(rc, why);
}
int64_t emw_read_bytes() { return emw_read; }                         // what the latest solve / export read back
void emw_alloc_limit(int64_t bytes) { emw_limit = bytes; }            // allocations above it are refused (0: none is)
}

#if defined(AASM_EMUL_SAN_MAIN)
#include "emul_san.h"
// graphs_emul_san MODE IN OUT.  IN and OUT are files of int64 words, their layout the mode's.  In every mode each input and output
// array is a heap block of exactly its size, so the sanitizer ends the program at the first cell touched outside one.  Exit codes:
// 0, 2 for a file or a mode that cannot be used, from 3 on what the mode says.
using namespace emul_san;
namespace {
// MODE bf.  IN = {G, K, flags, VT, ET}, g_voff[G + 1], rowptr[VT + 1], col[ET], w5[5 * ET], src[G], sink[G].  Every graph is run on
// its own: emk_sssp_bellman_ford (else 3), and where its status is 0 emk_k_shortest_walks with `flags` too (else 4).
// OUT = per graph {status, cycle length, n_found, ksw status}, d5[5 * V], prev[V], the cycle, dist5[5 * n_found].
int san_bf(const std::vector<int64_t> &raw, std::vector<int64_t> &out) {
    if (raw.size() < 5) return 2;
    const int64_t G = raw[0], K = raw[1], flags = raw[2], VT = raw[3], ET = raw[4];
    if ((int64_t)raw.size() != 5 + (G + 1) + (VT + 1) + ET + 5 * ET + 2 * G) return 2;
    const int64_t *g_voff = raw.data() + 5, *rowptr = g_voff + G + 1, *col = rowptr + VT + 1, *w5 = col + ET, *src = w5 + 5 * ET, *sink = src + G;
    for (int64_t g = 0; g < G; g++) {
        const int64_t vb = g_voff[g], V = g_voff[g + 1] - vb, eb = rowptr[vb], E = rowptr[vb + V] - eb;
        const int64_t voff1[2] = {0, V};
        int64_t *vo = exact<int64_t>(voff1, 2), *rp = exact<int64_t>(rowptr + vb, V + 1), *w = exact<int64_t>(w5 + 5 * eb, 5 * E);
        for (int64_t v = 0; v <= V; v++) rp[v] -= eb;
        int32_t *cl = exact<int32_t>(col + eb, E), *s = exact<int32_t>(src + g, 1), *t = exact<int32_t>(sink + g, 1);
        int64_t *d5 = zeros<int64_t>(5 * V), *coff = zeros<int64_t>(2);
        int32_t *prev = zeros<int32_t>(V), *st = zeros<int32_t>(1), *cyc = zeros<int32_t>(V + 1);
        if (emk_sssp_bellman_ford(1, vo, rp, cl, w, s, d5, prev, st, coff, cyc, nullptr) != AASM_OK) return 3;
        aasm_ksw_out *ko = (aasm_ksw_out *)std::calloc(1, sizeof(aasm_ksw_out));
        if (st[0] == 0 && emk_k_shortest_walks(1, vo, rp, cl, w, s, t, K, (int)flags, ko, 0) != AASM_OK) return 4;
        const int64_t nf = st[0] == 0 ? ko->n_found[0] : 0;
        out.insert(out.end(), {(int64_t)st[0], coff[1], nf, st[0] == 0 ? (int64_t)ko->status[0] : 0});
        put(out, d5, 5 * V); put(out, prev, V); put(out, cyc, coff[1]);
        if (nf) put(out, ko->dist5, 5 * nf);
        emk_free(ko);
        void *blocks[] = {vo, rp, w, cl, s, t, d5, coff, prev, st, cyc, ko};
        for (void *p : blocks) std::free(p);
    }
    return 0;
}

// MODE dag.  IN = {G, VT, ET}, g_voff[G + 1], rowptr[VT + 1], col[ET], w5[5 * ET], src[G].  Every graph is run on its own:
// emk_sssp_dag with its order (else 3), and emk_topology_sort (else 4), whose status and order must be the same (else 5).
// OUT = per graph {status}, d5[5 * V], prev[V], order[V].
int san_dag(const std::vector<int64_t> &raw, std::vector<int64_t> &out) {
    if (raw.size() < 3) return 2;
    const int64_t G = raw[0], VT = raw[1], ET = raw[2];
    if ((int64_t)raw.size() != 3 + (G + 1) + (VT + 1) + ET + 5 * ET + G) return 2;
    const int64_t *g_voff = raw.data() + 3, *rowptr = g_voff + G + 1, *col = rowptr + VT + 1, *w5 = col + ET, *src = w5 + 5 * ET;
    for (int64_t g = 0; g < G; g++) {
        const int64_t vb = g_voff[g], V = g_voff[g + 1] - vb, eb = rowptr[vb], E = rowptr[vb + V] - eb;
        const int64_t voff1[2] = {0, V};
        int64_t *vo = exact<int64_t>(voff1, 2), *rp = exact<int64_t>(rowptr + vb, V + 1), *w = exact<int64_t>(w5 + 5 * eb, 5 * E);
        for (int64_t v = 0; v <= V; v++) rp[v] -= eb;
        int32_t *cl = exact<int32_t>(col + eb, E), *s = exact<int32_t>(src + g, 1);
        int64_t *d5 = zeros<int64_t>(5 * V);
        int32_t *prev = zeros<int32_t>(V), *order = zeros<int32_t>(V), *order2 = zeros<int32_t>(V), *st = zeros<int32_t>(1), *st2 = zeros<int32_t>(1);
        if (emk_sssp_dag(1, vo, rp, cl, w, s, d5, prev, order, st) != AASM_OK) return 3;
        if (emk_topology_sort(1, vo, rp, cl, order2, st2) != AASM_OK) return 4;
        if (st[0] != st2[0] || std::memcmp(order, order2, (size_t)V * 4) != 0) return 5;
        out.push_back(st[0]);
        put(out, d5, 5 * V); put(out, prev, V); put(out, order, V);
        void *blocks[] = {vo, rp, w, cl, s, d5, prev, order, order2, st, st2};
        for (void *p : blocks) std::free(p);
    }
    return 0;
}

// MODE resident.  IN = {G, NV, NE, has_w5, has_cost, lim} - NV, NE the lengths as STATED -, then g_voff[G + 1], rowptr[NV + 1],
// col[NE], w5[5 * NE] (has_w5), cost[NE] (has_cost), src[G].  The batch is made by both creation paths, which must agree (else 3); a
// refused batch gives OUT = {rc} and the message on stdout.  Else all five entries run on the wrapped batch (topology_sort on the
// uploaded one): OUT = {0}, then per entry {rc} and, where rc is 0, its outputs as int64 in the entry's argument order, dag's order
// last (dijkstra, bellman_ford, topology_sort, dag, dial; an entry whose array the batch lacks gives its AASM_E_INVAL).
int san_resident(const std::vector<int64_t> &raw, std::vector<int64_t> &out, std::string &said) {
    if (raw.size() < 6) return 2;
    const int64_t G = raw[0], NV = raw[1], NE = raw[2], has_w5 = raw[3], has_cost = raw[4], lim = raw[5];
    if (G < 1 || NV < 0 || NE < 0 || (int64_t)raw.size() != 6 + (G + 1) + (NV + 1) + NE + (has_w5 ? 5 * NE : 0) + (has_cost ? NE : 0) + G) return 2;
    const int64_t *p = raw.data() + 6;
    aasm_graphs_in in;
    memset(&in, 0, sizeof(in));
    in.n_graphs = G; in.n_vertices = NV; in.n_edges = NE; in.lim = (int32_t)lim;
    int64_t *voff = exact<int64_t>(p, G + 1); p += G + 1;
    int64_t *rp = exact<int64_t>(p, NV + 1); p += NV + 1;
    int32_t *col = exact<int32_t>(p, NE); p += NE;
    int64_t *w5 = has_w5 ? exact<int64_t>(p, 5 * NE) : nullptr; p += has_w5 ? 5 * NE : 0;
    int32_t *cost = has_cost ? exact<int32_t>(p, NE) : nullptr; p += has_cost ? NE : 0;
    int32_t *src = exact<int32_t>(p, G);
    in.g_voff = voff; in.rowptr = rp; in.col = col; in.w5 = w5; in.cost = cost;
    void *wrapped = nullptr, *uploaded = nullptr;
    const int rc = emr_graphs_make(&in, 1, &wrapped);
    const std::string msg = emr_last_error();
    const int rc2 = emr_graphs_make(&in, 0, &uploaded);
    if (rc != rc2 || msg != emr_last_error()) return 3;
    out.push_back(rc);
    if (rc == AASM_OK) {
        int64_t *d5 = zeros<int64_t>(5 * NV), *coff = zeros<int64_t>(G + 1), *dist = zeros<int64_t>(NV), *pre = zeros<int64_t>(NV);
        int32_t *prev = zeros<int32_t>(NV), *st = zeros<int32_t>(G), *cyc = zeros<int32_t>(NV + G), *order = zeros<int32_t>(NV);
        int r = emr_dijkstra(wrapped, src, d5, prev);
        out.push_back(r);
        if (r == AASM_OK) { put(out, d5, 5 * NV); put(out, prev, NV); }
        r = emr_bellman_ford(wrapped, src, d5, prev, st, coff, cyc);
        out.push_back(r);
        if (r == AASM_OK) { put(out, d5, 5 * NV); put(out, prev, NV); put(out, st, G); put(out, coff, G + 1); put(out, cyc, coff[G]); }
        r = emr_topology_sort(uploaded, order, st);
        out.push_back(r);
        if (r == AASM_OK) { put(out, order, NV); put(out, st, G); }
        r = emr_dag(wrapped, src, d5, prev, order, st);
        out.push_back(r);
        if (r == AASM_OK) { put(out, d5, 5 * NV); put(out, prev, NV); put(out, st, G); put(out, order, NV); }
        r = emr_dial(wrapped, src, dist, pre, st);
        out.push_back(r);
        if (r == AASM_OK) { put(out, dist, NV); put(out, pre, NV); put(out, st, G); }
        void *blocks[] = {d5, coff, dist, pre, prev, st, cyc, order};
        for (void *b : blocks) std::free(b);
        emr_graphs_free(wrapped); emr_graphs_free(uploaded);
    } else {
        said = msg;
    }
    void *blocks[] = {voff, rp, col, w5, cost, src};
    for (void *b : blocks) std::free(b);
    return 0;
}

// MODE ksw_resident.  IN = {G, NV, NE, has_w5, k, flags, mode}, then g_voff[G + 1], rowptr[NV + 1], col[NE], w5[5 * NE] (has_w5),
// source[G], sink[G].  The batch is made by both creation paths and solved on both, which must agree (else 6).
// mode: 1 the export gets a serial one too high, 2 a topology_sort runs between solve and export (which must succeed, else 3), 4 dist5
// is NULL.  OUT = {rc} of the first call that refused (its message on stdout), else {0, n_walks, n_walk_edges} and n_found, found_off,
// dist5, heap_nodes, status, then walk_off, walk_edges (AASM_KSW_WALKS), d5, best (AASM_KSW_TREE), exported twice, which must agree
// (else 5) and read nothing back (else 4).
int san_ksw_resident(const std::vector<int64_t> &raw, std::vector<int64_t> &out, std::string &said) {
    if (raw.size() < 7) return 2;
    const int64_t G = raw[0], NV = raw[1], NE = raw[2], has_w5 = raw[3], k = raw[4], flags = raw[5], mode = raw[6];
    if (G < 1 || NV < 0 || NE < 0 || (int64_t)raw.size() != 7 + (G + 1) + (NV + 1) + NE + (has_w5 ? 5 * NE : 0) + 2 * G) return 2;
    const int64_t *p = raw.data() + 7;
    aasm_graphs_in in;
    memset(&in, 0, sizeof(in));
    in.n_graphs = G; in.n_vertices = NV; in.n_edges = NE;
    int64_t *voff = exact<int64_t>(p, G + 1); p += G + 1;
    int64_t *rp = exact<int64_t>(p, NV + 1); p += NV + 1;
    int32_t *col = exact<int32_t>(p, NE); p += NE;
    int64_t *w5 = has_w5 ? exact<int64_t>(p, 5 * NE) : nullptr; p += has_w5 ? 5 * NE : 0;
    int32_t *src = exact<int32_t>(p, G); p += G;
    int32_t *sink = exact<int32_t>(p, G);
    in.g_voff = voff; in.rowptr = rp; in.col = col; in.w5 = w5;
    std::vector<void *> blocks = {voff, rp, col, w5, src, sink};
    std::vector<int64_t> result[2];
    for (int wrap = 0; wrap < 2; wrap++) {
        void *gb = nullptr;
        int rc = emr_graphs_make(&in, wrap, &gb);
        aasm_ksw_sizes sz;
        if (rc == AASM_OK) rc = emw_solve(gb, src, sink, k, (int)flags, &sz);
        std::vector<int64_t> first;
        for (int round = 0; round < 2 && rc == AASM_OK; round++) {
            aasm_ksw_dev_out o;
            memset(&o, 0, sizeof(o));
            const bool ww = flags & AASM_KSW_WALKS, wt = flags & AASM_KSW_TREE;
            o.n_found = zeros<int64_t>(G); o.found_off = zeros<int64_t>(G + 1); o.dist5 = (mode & 4) ? nullptr : zeros<int64_t>(5 * sz.n_walks);
            o.heap_nodes = zeros<int64_t>(G); o.status = zeros<int32_t>(G);
            if (ww) { o.walk_off = zeros<int64_t>(sz.n_walks + 1); o.walk_edges = zeros<int64_t>(sz.n_walk_edges); }
            if (wt) { o.d5 = zeros<int64_t>(5 * NV); o.best = zeros<int32_t>(NV); }
            void *mine[] = {o.n_found, o.found_off, o.dist5, o.heap_nodes, o.status, o.walk_off, o.walk_edges, o.d5, o.best};
            blocks.insert(blocks.end(), mine, mine + 9);
            aasm_ksw_sizes s2 = sz;
            if (mode & 1) s2.serial++;
            if (mode & 2) {
                int32_t *order = zeros<int32_t>(NV), *st = zeros<int32_t>(G);
                blocks.push_back(order); blocks.push_back(st);
                if (emr_topology_sort(gb, order, st) != AASM_OK) return 3;
            }
            rc = emw_export(gb, &s2, &o);
            if (rc != AASM_OK) break;
            if (emw_read_bytes() != 0) return 4;                     // the export reads nothing back
            std::vector<int64_t> now = {0, sz.n_walks, sz.n_walk_edges};
            put(now, o.n_found, G); put(now, o.found_off, G + 1); put(now, o.dist5, 5 * sz.n_walks); put(now, o.heap_nodes, G); put(now, o.status, G);
            if (ww) { put(now, o.walk_off, sz.n_walks + 1); put(now, o.walk_edges, sz.n_walk_edges); }
            if (wt) { put(now, o.d5, 5 * NV); put(now, o.best, NV); }
            if (round == 0) first = now;
            else if (now != first) return 5;
        }
        if (rc != AASM_OK) { result[wrap].assign(1, rc); said = emr_last_error(); }
        else result[wrap] = first;
        if (gb) emr_graphs_free(gb);
    }
    for (void *b : blocks) std::free(b);
    if (result[0] != result[1]) return 6;
    out = result[0];
    return 0;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const std::string mode = argv[1];
    std::vector<int64_t> raw, out;
    std::string said;
    if (!read_words(argv[2], raw)) return 2;
    const int rc = mode == "bf" ? san_bf(raw, out) : mode == "dag" ? san_dag(raw, out) : mode == "resident" ? san_resident(raw, out, said)
                 : mode == "ksw_resident" ? san_ksw_resident(raw, out, said) : 2;
    if (rc != 0) return rc;
    std::fputs(said.c_str(), stdout);
    return write_words(argv[3], out) ? 0 : 2;
}
#endif
