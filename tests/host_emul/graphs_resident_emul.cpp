// tests/host_emul/graphs_resident_emul.cpp -- TEST INFRASTRUCTURE ONLY.
//
// Resident graph batches (alignasm_amd/csrc/aasm_graphs.h: the kernel table AASM_GRAPHS_KERNELS, both creation paths, the five
// *_device drivers) over graphs_emul.cpp's GraphEmu, compiled for the HOST: "device" memory is host memory, so the pointer-attribute
// checks are skipped (NULL and alignment are still asked), a workgroup runs its lanes one after the other, and fresh working memory is
// poisoned with 0xA5 before every call.  With AASM_GRAPHS_SAN_MAIN a program for the host address sanitizer (graphs_resident.mk).
#include "graphs_emul.cpp"

#include "../../alignasm_amd/csrc/aasm_graphs.h"

namespace {
AASM_EMUL_ROWS(graphs_rows, AASM_GRAPHS_KERNELS);
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
thread_local std::string emr_error;
int emr_done(int rc, const char *why) { emr_error = why; return rc; }
}  // namespace

extern "C" {
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
}

#if defined(AASM_GRAPHS_SAN_MAIN)
#include <cstdio>
// graphs_resident_emul_san IN OUT.  IN = int64 words {G, NV, NE, has_w5, has_cost, lim} - NV, NE the lengths as STATED -, then
// g_voff[G + 1], rowptr[NV + 1], col[NE], w5[5 * NE] (has_w5), cost[NE] (has_cost), src[G].  Every input and output array is a heap
// block of exactly its size, so the sanitizer ends the program at the first cell touched outside one.  The batch is made by both
// creation paths, which must agree; a refused batch gives OUT = {rc} and the message on stdout.  Else all five entries run on the
// wrapped batch (topology_sort on the uploaded one): OUT = {0}, then per entry {rc} and, where rc is 0, its outputs as int64 in the
// entry's argument order, dag's order last (dijkstra, bellman_ford, topology_sort, dag, dial; an entry whose array the batch lacks
// gives its AASM_E_INVAL).
template <class T> static T *exact(const int64_t *src, int64_t n) {
    T *p = (T *)std::malloc((size_t)(n > 0 ? n : 0) * sizeof(T) + (n > 0 ? 0 : 1));
    for (int64_t i = 0; i < n; i++) p[i] = src ? (T)src[i] : (T)0;
    return p;
}
template <class T> static void put(std::vector<int64_t> &out, const T *p, int64_t n) { for (int64_t i = 0; i < n; i++) out.push_back((int64_t)p[i]); }
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int64_t> raw;
    int64_t word;
    while (std::fread(&word, 8, 1, f) == 1) raw.push_back(word);
    std::fclose(f);
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
    std::vector<int64_t> out;
    void *wrapped = nullptr, *uploaded = nullptr;
    const int rc = emr_graphs_make(&in, 1, &wrapped);
    const std::string msg = emr_last_error();
    const int rc2 = emr_graphs_make(&in, 0, &uploaded);
    if (rc != rc2 || msg != emr_last_error()) return 3;
    out.push_back(rc);
    if (rc == AASM_OK) {
        int64_t *d5 = exact<int64_t>(nullptr, 5 * NV), *coff = exact<int64_t>(nullptr, G + 1), *dist = exact<int64_t>(nullptr, NV), *pre = exact<int64_t>(nullptr, NV);
        int32_t *prev = exact<int32_t>(nullptr, NV), *st = exact<int32_t>(nullptr, G), *cyc = exact<int32_t>(nullptr, NV + G), *order = exact<int32_t>(nullptr, NV);
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
        std::fputs(msg.c_str(), stdout);
    }
    void *blocks[] = {voff, rp, col, w5, cost, src};
    for (void *b : blocks) std::free(b);
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), 8, out.size(), f) != out.size()) return 2;
    std::fclose(f);
    return 0;
}
#endif
