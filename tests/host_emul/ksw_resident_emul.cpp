// tests/host_emul/ksw_resident_emul.cpp -- TEST INFRASTRUCTURE ONLY.
//
// k shortest walks on a resident graph batch (alignasm_amd/csrc/aasm_graphs.h: graphs_ksw / graphs_ksw_export and the kernels around
// aasm_ksw.h's) over graphs_resident_emul.cpp's ResidentEmu, compiled for the HOST, beside the emulated host driver
// (emk_k_shortest_walks) it is checked against.  The backend counts the bytes a call reads back and can refuse allocations above a
// size.  With AASM_KSWR_SAN_MAIN a program for the host address sanitizer (ksw_resident.mk).
#include "graphs_resident_emul.cpp"

namespace {
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
}  // namespace

extern "C" {
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

#if defined(AASM_KSWR_SAN_MAIN)
#include <cstdio>
// ksw_resident_emul_san IN OUT.  IN = int64 words {G, NV, NE, has_w5, k, flags, mode}, then g_voff[G + 1], rowptr[NV + 1], col[NE],
// w5[5 * NE] (has_w5), source[G], sink[G].  Every input and output array is a heap block of exactly its size, so the sanitizer ends
// the program at the first cell touched outside one.  The batch is made by both creation paths and solved on both, which must agree.
// mode: 1 the export gets a serial one too high, 2 a topology_sort runs between solve and export, 4 dist5 is NULL.
// OUT = {rc} of the first call that refused (its message on stdout), else {0, n_walks, n_walk_edges} and n_found, found_off, dist5,
// heap_nodes, status, then walk_off, walk_edges (AASM_KSW_WALKS), d5, best (AASM_KSW_TREE), exported twice, which must agree.
template <class T> static T *exact(const int64_t *src, int64_t n) {
    T *p = (T *)std::malloc((size_t)(n > 0 ? n : 0) * sizeof(T) + (n > 0 ? 0 : 1));
    for (int64_t i = 0; i < n; i++) p[i] = src ? (T)src[i] : (T)0;
    return p;
}
template <class T> static void put(std::vector<int64_t> &out, const T *p, int64_t n) { for (int64_t i = 0; i < n; i++) out.push_back((int64_t)p[i]); }
static int finish(const char *path, const std::vector<int64_t> &out, const std::string &msg) {
    std::fputs(msg.c_str(), stdout);
    FILE *f = std::fopen(path, "wb");
    if (!f || std::fwrite(out.data(), 8, out.size(), f) != out.size()) return 2;
    std::fclose(f);
    return 0;
}
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int64_t> raw;
    int64_t word;
    while (std::fread(&word, 8, 1, f) == 1) raw.push_back(word);
    std::fclose(f);
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
    std::string msg;
    int bad = 0;
    for (int wrap = 0; wrap < 2; wrap++) {
        std::vector<int64_t> &out = result[wrap];
        void *gb = nullptr;
        int rc = emr_graphs_make(&in, wrap, &gb);
        aasm_ksw_sizes sz;
        if (rc == AASM_OK) rc = emw_solve(gb, src, sink, k, (int)flags, &sz);
        std::vector<int64_t> first;
        for (int round = 0; round < 2 && rc == AASM_OK; round++) {
            aasm_ksw_dev_out o;
            memset(&o, 0, sizeof(o));
            const bool ww = flags & AASM_KSW_WALKS, wt = flags & AASM_KSW_TREE;
            o.n_found = exact<int64_t>(nullptr, G); o.found_off = exact<int64_t>(nullptr, G + 1); o.dist5 = (mode & 4) ? nullptr : exact<int64_t>(nullptr, 5 * sz.n_walks);
            o.heap_nodes = exact<int64_t>(nullptr, G); o.status = exact<int32_t>(nullptr, G);
            if (ww) { o.walk_off = exact<int64_t>(nullptr, sz.n_walks + 1); o.walk_edges = exact<int64_t>(nullptr, sz.n_walk_edges); }
            if (wt) { o.d5 = exact<int64_t>(nullptr, 5 * NV); o.best = exact<int32_t>(nullptr, NV); }
            void *mine[] = {o.n_found, o.found_off, o.dist5, o.heap_nodes, o.status, o.walk_off, o.walk_edges, o.d5, o.best};
            blocks.insert(blocks.end(), mine, mine + 9);
            aasm_ksw_sizes s2 = sz;
            if (mode & 1) s2.serial++;
            if (mode & 2) {
                int32_t *order = exact<int32_t>(nullptr, NV), *st = exact<int32_t>(nullptr, G);
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
        if (rc != AASM_OK) { out.assign(1, rc); msg = emr_last_error(); bad++; }
        else out = first;
        if (gb) emr_graphs_free(gb);
    }
    for (void *b : blocks) std::free(b);
    if (result[0] != result[1]) return 6;
    return finish(argv[2], result[0], bad ? msg : std::string());
}
#endif
