// tests/host_emul/bf_emul.cpp -- TEST INFRASTRUCTURE ONLY.
//
// graphs_emul.cpp's entries with aasm_sssp_bellman_ford beside them (alignasm_amd/csrc/aasm_sssp.h: kb_sssp_bellman_ford, its argument
// checks and its host driver), compiled for the HOST as there: one working lane per wave, so a chunk of a list is one edge and the
// kernel is the reference's own walk.  With AASM_BF_SAN_MAIN a program for the host address sanitizer (bf.mk).
#include "graphs_emul.cpp"

extern "C" {
// aasm_sssp_bellman_ford() without a device.  qhigh: NULL, or n_graphs cells for the high-water marks of the graphs' queues (a debug
// return: the room is 2 * (E + 2) entries, emk_bf_queue_room).
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
}

#if defined(AASM_BF_SAN_MAIN)
#include <cstdio>
// bf_emul_san IN OUT.  IN = int64 words {G, K, flags, VT, ET}, g_voff[G + 1], rowptr[VT + 1], col[ET], w5[5 * ET], src[G], sink[G].
// Every graph is run on its own, each array a heap block of exactly its size, so the sanitizer ends the program at the first cell
// touched outside one: emk_sssp_bellman_ford, and where its status is 0 emk_k_shortest_walks with `flags` too.
// OUT = per graph {status, cycle length, n_found, ksw status}, d5[5 * V], prev[V], the cycle, dist5[5 * n_found].
template <class T, class S> static T *exact(const S *src, int64_t n) {
    T *p = (T *)std::malloc((size_t)(n ? n : 1) * sizeof(T));
    for (int64_t i = 0; i < n; i++) p[i] = src ? (T)src[i] : (T)0;
    return p;
}
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int64_t> raw;
    int64_t word;
    while (std::fread(&word, 8, 1, f) == 1) raw.push_back(word);
    std::fclose(f);
    if (raw.size() < 5) return 2;
    const int64_t G = raw[0], K = raw[1], flags = raw[2], VT = raw[3], ET = raw[4];
    if ((int64_t)raw.size() != 5 + (G + 1) + (VT + 1) + ET + 5 * ET + 2 * G) return 2;
    const int64_t *g_voff = raw.data() + 5, *rowptr = g_voff + G + 1, *col = rowptr + VT + 1, *w5 = col + ET, *src = w5 + 5 * ET, *sink = src + G;
    std::vector<int64_t> out;
    for (int64_t g = 0; g < G; g++) {
        const int64_t vb = g_voff[g], V = g_voff[g + 1] - vb, eb = rowptr[vb], E = rowptr[vb + V] - eb;
        const int64_t voff1[2] = {0, V};
        int64_t *vo = exact<int64_t>(voff1, 2), *rp = exact<int64_t>(rowptr + vb, V + 1), *w = exact<int64_t>(w5 + 5 * eb, 5 * E);
        for (int64_t v = 0; v <= V; v++) rp[v] -= eb;
        int32_t *cl = exact<int32_t>(col + eb, E), *s = exact<int32_t>(src + g, 1), *t = exact<int32_t>(sink + g, 1);
        int64_t *d5 = exact<int64_t>((const int64_t *)nullptr, 5 * V), *coff = exact<int64_t>((const int64_t *)nullptr, 2);
        int32_t *prev = exact<int32_t>((const int64_t *)nullptr, V), *st = exact<int32_t>((const int64_t *)nullptr, 1);
        int32_t *cyc = exact<int32_t>((const int64_t *)nullptr, V + 1);
        if (emk_sssp_bellman_ford(1, vo, rp, cl, w, s, d5, prev, st, coff, cyc, nullptr) != AASM_OK) return 3;
        aasm_ksw_out *ko = (aasm_ksw_out *)std::calloc(1, sizeof(aasm_ksw_out));
        if (st[0] == 0 && emk_k_shortest_walks(1, vo, rp, cl, w, s, t, K, (int)flags, ko, 0) != AASM_OK) return 4;
        const int64_t nf = st[0] == 0 ? ko->n_found[0] : 0;
        out.insert(out.end(), {(int64_t)st[0], coff[1], nf, st[0] == 0 ? (int64_t)ko->status[0] : 0});
        out.insert(out.end(), d5, d5 + 5 * V);
        out.insert(out.end(), prev, prev + V);
        out.insert(out.end(), cyc, cyc + coff[1]);
        if (nf) out.insert(out.end(), ko->dist5, ko->dist5 + 5 * nf);
        emk_free(ko);
        void *blocks[] = {vo, rp, w, cl, s, t, d5, coff, prev, st, cyc, ko};
        for (void *p : blocks) std::free(p);
    }
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), 8, out.size(), f) != out.size()) return 2;
    std::fclose(f);
    return 0;
}
#endif
