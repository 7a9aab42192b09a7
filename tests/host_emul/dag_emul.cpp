// tests/host_emul/dag_emul.cpp -- TEST INFRASTRUCTURE ONLY.
//
// graphs_emul.cpp's entries with aasm_topology_sort and aasm_sssp_dag beside them (alignasm_amd/csrc/aasm_sssp.h: kb_sssp_dag, its
// argument checks and its host driver), compiled for the HOST as there: one working lane per wave, so a chunk of a list is one edge
// and the kernel is the reference's own walk.  With AASM_DAG_SAN_MAIN a program for the host address sanitizer (dag.mk).
#include "graphs_emul.cpp"

extern "C" {
// aasm_topology_sort() without a device
int emk_topology_sort(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, int32_t *order, int32_t *status) {
    const char *why = "";
    const int rc = dag_check_args(n_graphs, g_voff, rowptr, col, nullptr, nullptr, nullptr, nullptr, order, status, true, &why);
    if (rc != AASM_OK) return rc;
    GraphEmu be;
    return dag_run(be, n_graphs, g_voff, rowptr, col, nullptr, nullptr, nullptr, nullptr, order, status, &why);
}
// aasm_sssp_dag() without a device; order may be NULL
int emk_sssp_dag(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5, const int32_t *src,
                 int64_t *d5, int32_t *prev, int32_t *order, int32_t *status) {
    const char *why = "";
    const int rc = dag_check_args(n_graphs, g_voff, rowptr, col, w5, src, d5, prev, order, status, false, &why);
    if (rc != AASM_OK) return rc;
    GraphEmu be;
    return dag_run(be, n_graphs, g_voff, rowptr, col, w5, src, d5, prev, order, status, &why);
}
}

#if defined(AASM_DAG_SAN_MAIN)
#include <cstdio>
// dag_emul_san IN OUT.  IN = int64 words {G, VT, ET}, g_voff[G + 1], rowptr[VT + 1], col[ET], w5[5 * ET], src[G].
// Every graph is run on its own, each array a heap block of exactly its size, so the sanitizer ends the program at the first cell
// touched outside one: emk_sssp_dag with its order, and emk_topology_sort, whose order must be the same.
// OUT = per graph {status}, d5[5 * V], prev[V], order[V].
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
    if (raw.size() < 3) return 2;
    const int64_t G = raw[0], VT = raw[1], ET = raw[2];
    if ((int64_t)raw.size() != 3 + (G + 1) + (VT + 1) + ET + 5 * ET + G) return 2;
    const int64_t *g_voff = raw.data() + 3, *rowptr = g_voff + G + 1, *col = rowptr + VT + 1, *w5 = col + ET, *src = w5 + 5 * ET;
    std::vector<int64_t> out;
    for (int64_t g = 0; g < G; g++) {
        const int64_t vb = g_voff[g], V = g_voff[g + 1] - vb, eb = rowptr[vb], E = rowptr[vb + V] - eb;
        const int64_t voff1[2] = {0, V};
        int64_t *vo = exact<int64_t>(voff1, 2), *rp = exact<int64_t>(rowptr + vb, V + 1), *w = exact<int64_t>(w5 + 5 * eb, 5 * E);
        for (int64_t v = 0; v <= V; v++) rp[v] -= eb;
        int32_t *cl = exact<int32_t>(col + eb, E), *s = exact<int32_t>(src + g, 1);
        int64_t *d5 = exact<int64_t>((const int64_t *)nullptr, 5 * V);
        int32_t *prev = exact<int32_t>((const int64_t *)nullptr, V), *order = exact<int32_t>((const int64_t *)nullptr, V);
        int32_t *order2 = exact<int32_t>((const int64_t *)nullptr, V);
        int32_t *st = exact<int32_t>((const int64_t *)nullptr, 1), *st2 = exact<int32_t>((const int64_t *)nullptr, 1);
        if (emk_sssp_dag(1, vo, rp, cl, w, s, d5, prev, order, st) != AASM_OK) return 3;
        if (emk_topology_sort(1, vo, rp, cl, order2, st2) != AASM_OK) return 4;
        if (st[0] != st2[0] || std::memcmp(order, order2, (size_t)V * 4) != 0) return 5;
        out.push_back(st[0]);
        out.insert(out.end(), d5, d5 + 5 * V);
        out.insert(out.end(), prev, prev + V);
        out.insert(out.end(), order, order + V);
        void *blocks[] = {vo, rp, w, cl, s, d5, prev, order, order2, st, st2};
        for (void *p : blocks) std::free(p);
    }
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(out.data(), 8, out.size(), f) != out.size()) return 2;
    std::fclose(f);
    return 0;
}
#endif
