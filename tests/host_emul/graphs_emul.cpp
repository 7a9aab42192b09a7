// tests/host_emul/graphs_emul.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The generic graph entries - dijkstra and Dial (alignasm_amd/csrc/aasm_sssp.h), k shortest walks (aasm_ksw.h) - with the
// product's argument checks and host drivers, compiled for the HOST: a workgroup runs as its one working lane (nthreads = 1),
// device memory and LDS are poisoned host memory.  The product library never links this file; its entries need a HIP device.
#define AASM_HOST_EMUL 1
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../alignasm_amd/csrc/aasm_ksw.h"
#include "emul_launch.h"

using namespace aasm;

namespace {
AASM_EMUL_ROWS(ksw_rows, AASM_KSW_KERNELS);
AASM_EMUL_ROWS(sssp_rows, AASM_SSSP_KERNELS);
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
}  // namespace

extern "C" {
// aasm_k_shortest_walks() without a device; budget: bytes of "device" memory per chunk of graphs (<= 0: the product's 4 GiB)
int emk_k_shortest_walks(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5,
                         const int32_t *source, const int32_t *sink, int64_t k, int flags, aasm_ksw_out *out, int64_t budget) {
    const char *why = "";
    const int rc = ksw_check_args(n_graphs, g_voff, rowptr, col, w5, source, sink, k, flags, out, &why);
    if (rc != AASM_OK) return rc;
    GraphEmu be;
    return ksw_run(be, n_graphs, g_voff, rowptr, col, w5, source, sink, k, flags, out, budget > 0 ? budget : (int64_t)4 << 30);
}
void emk_free(aasm_ksw_out *out) { ksw_free_out(out); }

// aasm_sssp_dijkstra() without a device
int emk_sssp_dijkstra(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5,
                      const int32_t *src, int64_t *d5, int32_t *prev) {
    const char *why = "";
    const int rc = dijkstra_check_args(n_graphs, g_voff, rowptr, col, w5, src, d5, prev, &why);
    if (rc != AASM_OK) return rc;
    GraphEmu be;
    return dijkstra_run(be, n_graphs, g_voff, rowptr, col, w5, src, d5, prev, &why);
}

// aasm_sssp_dial() without a device
int emk_sssp_dial(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int32_t *cost,
                  const int32_t *src, int lim, int64_t *dist, int64_t *pre) {
    const char *why = "";
    const int rc = dial_check_args(n_graphs, g_voff, rowptr, col, cost, src, lim, dist, pre, &why);
    if (rc != AASM_OK) return rc;
    GraphEmu be;
    return dial_run(be, n_graphs, g_voff, rowptr, col, cost, src, lim, dist, pre, &why);
}
}
