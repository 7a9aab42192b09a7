// tests/host_emul/export_emul.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The device-side export of a result (pack_sizes + pack_export, aasm_pipeline.h; kernels kb_pack_*) run by the 1-lane host
// emulation on the workspace of an emulated solve, beside fetch_results on the same workspace: the test compares the two.
// Reuses emul.cpp (its backend and solve) unchanged.
#include "emul.cpp"

namespace {
PackWS g_pk;
}  // namespace

extern "C" {
// emulated solve; then the pack's sizes (sz[5]: n_contigs, n_main, n_alt, n_all_paths, n_all_elems)
int emx_solve_and_size(const aasm_batch_in *in, const aasm_opts *opts, int64_t *sz) {
    delete g_be;
    g_be = new EmuBackend();
    g_pk = PackWS();
    aasm_opts o{};
    if (opts) o = *opts;
    PipelineSizes ps;
    int rc = run_pipeline(*g_be, *in, o, g_ws, ps);
    if (rc != AASM_OK) return rc;
    rc = pack_alloc(*g_be, g_ws, g_pk);
    if (rc != AASM_OK) return rc;
    rc = pack_sizes(*g_be, g_ws, g_pk);
    if (rc != AASM_OK) return rc;
    for (int i = 0; i < 5; i++) sz[i] = g_pk.sizes[i];
    return AASM_OK;
}
// Breaks the rank invariant of the place kernel on purpose, on the last solve's records, and sizes again: mode 0 gives the
// contig's second kept record the seq of its first (a slot claimed twice), mode 1 gives its first kept record a seq past
// all_seq (a rank out of range).  Returns the contig, or -1 when no contig has two kept records.
int64_t emx_break_rank(int mode, int64_t *sz) {
    if (!g_be) return -1;
    const int64_t nar = std::min<int64_t>(g_ws.counters[CNT_AR], g_ws.ar_cap);
    for (int64_t r = 0; r < nar; r++) {
        const int32_t c = g_ws.ar_ctg[r];
        if (g_ws.ar_gen[r] != g_ws.all_gen[c]) continue;
        for (int64_t q = r + 1; q < nar; q++) {
            if (g_ws.ar_ctg[q] != c || g_ws.ar_gen[q] != g_ws.all_gen[c]) continue;
            if (mode == 0) g_ws.ar_seq[q] = g_ws.ar_seq[r];
            else g_ws.ar_seq[r] = g_ws.all_seq[c] + 5;
            g_pk.sized = false;
            if (pack_sizes(*g_be, g_ws, g_pk) != AASM_OK) return -1;
            for (int i = 0; i < 5; i++) sz[i] = g_pk.sizes[i];
            return c;
        }
    }
    return -1;
}
// the export of the last solve into caller (host) arrays sized by emx_solve_and_size
int emx_export(const aasm_dev_out *dst) {
    if (!g_be || !g_pk.sized) return AASM_E_INVAL;
    pack_export(*g_be, g_ws, g_pk, *dst);
    return g_be->failed() ? AASM_E_HIP : AASM_OK;
}
// fetch_results on the same workspace (release with emul_free_out)
int emx_fetch(aasm_batch_out *out) {
    if (!g_be) return AASM_E_INVAL;
    PipelineSizes ps;
    ps.C = g_ws.C; ps.R = g_ws.R; ps.S = g_ws.S; ps.VT = g_ws.VT; ps.ET = g_ws.ET;
    return fetch_results(*g_be, g_ws, ps, out);
}
}
