// tests/host_emul/alt_emul.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The --alt merge on the device (alignasm_amd/csrc/aasm_alt.h: alt_merge_run behind the reader's front) compiled for the HOST with
// one lane per block, so the CPU tier can check the merged batch and its row columns against the host route (aasm_paf_merge_alt_mem
// on the host reader's container).  One lane cannot see a fault between the lanes of the cooperative copies, nor a race of the
// atomic passes: those are the GPU tier's.
//  * libaasm_emul_alt.so: emalt_merge(), aasm_paf_merge_alt_device's contract on the arrays of a host container: the "resident"
//    batch is made of heap blocks of exactly the arrays' sizes, which the merge must leave as they are (checked after every call).
//    emalt_host_cols(): rows_host_cols of a container, the yardstick's row columns.
//  * alt_emul_san MAIN ALT BASELINE ...: the same in a program built with the host address sanitizer.  Every "device" array is a
//    heap block of exactly its size - the alt text and the resident arrays among them - so a load outside them or a store outside
//    an array ends the program.
#define AASM_HOST_EMUL 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../alignasm_amd/csrc/aasm_alt.h"
#include "../../alignasm_amd/csrc/aasm_rows.h"
#include "emul_launch.h"

using namespace aasm;

namespace {
AASM_EMUL_ROWS(read_rows, AASM_READ_KERNELS);
AASM_EMUL_ROWS(alt_rows, AASM_ALT_KERNELS);
struct EmuAlt {
    int64_t max_blocks;                                              // (fewer blocks than items: the grid-stride loops)
    std::vector<void *> blocks;
    ~EmuAlt() { for (void *p : blocks) std::free(p); }
    bool ok() const { return true; }
    int code() const { return AASM_E_NOMEM; }
    void *alloc(size_t n) { void *p = std::malloc(n ? n : 1); std::memset(p, 0xA5, n ? n : 1); blocks.push_back(p); return p; }   // (poisoned, as aasm_debug_poison does)
    void release(void *p) { keep(p); std::free(p); }
    void keep(void *p) { auto it = std::find(blocks.begin(), blocks.end(), p); if (it != blocks.end()) blocks.erase(it); }
    void h2d(void *d, const void *h, size_t n) { if (n) std::memcpy(d, h, n); }
    void d2h(void *h, const void *d, size_t n) { if (n) std::memcpy(h, d, n); }
    void fill32(void *p, int32_t v, int64_t count) { for (int64_t i = 0; i < count; i++) ((int32_t *)p)[i] = v; }
    template <class T> void scan(const T *in, int64_t n, int64_t *out) { int64_t s = 0; for (int64_t i = 0; i < n; i++) { out[i] = s; s += (int64_t)in[i]; } out[n] = s; }
    void scan_i32(const int32_t *in, int64_t n, int64_t *out) { scan(in, n, out); }
    void scan_u8(const uint8_t *in, int64_t n, int64_t *out) { scan(in, n, out); }
    void stage(const char *) {}
    void launch_read(int kr, int64_t nblocks, int nthreads, const ReadArgs &a) {
        emul_launch(read_rows, kr, nthreads, 0, nblocks, max_blocks, [&](const KCtx &k) { run_read_body(kr, k, a); });
    }
    void launch_alt(int ka, int64_t nblocks, int nthreads, const AltArgs &a) {
        emul_launch(alt_rows, ka, nthreads, 0, nblocks, max_blocks, [&](const KCtx &k) { run_alt_body(ka, k, a); });
    }
};
struct EmuAltBatch { std::vector<void *> ptrs; };
struct HostCols { RowsHostCols h; };
int64_t g_verdicts = 0, g_merges = 0;

// a heap block of exactly n bytes holding src[0, n)
void *exact(const void *src, size_t n, std::vector<std::pair<void *, std::vector<char>>> &made) {
    void *p = std::malloc(n ? n : 1);
    if (n) std::memcpy(p, src, n);
    made.emplace_back(p, std::vector<char>((const char *)src, (const char *)src + n));
    return p;
}
}  // namespace

extern "C" {
// aasm_paf_merge_alt_device(batch and columns of `paf`, alt, ...) without a device: *view and *cols hold HOST arrays owned by
// *handle (emalt_free); max_blocks > 0 caps every grid; *names_bytes: the length of cols->names.  AASM_E_INTERNAL: the merge wrote
// into one of its input arrays.
int emalt_merge(const aasm_paf *paf, const char *alt, int64_t alt_len, double baseline, int flags, int64_t max_blocks, void **handle, aasm_batch_in *view,
                aasm_row_cols *cols, int64_t *names_bytes) {
    if (handle) *handle = nullptr;
    if (!paf || !alt || alt_len < 0 || !handle || !view || !cols || !names_bytes || !paf->device_ranges) return AASM_E_INVAL;
    aasm_batch_in hv;
    if (aasm_paf_batch(paf, &hv) != AASM_OK || hv.rng_qry_l || !hv.cs_text) return AASM_E_INVAL;
    RowsHostCols hc;
    if (!rows_host_cols(*paf, 0, hv.n_contigs, hc)) return AASM_E_INVAL;
    const size_t C = (size_t)hv.n_contigs, R = (size_t)hv.n_records, T = (size_t)hv.rec_cs_off[R];
    std::vector<std::pair<void *, std::vector<char>>> made;
    aasm_batch_in in = hv;
    in.ctg_rec_off = (const int64_t *)exact(hv.ctg_rec_off, (C + 1) * 8, made);
    in.qry_str = (const int64_t *)exact(hv.qry_str, R * 8, made); in.qry_end = (const int64_t *)exact(hv.qry_end, R * 8, made);
    in.ref_str = (const int64_t *)exact(hv.ref_str, R * 8, made); in.ref_end = (const int64_t *)exact(hv.ref_end, R * 8, made);
    in.qry_total = (const int64_t *)exact(hv.qry_total, R * 8, made); in.ref_chr = (const int32_t *)exact(hv.ref_chr, R * 4, made);
    in.aln_fwd = (const uint8_t *)exact(hv.aln_fwd, R, made); in.map_qul = (const uint8_t *)exact(hv.map_qul, R, made);
    in.rec_rng_off = (const int64_t *)exact(hv.rec_rng_off, (R + 1) * 8, made); in.rec_cs_off = (const int64_t *)exact(hv.rec_cs_off, (R + 1) * 8, made);
    in.cs_text = (const char *)exact(hv.cs_text, T, made);
    aasm_row_cols ic;
    ic.n_chr = (int64_t)hc.chr_name_off.size() - 1;
    ic.ref_total = (const int64_t *)exact(hc.ref_total.data(), R * 8, made); ic.mat_num = (const int32_t *)exact(hc.mat_num.data(), R * 4, made);
    ic.aln_len = (const int32_t *)exact(hc.aln_len.data(), R * 4, made); ic.row_index = (const int32_t *)exact(hc.row_index.data(), R * 4, made);
    ic.cord_type = (const uint8_t *)exact(hc.cord_type.data(), R, made); ic.names = (const char *)exact(hc.names.data(), hc.names.size(), made);
    ic.ctg_name_off = (const int64_t *)exact(hc.ctg_name_off.data(), hc.ctg_name_off.size() * 8, made);
    ic.chr_name_off = (const int64_t *)exact(hc.chr_name_off.data(), hc.chr_name_off.size() * 8, made);
    char *text = (char *)std::malloc(alt_len ? (size_t)alt_len : 1);    // (exactly the text: nothing readable behind it)
    std::memcpy(text, alt, (size_t)alt_len);
    AltOut o;
    int rc;
    {
        EmuAlt be{max_blocks};
        rc = alt_merge_run(be, in, ic, text, alt_len, baseline, flags, o);
    }
    bool intact = true;
    for (auto &m : made) { intact = intact && (m.second.empty() || std::memcmp(m.first, m.second.data(), m.second.size()) == 0); std::free(m.first); }
    if (rc == AASM_OK) {
        if (!intact) { for (void *p : alt_out_arrays(o)) std::free(p); std::free(text); return AASM_E_INTERNAL; }
        EmuAltBatch *h = new EmuAltBatch();
        h->ptrs = alt_out_arrays(o);
        alt_out_views(o, *view, *cols);
        *names_bytes = o.names_bytes;
        *handle = h;
        g_merges++;
        std::free(text);
        return AASM_OK;
    }
    if (rc == AASM_ALT_DECLINED) { g_verdicts++; rc = alt_host_says(text, alt_len, o); }
    std::free(text);
    return intact ? rc : AASM_E_INTERNAL;
}
void emalt_free(void *handle) {
    EmuAltBatch *h = (EmuAltBatch *)handle;
    if (!h) return;
    for (void *p : h->ptrs) std::free(p);
    delete h;
}
// rows_host_cols(paf, 0, n_contigs): host arrays in *cols, owned by *handle (emalt_host_cols_free)
int emalt_host_cols(const aasm_paf *paf, void **handle, aasm_row_cols *cols) {
    if (!paf || !handle || !cols) return AASM_E_INVAL;
    HostCols *k = new HostCols();
    if (!rows_host_cols(*paf, 0, paf->n_contigs(), k->h)) { delete k; return AASM_E_INVAL; }
    cols->n_chr = (int64_t)k->h.chr_name_off.size() - 1;
    cols->ref_total = k->h.ref_total.data(); cols->mat_num = k->h.mat_num.data(); cols->aln_len = k->h.aln_len.data(); cols->row_index = k->h.row_index.data();
    cols->cord_type = k->h.cord_type.data(); cols->names = k->h.names.data(); cols->ctg_name_off = k->h.ctg_name_off.data(); cols->chr_name_off = k->h.chr_name_off.data();
    *handle = k;
    return AASM_OK;
}
void emalt_host_cols_free(void *handle) { delete (HostCols *)handle; }
int64_t emalt_counter(int which) { return which == 0 ? g_verdicts : g_merges; }
}

#if defined(AASM_EMUL_SAN_MAIN)
#include "emul_san.h"
// alt_emul_san MAIN ALT BASELINE ...: every triple through the emulated merge, under every combination of the two hooks, grids capped
// at 3 blocks as well as free.  Prints one line per run: the alt file's name, the flags, the entry's code, merged records, reference
// names, bytes of names.  The sanitizer ends the program at the first bad access, and reports a block nobody freed.
int main(int argc, char **argv) {
    for (int i = 1; i + 2 < argc; i += 3) {
        std::vector<char> main_text, alt;
        if (!emul_san::read_bytes(argv[i], main_text) || !emul_san::read_bytes(argv[i + 1], alt)) return 2;
        const double baseline = std::atof(argv[i + 2]);
        aasm_paf *paf = nullptr;
        if (aasm_paf_parse_mem_opts(main_text.data(), (int64_t)main_text.size(), AASM_READ_DEVICE_RANGES, &paf) != AASM_OK) return 2;
        for (int flags : {0, AASM_READ_H_WEAK_HASH, AASM_READ_H_FEW_BLOCKS, AASM_READ_H_WEAK_HASH | AASM_READ_H_FEW_BLOCKS})
            for (int64_t cap : {(int64_t)0, (int64_t)3}) {
                void *h = nullptr;
                aasm_batch_in v;
                aasm_row_cols c;
                int64_t nb = -1;
                const int rc = emalt_merge(paf, alt.empty() ? "" : alt.data(), (int64_t)alt.size(), baseline, flags, cap, &h, &v, &c, &nb);
                if (rc == AASM_E_INTERNAL) return 3;
                std::printf("%s %d %d %lld %lld %lld\n", argv[i + 1], flags, rc, rc == AASM_OK ? (long long)v.n_records : -1ll, rc == AASM_OK ? (long long)c.n_chr : -1ll, (long long)nb);
                emalt_free(h);
            }
        aasm_paf_free(paf);
    }
    return 0;
}
#endif
