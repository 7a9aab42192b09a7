// tests/host_emul/read_emul.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The device reader (alignasm_amd/csrc/aasm_read.h: the kernel bodies and their driver read_run) compiled for the HOST with one
// lane per block, together with the host codec (aasm_paf.cpp) it shares the slow path and the container with, so the CPU tier can
// check it against the I/O oracle and the host reader.
//  * libaasm_emul_read.so: emr_parse_device(), aasm_paf_parse_device's contract with host arrays in the view; the library's own
//    aasm_paf_batch / aasm_paf_to_text / aasm_paf_free / aasm_last_error serve the container it returns.
//  * read_emul_san FILE...: the same in a program built with the host address sanitizer.  Every "device" array is a heap block
//    of exactly its size - the text among them - so a read outside [0, len) ends the program.
#define AASM_HOST_EMUL 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../alignasm_amd/csrc/aasm_read.h"
#include "emul_launch.h"

using namespace aasm;

namespace {
AASM_EMUL_ROWS(read_rows, AASM_READ_KERNELS);
struct EmuRead {
    int64_t max_blocks;                                              // (fewer blocks than items: the grid-stride loops)
    std::vector<void *> blocks;
    ~EmuRead() { for (void *p : blocks) std::free(p); }
    bool ok() const { return true; }
    int code() const { return AASM_E_NOMEM; }
    void *alloc(size_t n) { void *p = std::malloc(n ? n : 1); blocks.push_back(p); return p; }
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
};
struct EmuBatch { std::vector<void *> ptrs; };
int64_t g_slow_rows = 0, g_fallbacks = 0;
}  // namespace

extern "C" {
// aasm_paf_parse_device without a device: *view holds HOST arrays owned by *handle (emr_free); max_blocks > 0 caps every grid
int emr_parse_device(const char *text, int64_t len, int flags, int64_t max_blocks, aasm_paf **paf_out, void **handle, aasm_batch_in *view) {
    if (paf_out) *paf_out = nullptr;
    if (handle) *handle = nullptr;
    if (!text || len < 0 || (handle == nullptr) != (view == nullptr) || (!paf_out && !handle)) return AASM_E_INVAL;
    aasm_paf *paf = paf_out ? new aasm_paf() : nullptr;
    ReadOut o;
    int rc;
    {
        EmuRead be{max_blocks, {}};
        rc = read_run(be, text, len, flags, paf, handle != nullptr, o);
    }
    if (rc == AASM_OK) {
        g_slow_rows = o.slow_rows;
        if (handle) {
            EmuBatch *h = new EmuBatch();
            h->ptrs = {o.ctg_rec_off, o.qry_str, o.qry_end, o.ref_str, o.ref_end, o.qry_total, o.ref_chr, o.aln_fwd, o.map_qul, o.rec_rng_off, o.cs_text, o.rec_cs_off};
            std::memset(view, 0, sizeof *view);
            view->n_contigs = o.C; view->n_records = o.R; view->n_ranges = o.n_ranges;
            view->ctg_rec_off = o.ctg_rec_off; view->qry_str = o.qry_str; view->qry_end = o.qry_end; view->ref_str = o.ref_str; view->ref_end = o.ref_end;
            view->qry_total = o.qry_total; view->ref_chr = o.ref_chr; view->aln_fwd = o.aln_fwd; view->map_qul = o.map_qul; view->rec_rng_off = o.rec_rng_off;
            view->cs_text = o.cs_text; view->rec_cs_off = o.rec_cs_off;
            *handle = h;
        }
        if (paf_out) *paf_out = paf;
        return AASM_OK;
    }
    delete paf;
    if (rc < 0) return rc;
    g_fallbacks++;
    return read_host_verdict(text, len);
}
void emr_free(void *handle) {
    EmuBatch *h = (EmuBatch *)handle;
    if (!h) return;
    for (void *p : h->ptrs) std::free(p);
    delete h;
}
int64_t emr_counter(int which) { return which == 0 ? g_slow_rows : g_fallbacks; }
int64_t emr_tile(void) { return AASM_READ_TILE; }
}

#if defined(AASM_EMUL_SAN_MAIN)
#include "emul_san.h"
// read_emul_san FILE...: every file through the emulated reader, container and batch, grids capped at 3 blocks as well as free.
// Prints one line per file: its name, the entry's code, the row count.  The sanitizer ends the program at the first bad access.
int main(int argc, char **argv) {
    for (int i = 1; i < argc; i++) {
        std::vector<char> data;
        if (!emul_san::read_bytes(argv[i], data)) return 2;
        char *text = emul_san::exact<char>(data.data(), (int64_t)data.size());   // (exactly the text: nothing readable behind it)
        for (int64_t cap : {(int64_t)0, (int64_t)3}) {
            aasm_paf *paf = nullptr;
            void *h = nullptr;
            aasm_batch_in v;
            const int rc = emr_parse_device(text, (int64_t)data.size(), 0, cap, &paf, &h, &v);
            std::printf("%s %d %lld\n", argv[i], rc, rc == AASM_OK ? (long long)v.n_records : -1ll);
            emr_free(h);
            aasm_paf_free(paf);
        }
        std::free(text);
    }
    return 0;
}
#endif
