// tests/host_emul/read_cols_emul.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The device reader under AASM_READ_ROW_COLS (alignasm_amd/csrc/aasm_read.h: read_run with the names, name-offset and row-id
// kernels behind the pack) compiled for the HOST with one lane per block, so the CPU tier can check the resident row columns
// against rows_host_cols of the host reader's container.  One lane cannot see a fault between the lanes of the cooperative name
// copy: that is the GPU tier's.
//  * libaasm_emul_read_cols.so: emrc_parse(), aasm_paf_parse_device_rows' contract without a container, host arrays in the view
//    and the columns.  device_text = 1 is the AASM_READ_TEXT_ON_DEVICE form: the "device" text is a heap block of exactly len
//    bytes which the reader must use as it stands - every launch is checked to read that block, and the block to be unchanged.
//  * read_cols_emul_san FILE...: the same in a program built with the host address sanitizer.  Every "device" array is a heap
//    block of exactly its size - the text and `names` among them - so a load outside [0, len) or a store outside an array ends
//    the program.
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
struct EmuReadCols {
    int64_t max_blocks;                                              // (fewer blocks than items: the grid-stride loops)
    const void *own_text;                                            // device-text form: the block every launch must read
    bool text_ok = true;
    std::vector<void *> blocks;
    ~EmuReadCols() { for (void *p : blocks) std::free(p); }
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
        if (own_text && (const void *)a.text != own_text) text_ok = false;
        emul_launch(read_rows, kr, nthreads, 0, nblocks, max_blocks, [&](const KCtx &k) { run_read_body(kr, k, a); });
    }
};
struct EmuColsBatch { std::vector<void *> ptrs; };
int64_t g_slow_rows = 0, g_fallbacks = 0;
}  // namespace

extern "C" {
// aasm_paf_parse_device_rows(text, len, flags, ., NULL, up, dev_view, dev_cols) without a device: *view and *cols hold HOST arrays
// owned by *handle (emrc_free); max_blocks > 0 caps every grid; *names_bytes: the length of cols->names
int emrc_parse(const char *text, int64_t len, int flags, int64_t max_blocks, int device_text, void **handle, aasm_batch_in *view, aasm_row_cols *cols, int64_t *names_bytes) {
    if (handle) *handle = nullptr;
    if (!text || len < 0 || !handle || !view || !cols || !names_bytes) return AASM_E_INVAL;
    char *dev = nullptr;
    if (device_text) {                                               // (exactly the text: nothing readable behind it)
        dev = (char *)std::malloc(len ? (size_t)len : 1);
        std::memcpy(dev, text, (size_t)len);
    }
    ReadOut o;
    int rc;
    bool text_ok;
    {
        EmuReadCols be{max_blocks, dev};
        rc = read_run(be, dev ? dev : text, len, flags | AASM_READ_ROW_COLS | (dev ? AASM_READ_TEXT_ON_DEVICE : 0), nullptr, true, o);
        text_ok = be.text_ok;
    }
    if (dev && (!text_ok || std::memcmp(dev, text, (size_t)len) != 0)) rc = AASM_E_INTERNAL;   // the text was copied, or written
    std::free(dev);
    if (rc == AASM_OK) {
        g_slow_rows = o.slow_rows;
        EmuColsBatch *h = new EmuColsBatch();
        h->ptrs = {o.ctg_rec_off, o.qry_str, o.qry_end, o.ref_str, o.ref_end, o.qry_total, o.ref_chr, o.aln_fwd, o.map_qul, o.rec_rng_off, o.cs_text, o.rec_cs_off,
                   o.ref_total, o.mat_num, o.aln_len, o.row_index, o.cord_type, o.names, o.ctg_name_off, o.chr_name_off};
        std::memset(view, 0, sizeof *view);
        view->n_contigs = o.C; view->n_records = o.R; view->n_ranges = o.n_ranges;
        view->ctg_rec_off = o.ctg_rec_off; view->qry_str = o.qry_str; view->qry_end = o.qry_end; view->ref_str = o.ref_str; view->ref_end = o.ref_end;
        view->qry_total = o.qry_total; view->ref_chr = o.ref_chr; view->aln_fwd = o.aln_fwd; view->map_qul = o.map_qul; view->rec_rng_off = o.rec_rng_off;
        view->cs_text = o.cs_text; view->rec_cs_off = o.rec_cs_off;
        cols->n_chr = o.n_chr; cols->ref_total = o.ref_total; cols->mat_num = o.mat_num; cols->aln_len = o.aln_len; cols->row_index = o.row_index;
        cols->cord_type = o.cord_type; cols->names = o.names; cols->ctg_name_off = o.ctg_name_off; cols->chr_name_off = o.chr_name_off;
        *names_bytes = o.names_bytes;
        *handle = h;
        return AASM_OK;
    }
    if (rc < 0) return rc;
    g_fallbacks++;
    return read_host_verdict(text, len);
}
void emrc_free(void *handle) {
    EmuColsBatch *h = (EmuColsBatch *)handle;
    if (!h) return;
    for (void *p : h->ptrs) std::free(p);
    delete h;
}
int64_t emrc_counter(int which) { return which == 0 ? g_slow_rows : g_fallbacks; }
int64_t emrc_pack_lanes(void) { return AASM_READ_PACK_LANES; }
}

#if defined(AASM_EMUL_SAN_MAIN)
#include "emul_san.h"
// read_cols_emul_san FILE...: every file through the emulated reader with row columns, host text and "device" text, grids capped
// at 3 blocks as well as free.  Prints one line per run: the file's name, the entry's code, rows, reference names, bytes of names.
// The sanitizer ends the program at the first bad access, and reports a block nobody freed.
int main(int argc, char **argv) {
    for (int i = 1; i < argc; i++) {
        std::vector<char> data;
        if (!emul_san::read_bytes(argv[i], data)) return 2;
        char *text = emul_san::exact<char>(data.data(), (int64_t)data.size());   // (exactly the text: nothing readable behind it)
        for (int64_t cap : {(int64_t)0, (int64_t)3})
            for (int device_text : {0, 1}) {
                void *h = nullptr;
                aasm_batch_in v;
                aasm_row_cols c;
                int64_t nb = -1;
                const int rc = emrc_parse(text, (int64_t)data.size(), 0, cap, device_text, &h, &v, &c, &nb);
                std::printf("%s %d %lld %lld %lld\n", argv[i], rc, rc == AASM_OK ? (long long)v.n_records : -1ll, rc == AASM_OK ? (long long)c.n_chr : -1ll, (long long)nb);
                emrc_free(h);
            }
        std::free(text);
    }
    return 0;
}
#endif
