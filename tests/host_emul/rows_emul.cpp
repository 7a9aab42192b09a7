// tests/host_emul/rows_emul.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The rows kernels (alignasm_amd/csrc/aasm_rows.h: kb_rows_len, kb_rows_fill, launched by rows_launch_len / rows_launch_fill)
// compiled for the HOST with one lane per block, so the CPU tier can check row lengths, offsets, digits, the irregular walk and
// the error contract against the oracle's files and the host writers.  One lane cannot see a fault between the lanes of the
// cooperative copy: that is the GPU tier's.
//  * libaasm_emul_rows.so: emw_rows_sizes() / emw_rows_format(), the entries' argument order with host arrays, and
//    emw_row_cols(): the row columns of a container as host arrays; emw_cut_pieces(): the device writer's piece cutter
//    (rows_cut_pieces) over a host array, with a record of what it fetched.
//  * rows_emul_san: the same bodies in a program built with the host address sanitizer, which formats every list into a heap
//    block of exactly its bytes and reads every record's tag from a private block that ends where the tag ends.
#define AASM_HOST_EMUL 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../alignasm_amd/csrc/aasm_rows.h"
#include "emul_launch.h"

using namespace aasm;

namespace {
AASM_EMUL_ROWS(rows_rows, AASM_ROWS_KERNELS);
struct EmuRows {
    int64_t max_blocks;                                              // (fewer blocks than chunks: the grid-stride loops)
    void launch_rows(int kw, int64_t nblocks, int nthreads, const RowsArgs &a) {
        emul_launch(rows_rows, kw, nthreads, 0, nblocks, max_blocks, [&](const KCtx &k) { run_rows_body(kw, k, a); });
    }
};
int sizes(const aasm_batch_in *in, const aasm_row_cols *cols, const aasm_out_sizes *sz, const aasm_dev_out *out, const aasm_dev_cuts *cuts,
          const aasm_dev_rows *ro, int64_t max_blocks, aasm_rows_info *info) {
    if (!in || !cols || !sz || !out || !cuts || !ro || !info || !in->cs_text || !in->rec_cs_off) return AASM_E_INVAL;
    RowsArgs a;
    if (!rows_args(*in, *cols, *sz, *out, *cuts, *ro, a)) return AASM_E_INVAL;
    int64_t words[RW_WORDS] = {0, AASM_ROWS_NO_KEY};
    a.words = words;
    EmuRows be{max_blocks};
    rows_launch_len(be, a, 0);
    for (int l = 0; l < 3; l++) {                                    // the scan, in place: lengths at [i + 1] -> offsets
        int64_t *o = a.row_off[l];
        if (!o) { if (a.c.n[l]) return AASM_E_INVAL; info->bytes[l] = 0; continue; }
        o[0] = 0;
        for (int64_t i = 0; i < a.c.n[l]; i++) o[i + 1] += o[i];
        info->bytes[l] = o[a.c.n[l]];
    }
    rows_info_of(words, *info);
    return AASM_OK;
}
int format(const aasm_batch_in *in, const aasm_row_cols *cols, const aasm_out_sizes *sz, const aasm_dev_out *out, const aasm_dev_cuts *cuts,
           const aasm_dev_rows *ro, const aasm_rows_info *info, int list, int64_t e0, int64_t e1, char *text, int64_t max_blocks) {
    if (!in || !cols || !sz || !out || !cuts || !ro || !info || !in->cs_text || !in->rec_cs_off) return AASM_E_INVAL;
    RowsArgs a;
    if (!rows_args(*in, *cols, *sz, *out, *cuts, *ro, a)) return AASM_E_INVAL;
    if (rows_format_refusal(a, *info, list, e0, e1)) return AASM_E_INVAL;
    for (int l = 0; l < 3; l++)                                      // info is what the sizes call left in these arrays
        if ((a.c.n[l] > 0 && (!a.row_off[l] || a.row_off[l][a.c.n[l]] != info->bytes[l])) || (a.c.n[l] == 0 && info->bytes[l] != 0)) return AASM_E_INVAL;
    if (e1 > e0 && !text) return AASM_E_INVAL;
    EmuRows be{max_blocks};
    rows_launch_fill(be, a, list, e0, e1, text, 0);
    return AASM_OK;
}
}  // namespace

extern "C" {
// aasm_rows_sizes_device / aasm_rows_format_device on host arrays; max_blocks > 0 caps the grids
int emw_rows_sizes(const aasm_batch_in *in, const aasm_row_cols *cols, const aasm_out_sizes *sz, const aasm_dev_out *out, const aasm_dev_cuts *cuts,
                   const aasm_dev_rows *ro, int64_t max_blocks, aasm_rows_info *info) {
    return sizes(in, cols, sz, out, cuts, ro, max_blocks, info);
}
int emw_rows_format(const aasm_batch_in *in, const aasm_row_cols *cols, const aasm_out_sizes *sz, const aasm_dev_out *out, const aasm_dev_cuts *cuts,
                    const aasm_dev_rows *ro, const aasm_rows_info *info, int list, int64_t e0, int64_t e1, char *text, int64_t max_blocks) {
    return format(in, cols, sz, out, cuts, ro, info, list, e0, e1, text, max_blocks);
}
int64_t emw_chunk(void) { return AASM_ROWS_CHUNK; }
int64_t emw_len_chunk(void) { return AASM_CUT_CHUNK; }
// aasm_paf_upload_rows without the upload: the columns of contigs [c0, c1) of a container as host arrays the handle owns
struct emw_cols { RowsHostCols h; };
int emw_row_cols(const aasm_paf *paf, int64_t c0, int64_t c1, emw_cols **keep, aasm_row_cols *cols) {
    if (!paf || !keep || !cols) return AASM_E_INVAL;
    emw_cols *k = new emw_cols();
    if (!rows_host_cols(*paf, c0, c1, k->h)) { delete k; return AASM_E_INVAL; }
    cols->n_chr = (int64_t)k->h.chr_name_off.size() - 1;
    cols->ref_total = k->h.ref_total.data(); cols->mat_num = k->h.mat_num.data(); cols->aln_len = k->h.aln_len.data();
    cols->row_index = k->h.row_index.data(); cols->cord_type = k->h.cord_type.data(); cols->names = k->h.names.data();
    cols->ctg_name_off = k->h.ctg_name_off.data(); cols->chr_name_off = k->h.chr_name_off.data();
    *keep = k;
    return AASM_OK;
}
void emw_row_cols_free(emw_cols *k) { delete k; }
// rows_cut_pieces (aasm_writer_append_device's pieces) over a host array of n + 1 offsets: the pieces as {list, e0, e1, b0, b1}
// into out[5 * cap] -> their number, -1: more than cap.  The fetches of the last call stay behind for emw_cut_fetches.
static std::vector<int64_t> g_fetches;                               // {first, stride, count} per fetch
int64_t emw_cut_pieces(const int64_t *off, int64_t n, int64_t total, int list, int64_t limit, int64_t *out, int64_t cap) {
    g_fetches.clear();
    std::vector<RowsPiece> pieces;
    auto fetch = [&](int64_t first, int64_t stride, int64_t count, int64_t *dst) {
        g_fetches.insert(g_fetches.end(), {first, stride, count});
        for (int64_t k = 0; k < count; k++) dst[k] = off[first + k * stride];
        return true;
    };
    if (!rows_cut_pieces(fetch, n, total, list, limit, pieces)) return -2;
    if ((int64_t)pieces.size() > cap) return -1;
    for (size_t k = 0; k < pieces.size(); k++) {
        const RowsPiece &p = pieces[k];
        const int64_t v[5] = {p.list, p.e0, p.e1, p.b0, p.b1};
        std::memcpy(out + 5 * k, v, sizeof v);
    }
    return (int64_t)pieces.size();
}
int64_t emw_cut_fetches(int64_t *out, int64_t cap) {                 // -> the fetches of the last emw_cut_pieces call, 3 words each
    const int64_t m = (int64_t)g_fetches.size() / 3;
    for (int64_t k = 0; k < m && k < cap; k++) std::memcpy(out + 3 * k, g_fetches.data() + 3 * k, 24);
    return m;
}
int64_t emw_sample(void) { return AASM_ROWS_SAMPLE; }
}

#if defined(AASM_EMUL_SAN_MAIN)
#include "emul_san.h"
// rows_emul_san IN OUT.  IN, in 8-byte words: {C, R, n_chr, NM, NA, NP, NE, names bytes, text bytes}, then per record qry_total,
// qry_str, qry_end, ref_total, rec_cs_off[R + 1], ctg_rec_off[C + 1], ctg_name_off[C + 1], chr_name_off[n_chr + 1], main_off[C + 1],
// alt_off[C + 1], all_path_off[C + 1], all_elem_off[NP + 1], the NM + NA + NE elements (40 bytes each), their plans (48 bytes
// each), per record ref_chr, mat_num, aln_len, row_index (int32; the four arrays padded to whole words), aln_fwd, map_qul, cord_type
// (bytes), the names and the cs text (padded to whole words).  OUT: the three lists' text, back to back.
// Every list is formatted into a heap block of EXACTLY its bytes, and every record's tag lies in a private block that ends where
// the tag ends and starts at the tag's own alignment inside an 8-byte word: the sanitizer ends the program at the first byte
// read behind a tag or written outside the text.
int main(int argc, char **argv) {
    std::vector<int64_t> raw;
    if (argc != 3 || !emul_san::read_words(argv[1], raw) || raw.size() < 9) return 2;
    const int64_t C = raw[0], R = raw[1], NCHR = raw[2], NM = raw[3], NA = raw[4], NP = raw[5], NE = raw[6], NB = raw[7], TB = raw[8];
    const int64_t *p = raw.data() + 9;
    auto take = [&](int64_t n) { const int64_t *q = p; p += n; return q; };
    const int64_t *qtot = take(R), *qs = take(R), *qe = take(R), *rtot = take(R), *cs_off = take(R + 1), *rec_off = take(C + 1), *ctg_name_off = take(C + 1),
                  *chr_name_off = take(NCHR + 1), *main_off = take(C + 1), *alt_off = take(C + 1), *path_off = take(C + 1), *elem_off = take(NP + 1);
    const aasm_out_elem *el = (const aasm_out_elem *)take((NM + NA + NE) * 5);
    const aasm_cut_plan *pl = (const aasm_cut_plan *)take((NM + NA + NE) * 6);
    const int64_t r4 = (R * 4 + 7) / 8;
    const int32_t *ref_chr = (const int32_t *)take(r4), *mat = (const int32_t *)take(r4), *aln = (const int32_t *)take(r4), *row_index = (const int32_t *)take(r4);
    const uint8_t *fwd = (const uint8_t *)p, *mq = fwd + R, *cord = mq + R;
    p += (3 * R + 7) / 8;
    const char *names = (const char *)take((NB + 7) / 8), *text = (const char *)take((TB + 7) / 8);
    if (p > raw.data() + raw.size()) return 2;
    // the tags, each in a block of its own
    std::vector<char *> blocks((size_t)R);
    for (int64_t r = 0; r < R; r++) {
        const int64_t len = cs_off[r + 1] - cs_off[r], mis = cs_off[r] & 7;
        blocks[(size_t)r] = emul_san::block<char>(mis + len);
        std::memcpy(blocks[(size_t)r] + mis, text + cs_off[r], (size_t)len);
    }
    // A table of R + 1 offsets cannot hold R unrelated blocks, so the batch is rebuilt with 2 R records: record 2 r is the real one,
    // its tag at [rec_cs_off[2 r], rec_cs_off[2 r + 1]) relative to the first block, record 2 r + 1 a spacer no element names.
    std::vector<int64_t> x_cs_off((size_t)(2 * R) + 1, 0), x_rec_off((size_t)C + 1), x_qtot((size_t)(2 * R)), x_qs((size_t)(2 * R)), x_qe((size_t)(2 * R)), x_rtot((size_t)(2 * R));
    std::vector<int32_t> x_chr((size_t)(2 * R)), x_mat((size_t)(2 * R)), x_aln((size_t)(2 * R)), x_idx((size_t)(2 * R));
    std::vector<uint8_t> x_fwd((size_t)(2 * R)), x_mq((size_t)(2 * R)), x_cord((size_t)(2 * R));
    const char *origin = R ? blocks[0] : "";
    for (int64_t r = 0; r < R; r++) {
        const int64_t len = cs_off[r + 1] - cs_off[r], mis = cs_off[r] & 7;
        x_cs_off[(size_t)(2 * r)] = (blocks[(size_t)r] + mis) - origin; x_cs_off[(size_t)(2 * r) + 1] = x_cs_off[(size_t)(2 * r)] + len;
        for (int h = 0; h < 2; h++) {
            const size_t k = (size_t)(2 * r + h);
            x_qtot[k] = qtot[r]; x_qs[k] = qs[r]; x_qe[k] = qe[r]; x_rtot[k] = rtot[r]; x_chr[k] = ref_chr[r]; x_mat[k] = mat[r]; x_aln[k] = aln[r];
            x_idx[k] = row_index[r]; x_fwd[k] = fwd[r]; x_mq[k] = mq[r]; x_cord[k] = cord[r];
        }
    }
    if (R) x_cs_off[(size_t)(2 * R)] = x_cs_off[(size_t)(2 * R) - 1];
    for (int64_t c = 0; c <= C; c++) x_rec_off[(size_t)c] = 2 * rec_off[c];
    std::vector<aasm_out_elem> x_el(el, el + NM + NA + NE);
    for (aasm_out_elem &e : x_el) if (e.ctg_index >= 0) e.ctg_index *= 2;
    aasm_batch_in in;
    std::memset(&in, 0, sizeof in);
    in.n_contigs = C; in.n_records = 2 * R; in.ctg_rec_off = x_rec_off.data(); in.qry_str = x_qs.data(); in.qry_end = x_qe.data(); in.qry_total = x_qtot.data();
    in.ref_chr = x_chr.data(); in.aln_fwd = x_fwd.data(); in.map_qul = x_mq.data(); in.cs_text = origin; in.rec_cs_off = x_cs_off.data();
    aasm_row_cols cols;
    cols.n_chr = NCHR; cols.ref_total = x_rtot.data(); cols.mat_num = x_mat.data(); cols.aln_len = x_aln.data(); cols.row_index = x_idx.data();
    cols.cord_type = x_cord.data(); cols.names = names; cols.ctg_name_off = ctg_name_off; cols.chr_name_off = chr_name_off;
    aasm_dev_out o;
    std::memset(&o, 0, sizeof o);
    o.main_off = (int64_t *)main_off; o.alt_off = (int64_t *)alt_off; o.all_path_off = (int64_t *)path_off; o.all_elem_off = (int64_t *)elem_off;
    o.main_elems = x_el.data(); o.alt_elems = x_el.data() + NM; o.all_elems = x_el.data() + NM + NA;
    const aasm_out_sizes sz{C, NM, NA, NP, NE};
    const aasm_dev_cuts d{(aasm_cut_plan *)pl, (aasm_cut_plan *)pl + NM, (aasm_cut_plan *)pl + NM + NA};
    const int64_t n[3] = {NM, NA, NE};
    int64_t *ro[3];
    for (int l = 0; l < 3; l++) ro[l] = emul_san::block<int64_t>(n[l] + 1);               // (exactly n + 1 offsets)
    const aasm_dev_rows rows{ro[0], ro[1], ro[2]};
    aasm_rows_info info;
    if (sizes(&in, &cols, &sz, &o, &d, &rows, 0, &info) != AASM_OK) return 3;
    if (info.n_flagged != 0) return 4;
    std::vector<char> lists;
    for (int l = 0; l < 3; l++) {
        char *t = emul_san::block<char>(info.bytes[l]);              // (exactly the list's bytes)
        // in two ranges, so that a range's first byte is not the block's
        const int64_t mid = n[l] / 2;
        if (format(&in, &cols, &sz, &o, &d, &rows, &info, l, 0, mid, t, 0) != AASM_OK) return 5;
        if (format(&in, &cols, &sz, &o, &d, &rows, &info, l, mid, n[l], t + (ro[l][mid] - ro[l][0]), 3) != AASM_OK) return 5;
        lists.insert(lists.end(), t, t + info.bytes[l]);
        std::free(t);
    }
    for (int l = 0; l < 3; l++) std::free(ro[l]);
    for (char *b : blocks) std::free(b);
    return emul_san::write_bytes(argv[2], lists.data(), lists.size()) ? 0 : 2;
}
#endif
