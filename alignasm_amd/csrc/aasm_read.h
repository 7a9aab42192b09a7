// aasm_read.h -- the device reader (aasm_paf_parse_device): kernel bodies, kernel table, launches, host driver.
//
// The reader of alignasm.cpp:76-183 on the text as it lies in device memory: what the host reader's two passes do (read_pass1,
// read_pass2 in aasm_paf.cpp) as six launches and three scans, so that a resident batch in the cs form (cs_text / rec_cs_off, no
// rng_*) comes out without a host pass over the text.
//   row starts  a wave takes a tile of AASM_READ_TILE bytes, sixteen bytes per lane and load; byte p starts a row iff the byte
//               before it is a line feed (or p == 0), text[p] is none, and the line is not a lone carriage return.  Counts per
//               tile are scanned; the second pass writes row_start[] in order (wave prefix of the lanes' popcounts).
//   rows        one lane per row (K0's precedent, aasm_kernels.h kb_cs_ranges: eight bytes per load): the twelve columns, the
//               nine numbers on the fast path of fast_i64 ([-] and 1 - 18 digits), the first tag that starts "cs:Z:", its ':'
//               count, the spans of both names and a hash of the reference name.  A row that is none (columns, tag, length)
//               lowers the first-fault word; a row with a number off the fast path goes on the slow list, which the HOST
//               resolves with its own parse_row (strtoll's leniency stays in one place).
//   heads       a lane per row compares both names with the row before: contig heads (scanned into contig numbers) and the
//               rows whose reference name changes.
//   groups      heads scatter ctg_rec_off and the contig names' spans; rows with a changed reference name go to a hash table:
//               slot = {owner row (its name is the key), lowest row}, matched by hash, length, bytes; linear probing.
//   ref ids     the table's entries, a few, are listed, ordered by first row on the host and numbered; every row looks its
//               name up and takes the number: chr_map's first-appearance order (alignasm.cpp:119-123).
//   pack        tag lengths scanned into rec_cs_off, ':' counts into rec_rng_off; sixteen lanes per tag copy it into cs_text.
//   row columns (AASM_READ_ROW_COLS) what an output row prints beyond the batch stays resident as aasm_row_cols: the three numeric
//               columns as parsed, row_index / cord_type, and `names` - contig-name lengths scanned into ctg_name_off, the
//               reference names' offsets made on the host from the few table entries, sixteen lanes per name copying it.
// No load touches a byte outside [0, len): wide loads are taken only where their bytes are inside the text.
// The driver (read_run) is shared by the product backend (aasm_gpu.hip) and the 1-lane host emulation (tests/host_emul/read_emul.cpp).
#pragma once
#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "aasm_dev.h"
#include "aasm_paf.hpp"

namespace aasm {

#define AASM_READ_TILE 16384
#define AASM_READ_PACK_LANES (AASM_WAVE >= 16 ? 16 : 1)
enum { RW_FAULT = 0, RW_SLOW, RW_NEW, RW_CHR, RW_N };               // ReadArgs::words: first bad row, slow rows, rows with a changed reference name, table entries

struct ReadArgs {
    const uint8_t *text;
    int64_t len, n_tiles, R;
    int32_t weak_hash;                   // AASM_READ_H_WEAK_HASH
    int32_t n_chr;
    int32_t *tile_cnt;                   // [n_tiles]
    const int64_t *tile_off;             // [n_tiles + 1]
    int64_t *row_start;                  // [R]
    int64_t *qs, *qe, *rs, *re, *qtot, *rtot;
    int32_t *mat, *aln, *ref_chr;
    int64_t *aln64;                      // [R] column 11 as a full 64-bit value, or nullptr (the reader): the --alt merge's ratio
    uint8_t *fwd, *mq;
    int64_t *tag_start, *rn_start;       // [R] the tag and the reference name in the text
    int32_t *tag_len, *n_colon, *qn_len, *rn_len;
    uint64_t *rn_hash;
    int32_t *words;                      // [RW_N]
    int32_t *slow_row;                   // [R]
    uint8_t *head, *cnew;                // [R]
    const int64_t *head_off;             // [R + 1] contig of a row
    int64_t *ctg_rec_off, *ctg_pos;      // [C + 1], [C]
    int32_t *ctg_len;                    // [C]
    int32_t *tab_owner, *tab_min;        // [tab_mask + 1]
    int64_t tab_mask;
    int64_t *chr_info;                   // {first row, name start, name length} per table entry
    const int32_t *chr_sorted;           // [n_chr] the entries' first rows, ascending
    const int64_t *cs_off;               // [R + 1]
    char *cs_text;
    // AASM_READ_ROW_COLS
    int64_t C;
    const int64_t *ctg_name_off;         // [C + 1] into names
    const int64_t *chr_name_off;         // [n_chr + 1] into names, chr_name_off[0] = ctg_name_off[C]
    const int64_t *chr_pos;              // [n_chr] the reference names in the text, in first-appearance order
    char *names;
    int32_t *row_index;                  // [R]
    uint8_t *cord_type;                  // [R]
};

// the row starts among the bytes [o, o + 16) of the text, bit t for byte o + t (o a multiple of 16, o < len)
AASM_DEV uint32_t read_chunk_starts(const ReadArgs &a, int64_t o) {
    const int n = (int)(a.len - o < 16 ? a.len - o : 16);
    uint64_t w[2] = {0, 0};
    if (n == 16) {
#if defined(AASM_HOST_EMUL)
        std::memcpy(w, a.text + o, 16);
#else
        const I4 q = *(const I4 *)(a.text + o);                     // (the text's base is 256-byte aligned)
        w[0] = mk64(q.x, q.y); w[1] = mk64(q.z, q.w);
#endif
    } else
        for (int t = 0; t < n; t++) w[t >> 3] |= (uint64_t)a.text[o + t] << (8 * (t & 7));
    int prev = o > 0 ? a.text[o - 1] : '\n';
    const int next = o + n < a.len ? a.text[o + n] : '\n';           // (the end of the text ends a line)
    uint32_t m = 0;
    AASM_UNROLL
    for (int t = 0; t < 16; t++) {
        if (t < n) {
            const int c = (int)((w[t >> 3] >> (8 * (t & 7))) & 0xff);
            const int nx = t + 1 < n ? (int)((w[(t + 1) >> 3] >> (8 * ((t + 1) & 7))) & 0xff) : next;
            if (prev == '\n' && c != '\n' && !(c == '\r' && nx == '\n')) m |= 1u << t;
            prev = c;
        }
    }
    return m;
}
AASM_DEV int64_t read_tile_chunks(const ReadArgs &a, int64_t tile) {
    const int64_t t0 = tile * AASM_READ_TILE, t1 = t0 + AASM_READ_TILE < a.len ? t0 + AASM_READ_TILE : a.len;
    return (t1 - t0 + 15) >> 4;
}
// A wave per tile (grid-stride): the tile's row count
AASM_DEV void kb_read_count(const KCtx &k, const ReadArgs &a) {
    for (int64_t tile = k.bid; tile < a.n_tiles; tile += k.nblocks) {
        const int64_t nch = read_tile_chunks(a, tile), t0 = tile * AASM_READ_TILE;
        int64_t cnt = 0;
        for (int64_t c = k.tid; c < nch; c += k.nthreads) cnt += popc64(read_chunk_starts(a, t0 + c * 16));
        cnt = wave_sum(cnt);
        if (k.lane == 0) a.tile_cnt[tile] = (int32_t)cnt;
    }
}
// ... and its row starts, in text order, from tile_off[tile] on
AASM_DEV void kb_read_starts(const KCtx &k, const ReadArgs &a) {
    for (int64_t tile = k.bid; tile < a.n_tiles; tile += k.nblocks) {
        const int64_t nch = read_tile_chunks(a, tile), t0 = tile * AASM_READ_TILE;
        int64_t base = a.tile_off[tile];
        for (int64_t c0 = 0; c0 < nch; c0 += k.nthreads) {
            const int64_t c = c0 + k.tid;
            uint32_t m = c < nch ? read_chunk_starts(a, t0 + c * 16) : 0u;
            const int n = popc64(m), incl = wave_incl_add(n);
            int64_t w = base + incl - n;
            while (m) { a.row_start[w++] = t0 + c * 16 + (ffs64(m) - 1); m &= m - 1; }
            base += wave_bcast(incl, AASM_WAVE - 1);
        }
    }
}

#define AASM_READ_HASH0 0xcbf29ce484222325ull                       // FNV-1a
#define AASM_READ_HASH_MUL 0x100000001b3ull
// Row i: parse_row + record_of (aasm_paf.cpp) for a lane.  Columns are counted by their tabs; a numeric field is taken while it
// is [-]digits (at most 18 of them), anything else sends the row to the slow list.
AASM_DEV void read_row_lane(const ReadArgs &a, int64_t i) {
    const uint8_t *tx = a.text;
    const int64_t len = a.len, p0 = a.row_start[i];
    int64_t v_qtot = 0, v_qs = 0, v_qe = 0, v_rtot = 0, v_rs = 0, v_re = 0, v_mat = 0, v_aln = 0, v_mq = 0;
    int col = 0;                                                     // the open field: its column, first byte, number state
    int64_t fs = p0, val = 0;
    int nd = 0;
    bool neg = false, fbad = false, slow = false, fwd = false, found = false;
    int64_t rn_s = p0, tag_s = p0, tag_l = 0, rn_l = 0, qn_l = 0;
    uint64_t h = AASM_READ_HASH0;
    int tm = 0;                                                      // bytes of "cs:Z:" the open tag has matched
    int32_t colons = 0, tag_colons = 0;
    const uint64_t pat = (uint64_t)'c' | (uint64_t)'s' << 8 | (uint64_t)':' << 16 | (uint64_t)'Z' << 24 | (uint64_t)':' << 32;
    auto close_field = [&](int64_t q) {                              // the open field is [fs, q)
        const int64_t v = neg ? -val : val;
        const bool num_ok = nd >= 1 && nd <= 18 && !fbad;
        switch (col) {
            case 0: qn_l = q - fs; break;
            case 1: v_qtot = v; slow |= !num_ok; break;
            case 2: v_qs = v; slow |= !num_ok; break;
            case 3: v_qe = v; slow |= !num_ok; break;
            case 4: break;
            case 5: rn_s = fs; rn_l = q - fs; break;
            case 6: v_rtot = v; slow |= !num_ok; break;
            case 7: v_rs = v; slow |= !num_ok; break;
            case 8: v_re = v; slow |= !num_ok; break;
            case 9: v_mat = v; slow |= !num_ok; break;
            case 10: v_aln = v; slow |= !num_ok; break;
            case 11: v_mq = v; slow |= !num_ok; break;
            default:
                if (!found && tm == 5) { found = true; tag_s = fs; tag_l = q - fs; tag_colons = colons; }
        }
    };
    int64_t end = len;
    bool open = true;
    for (int64_t pos = p0; pos < len && open; ) {
        int nb;
        uint64_t wd = cs_next_word(tx, pos, len, nb);                // the next <= 8 bytes, first byte lowest; inside [0, len)
        for (int t = 0; t < nb; t++) {
            const int c = (int)(wd & 0xff);
            wd >>= 8;
            const int64_t q = pos + t;
            bool eol = c == '\n';
            if (c == '\r') eol = q + 1 == len || tx[q + 1] == '\n';  // one trailing carriage return is no part of the row
            if (eol || c == '\t') {
                close_field(q);
                if (eol) { end = q; open = false; break; }
                if (col < 13) col++;
                fs = q + 1; val = 0; nd = 0; neg = false; fbad = false; tm = 0; colons = 0;
                continue;
            }
            const int64_t kf = q - fs;
            if (col >= 12) {
                if (!found) {
                    if (kf < 5) { if (tm == (int)kf && c == (int)((pat >> (8 * kf)) & 0xff)) tm++; }
                    else if (c == ':') colons++;
                }
            } else if (col == 5) h = (h ^ (uint64_t)c) * AASM_READ_HASH_MUL;
            else if (col == 4) { if (kf == 0) fwd = c == '+'; }
            else if (col != 0) {
                const unsigned dg = (unsigned)(c - '0');
                if (kf == 0 && c == '-') neg = true;
                else if (dg > 9u) fbad = true;
                else if (++nd <= 18) val = val * 10 + (int64_t)dg;
            }
        }
        pos += nb;
    }
    if (open) close_field(len);                                      // the last row of a text without a final line feed
    if (col < 11 || !found || end - p0 > INT32_MAX) atomic_min_i32(&a.words[RW_FAULT], (int32_t)i);
    if (slow) a.slow_row[atomic_add(&a.words[RW_SLOW], (int32_t)1)] = (int32_t)i;
    v_qe -= 1; v_re -= 1;                                            // closed intervals, the reference span in query order (:141-159)
    a.qs[i] = v_qs; a.qe[i] = v_qe; a.rs[i] = fwd ? v_rs : v_re; a.re[i] = fwd ? v_re : v_rs;
    a.qtot[i] = v_qtot; a.rtot[i] = v_rtot; a.mat[i] = (int32_t)v_mat; a.aln[i] = (int32_t)v_aln;
    if (a.aln64) a.aln64[i] = v_aln;
    a.fwd[i] = fwd ? 1 : 0; a.mq[i] = (uint8_t)v_mq;
    a.tag_start[i] = tag_s; a.tag_len[i] = (int32_t)tag_l; a.n_colon[i] = tag_colons;
    a.qn_len[i] = (int32_t)qn_l; a.rn_start[i] = rn_s; a.rn_len[i] = (int32_t)rn_l;
    a.rn_hash[i] = a.weak_hash ? (uint64_t)(rn_l & 3) : h;
}
AASM_DEV void kb_read_rows(const KCtx &k, const ReadArgs &a) {
    for (int64_t i = k.bid * k.nthreads + k.tid; i < a.R; i += k.nblocks * k.nthreads) read_row_lane(a, i);
}

AASM_DEV bool read_same_bytes(const uint8_t *tx, int64_t x, int64_t y, int32_t n) {
    for (int32_t t = 0; t < n; t++) if (tx[x + t] != tx[y + t]) return false;
    return true;
}
AASM_DEV bool read_same_ref(const ReadArgs &a, int64_t i, int64_t j) {
    return a.rn_len[i] == a.rn_len[j] && a.rn_hash[i] == a.rn_hash[j] && read_same_bytes(a.text, a.rn_start[i], a.rn_start[j], a.rn_len[i]);
}
// Row i against row i - 1: a new contig (alignasm.cpp:125-133)?  another reference name?
AASM_DEV void kb_read_heads(const KCtx &k, const ReadArgs &a) {
    for (int64_t i = k.bid * k.nthreads + k.tid; i < a.R; i += k.nblocks * k.nthreads) {
        const bool head = i == 0 || a.qn_len[i] != a.qn_len[i - 1] || !read_same_bytes(a.text, a.row_start[i], a.row_start[i - 1], a.qn_len[i]);
        const bool cnew = i == 0 || !read_same_ref(a, i, i - 1);
        a.head[i] = head ? 1 : 0; a.cnew[i] = cnew ? 1 : 0;
        if (cnew) atomic_add(&a.words[RW_NEW], (int32_t)1);
    }
}
// the slot of row i's reference name; claim: an empty slot met on the way becomes the name's
AASM_DEV int64_t read_ref_slot(const ReadArgs &a, int64_t i, bool claim) {
    int64_t s = (int64_t)(a.rn_hash[i] * 0x9e3779b97f4a7c15ull >> 20) & a.tab_mask;
    for (int64_t n = 0; n <= a.tab_mask; n++, s = (s + 1) & a.tab_mask) {
        int32_t o = a.tab_owner[s];
        if (o < 0) {
            if (!claim) return -1;
            o = atomic_cas_i32(&a.tab_owner[s], -1, (int32_t)i);
            if (o < 0) o = (int32_t)i;
        }
        if (o == (int32_t)i || read_same_ref(a, i, o)) return s;
    }
    return -1;
}
// Heads write their contig's first row and name span; rows with a changed reference name enter the table.
AASM_DEV void kb_read_groups(const KCtx &k, const ReadArgs &a) {
    for (int64_t i = k.bid * k.nthreads + k.tid; i < a.R; i += k.nblocks * k.nthreads) {
        if (a.head[i]) {
            const int64_t c = a.head_off[i];
            a.ctg_rec_off[c] = i; a.ctg_pos[c] = a.row_start[i]; a.ctg_len[c] = a.qn_len[i];
        }
        if (i == 0) a.ctg_rec_off[a.head_off[a.R]] = a.R;
        if (a.cnew[i]) {
            const int64_t s = read_ref_slot(a, i, true);
            if (s >= 0) atomic_min_i32(&a.tab_min[s], (int32_t)i);
        }
    }
}
AASM_DEV void kb_read_chr_list(const KCtx &k, const ReadArgs &a) {
    for (int64_t s = k.bid * k.nthreads + k.tid; s <= a.tab_mask; s += k.nblocks * k.nthreads)
        if (a.tab_owner[s] >= 0) {
            const int64_t j = atomic_add(&a.words[RW_CHR], (int32_t)1), r = a.tab_min[s];
            a.chr_info[3 * j] = r; a.chr_info[3 * j + 1] = a.rn_start[r]; a.chr_info[3 * j + 2] = a.rn_len[r];
        }
}
// ref_chr[i]: how many names appeared before the first row of row i's name
AASM_DEV void kb_read_ref_ids(const KCtx &k, const ReadArgs &a) {
    for (int64_t i = k.bid * k.nthreads + k.tid; i < a.R; i += k.nblocks * k.nthreads) {
        const int64_t s = read_ref_slot(a, i, false);
        const int32_t first = s >= 0 ? a.tab_min[s] : 0;
        int32_t lo = 0, hi = a.n_chr;
        while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if (a.chr_sorted[mid] < first) lo = mid + 1; else hi = mid; }
        a.ref_chr[i] = lo;
    }
}
AASM_DEV void read_copy8(char *dst, const uint8_t *src) { uint64_t w; __builtin_memcpy(&w, src, 8); __builtin_memcpy(dst, &w, 8); }
// AASM_READ_PACK_LANES lanes per tag: eight bytes per lane and step where eight are left in the tag, then the last bytes one by one
AASM_DEV void kb_read_pack(const KCtx &k, const ReadArgs &a) {
    const int G = AASM_READ_PACK_LANES, gl = k.tid % G;
    const int64_t per_block = k.nthreads / G;
    for (int64_t r = k.bid * per_block + k.tid / G; r < a.R; r += k.nblocks * per_block) {
        const uint8_t *src = a.text + a.tag_start[r];
        char *dst = a.cs_text + a.cs_off[r];
        const int64_t n = a.tag_len[r];
        for (int64_t o = (int64_t)gl * 8; o + 8 <= n; o += G * 8) read_copy8(dst + o, src + o);
        for (int64_t o = (n & ~(int64_t)7) + gl; o < n; o += G) dst[o] = (char)src[o];
    }
}
// AASM_READ_PACK_LANES lanes per name, contig names first, then the reference names: kb_read_pack's steps.  A load lies inside its
// name's span of the text, a store inside its span of `names`.
AASM_DEV void kb_read_names(const KCtx &k, const ReadArgs &a) {
    const int G = AASM_READ_PACK_LANES, gl = k.tid % G;
    const int64_t per_block = k.nthreads / G, n_names = a.C + a.n_chr;
    for (int64_t i = k.bid * per_block + k.tid / G; i < n_names; i += k.nblocks * per_block) {
        const int64_t j = i - a.C;
        const uint8_t *src = a.text + (j < 0 ? a.ctg_pos[i] : a.chr_pos[j]);
        const int64_t d0 = j < 0 ? a.ctg_name_off[i] : a.chr_name_off[j], n = (j < 0 ? a.ctg_name_off[i + 1] : a.chr_name_off[j + 1]) - d0;
        char *dst = a.names + d0;
        for (int64_t o = (int64_t)gl * 8; o + 8 <= n; o += G * 8) read_copy8(dst + o, src + o);
        for (int64_t o = (n & ~(int64_t)7) + gl; o < n; o += G) dst[o] = (char)src[o];
    }
}
// row_index[r] = r, cord_type[r] = TYPE_MAIN: what the host reader's container holds before a --alt merge
AASM_DEV void kb_read_row_ids(const KCtx &k, const ReadArgs &a) {
    for (int64_t i = k.bid * k.nthreads + k.tid; i < a.R; i += k.nblocks * k.nthreads) { a.row_index[i] = (int32_t)i; a.cord_type[i] = 0; }
}

// The reader's kernels (row shapes: aasm_dev.h), body called as body(k, a).  One lane per block in the host emulation:
// every body strides by k.nthreads, and a wave is one lane there.
#define AASM_READ_KERNELS(K, ...) \
    K(KR_COUNT, aasm_read_count, 64, 1, kb_read_count) \
    K(KR_STARTS, aasm_read_starts, 64, 1, kb_read_starts) \
    K(KR_ROWS, aasm_read_rows, 256, 1, kb_read_rows) \
    K(KR_HEADS, aasm_read_heads, 256, 1, kb_read_heads) \
    K(KR_GROUPS, aasm_read_groups, 256, 1, kb_read_groups) \
    K(KR_CHR_LIST, aasm_read_chr_list, 256, 1, kb_read_chr_list) \
    K(KR_REF_IDS, aasm_read_ref_ids, 256, 1, kb_read_ref_ids) \
    K(KR_PACK, aasm_read_pack, 256, 1, kb_read_pack) \
    K(KR_NAMES, aasm_read_names, 256, 1, kb_read_names) \
    K(KR_ROW_IDS, aasm_read_row_ids, 256, 1, kb_read_row_ids)
enum ReadKern { AASM_READ_KERNELS(AASM_ROW_ID, AASM_ROW_ID) KR_N };
constexpr int read_block[] = {AASM_READ_KERNELS(AASM_ROW_BLOCK, AASM_ROW_BLOCK)};
AASM_KERNEL_BODY(run_read_body, AASM_READ_KERNELS, ReadArgs)
#define AASM_READ_MAX_BLOCKS 8192        // beyond 32 per CU the items are taken grid-stride

// ---- driver ----------------------------------------------------------------------------------------------------------------
// What a device read leaves: the resident batch's arrays (device memory the caller now owns) and the counts.
struct ReadOut {
    int64_t C = 0, R = 0, n_ranges = 0, cs_bytes = 0, slow_rows = 0;
    int64_t *ctg_rec_off = nullptr, *qry_str = nullptr, *qry_end = nullptr, *ref_str = nullptr, *ref_end = nullptr, *qry_total = nullptr;
    int64_t *rec_rng_off = nullptr, *rec_cs_off = nullptr;
    int32_t *ref_chr = nullptr;
    uint8_t *aln_fwd = nullptr, *map_qul = nullptr;
    char *cs_text = nullptr;
    // AASM_READ_ROW_COLS (with want_dev): aasm_row_cols' arrays, rows_host_cols' layout (aasm_rows.h)
    int64_t n_chr = 0, names_bytes = 0;
    int64_t *ref_total = nullptr, *ctg_name_off = nullptr, *chr_name_off = nullptr;
    int32_t *mat_num = nullptr, *aln_len = nullptr, *row_index = nullptr;
    uint8_t *cord_type = nullptr;
    char *names = nullptr;
};
#define AASM_READ_FALLBACK 1             // read_run: the text is no PAF the device takes; the host reader says why

// The front of a device read, which the --alt merge (aasm_alt.h) shares: row starts, the rows' columns, and the host's word on the
// rows with a number off the fast path.  a.text, a.len and a.weak_hash are set; want_aln64: a.aln64 takes column 11 in full.
// behind_rows(): what the caller enqueues behind the rows kernel, before the host waits for the words (a.R is known by then).
// Returns AASM_OK with the words in `words`, AASM_READ_FALLBACK (a.R says how many rows were framed), or the backend's failure.
static inline int64_t read_blocks_for(int64_t items, int64_t per_block, int64_t max_blocks) {
    return std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, max_blocks));
}
template <class B, class F> int read_front(B &be, ReadArgs &a, const char *text, bool on_dev, int64_t max_blocks, int32_t (&words)[RW_N], bool want_aln64, F behind_rows) {
    auto blocks_for = [&](int64_t items, int per_block) { return read_blocks_for(items, per_block, max_blocks); };
    auto i64s = [&](int64_t n) { return (int64_t *)be.alloc((size_t)n * 8); };
    auto i32s = [&](int64_t n) { return (int32_t *)be.alloc((size_t)n * 4); };
    auto u8s = [&](int64_t n) { return (uint8_t *)be.alloc((size_t)n); };
    const int64_t len = a.len;
    const uint8_t *d_text = a.text;
    // ---- row starts
    be.stage("row starts");
    a.n_tiles = (len + AASM_READ_TILE - 1) / AASM_READ_TILE;
    a.tile_cnt = i32s(a.n_tiles);
    int64_t *tile_off = i64s(a.n_tiles + 1);
    a.tile_off = tile_off;
    be.launch_read(KR_COUNT, blocks_for(a.n_tiles, 1), read_block[KR_COUNT], a);
    be.scan_i32(a.tile_cnt, a.n_tiles, tile_off);
    int64_t R = 0;
    be.d2h(&R, tile_off + a.n_tiles, 8);
    if (!be.ok()) return be.code();
    a.R = R;
    if (R <= 0 || R > INT32_MAX) return AASM_READ_FALLBACK;          // "empty PAF", "more than 2147483647 rows"
    a.row_start = i64s(R);
    be.launch_read(KR_STARTS, blocks_for(a.n_tiles, 1), read_block[KR_STARTS], a);
    // ---- rows
    be.stage("rows");
    a.qs = i64s(R); a.qe = i64s(R); a.rs = i64s(R); a.re = i64s(R); a.qtot = i64s(R); a.rtot = i64s(R);
    a.mat = i32s(R); a.aln = i32s(R); a.fwd = u8s(R); a.mq = u8s(R);
    if (want_aln64) a.aln64 = i64s(R);
    a.tag_start = i64s(R); a.rn_start = i64s(R); a.tag_len = i32s(R); a.n_colon = i32s(R); a.qn_len = i32s(R); a.rn_len = i32s(R);
    a.rn_hash = (uint64_t *)i64s(R);
    a.words = i32s(RW_N); a.slow_row = i32s(R);
    const int32_t words0[RW_N] = {INT32_MAX, 0, 0, 0};
    be.h2d(a.words, words0, sizeof words0);
    be.launch_read(KR_ROWS, blocks_for(R, read_block[KR_ROWS]), read_block[KR_ROWS], a);
    behind_rows();
    be.d2h(words, a.words, sizeof words);
    if (!be.ok()) return be.code();
    if (words[RW_FAULT] != INT32_MAX) return AASM_READ_FALLBACK;     // a row that is none: the first one in file order
    // ---- numbers off the fast path: the host's own parse_row decides, and patches the row's columns on the device
    const int64_t n_slow = words[RW_SLOW];
    if (n_slow > 0) {
        be.stage("slow rows");
        std::vector<int32_t> rows((size_t)n_slow);
        be.d2h(rows.data(), a.slow_row, (size_t)n_slow * 4);
        std::vector<int64_t> starts;
        if (n_slow > 64) { starts.resize((size_t)R); be.d2h(starts.data(), a.row_start, (size_t)R * 8); }
        if (!be.ok()) return be.code();
        std::vector<char> fetched;                                   // (device text: the row's bytes come back, up to the next row's start)
        for (int32_t r : rows) {
            int64_t p = 0, p1 = len;
            if (starts.empty()) be.d2h(&p, a.row_start + r, 8); else p = starts[(size_t)r];
            if (on_dev && r + 1 < R) { if (starts.empty()) be.d2h(&p1, a.row_start + r + 1, 8); else p1 = starts[(size_t)r + 1]; }
            if (!be.ok()) return be.code();
            const char *row = on_dev ? nullptr : text + p;           // the row and what follows it: row[0, avail)
            const int64_t avail = p1 - p;
            if (on_dev) {
                fetched.resize((size_t)avail);
                be.d2h(fetched.data(), d_text + p, (size_t)avail);
                if (!be.ok()) return be.code();
                row = fetched.data();
            }
            const char *nl = (const char *)std::memchr(row, '\n', (size_t)avail);
            int64_t e = nl ? nl - row : avail;
            if (e > 0 && row[e - 1] == '\r') e--;
            ReadRowCols w;
            if (!read_slow_row(row, row + e, w)) return AASM_READ_FALLBACK;   // ROW_NUMBER: the host reader names the first one
            be.h2d(a.qs + r, &w.qry_str, 8); be.h2d(a.qe + r, &w.qry_end, 8); be.h2d(a.rs + r, &w.ref_str, 8); be.h2d(a.re + r, &w.ref_end, 8);
            be.h2d(a.qtot + r, &w.qry_total, 8); be.h2d(a.rtot + r, &w.ref_total, 8); be.h2d(a.mat + r, &w.mat_num, 4); be.h2d(a.aln + r, &w.aln_len, 4);
            be.h2d(a.mq + r, &w.map_qul, 1);
            if (a.aln64) be.h2d(a.aln64 + r, &w.aln_len64, 8);
        }
    }
    return be.ok() ? AASM_OK : be.code();
}

// read_run(be, ...) over a backend that provides
//   void *alloc(size_t)            device memory, nullptr after a failure (every later call is then a no-op); freed with the backend
//   void release(void *)           ... or now;   void keep(void *): the caller's from here on
//   h2d / d2h(dst, src, n)         d2h waits;   fill32(p, value, count)
//   scan_i32 / scan_u8(in, n, out) exclusive scan into int64 out[n + 1]
//   launch_read(kernel, blocks, threads, ReadArgs);   stage(name): a launch group's name, for timing;   bool ok()
// text: HOST memory; under AASM_READ_TEXT_ON_DEVICE device memory, 16-byte aligned, that is neither copied nor written (paf is
// nullptr then: the container is cut from host text).  paf: the container to fill, or nullptr; want_dev: hand the batch's arrays out
// in `out` (else they are freed), under AASM_READ_ROW_COLS the row columns' arrays with them.
// Returns AASM_OK, AASM_READ_FALLBACK, or the backend's failure as AASM_E_NOMEM / AASM_E_HIP through be.code().
template <class B> int read_run(B &be, const char *text, int64_t len, int flags, aasm_paf *paf, bool want_dev, ReadOut &out) {
    const int64_t max_blocks = (flags & AASM_READ_H_FEW_BLOCKS) ? 3 : AASM_READ_MAX_BLOCKS;   // (the hook: fewer blocks than items)
    auto blocks_for = [&](int64_t items, int per_block) { return read_blocks_for(items, per_block, max_blocks); };
    auto i64s = [&](int64_t n) { return (int64_t *)be.alloc((size_t)n * 8); };
    auto i32s = [&](int64_t n) { return (int32_t *)be.alloc((size_t)n * 4); };
    auto u8s = [&](int64_t n) { return (uint8_t *)be.alloc((size_t)n); };
    ReadArgs a;
    std::memset(&a, 0, sizeof a);
    if (len <= 0) return AASM_READ_FALLBACK;
    const bool on_dev = (flags & AASM_READ_TEXT_ON_DEVICE) != 0, row_cols = (flags & AASM_READ_ROW_COLS) != 0 && want_dev;
    if (on_dev && paf) return AASM_E_INVAL;
    be.stage("upload");
    uint8_t *d_text = on_dev ? (uint8_t *)const_cast<char *>(text) : u8s(len);
    if (!on_dev) be.h2d(d_text, text, (size_t)len);
    a.text = d_text; a.len = len; a.weak_hash = (flags & AASM_READ_H_WEAK_HASH) ? 1 : 0;
    // ---- row starts, rows, slow rows; the contig heads and both offset scans are enqueued behind the rows kernel
    int64_t *head_off = nullptr, *cs_off = nullptr, *rng_off = nullptr;
    int32_t words[RW_N];
    const int frc = read_front(be, a, text, on_dev, max_blocks, words, false, [&] {
        const int64_t R = a.R;
        a.ref_chr = i32s(R); a.head = u8s(R); a.cnew = u8s(R);
        head_off = i64s(R + 1); cs_off = i64s(R + 1); rng_off = i64s(R + 1);
        a.head_off = head_off; a.cs_off = cs_off;
        be.stage("contigs");
        be.launch_read(KR_HEADS, blocks_for(R, read_block[KR_HEADS]), read_block[KR_HEADS], a);
        be.scan_u8(a.head, R, head_off);
        be.stage("offsets");
        be.scan_i32(a.tag_len, R, cs_off);
        be.scan_i32(a.n_colon, R, rng_off);
    });
    if (frc != AASM_OK) return frc;
    const int64_t R = a.R, n_slow = words[RW_SLOW];
    int64_t C = 0, cs_bytes = 0, n_ranges = 0;
    be.d2h(&C, head_off + R, 8); be.d2h(&cs_bytes, cs_off + R, 8); be.d2h(&n_ranges, rng_off + R, 8);
    if (!be.ok()) return be.code();
    // ---- contigs, reference names by first appearance
    be.stage("reference ids");
    const int64_t n_new = words[RW_NEW];
    int64_t cap = 64;
    while (cap < 2 * n_new) cap <<= 1;
    a.tab_mask = cap - 1;
    a.tab_owner = i32s(cap); a.tab_min = i32s(cap);
    a.ctg_rec_off = i64s(C + 1); a.ctg_pos = i64s(C); a.ctg_len = i32s(C); a.chr_info = i64s(3 * n_new);
    be.fill32(a.tab_owner, -1, cap); be.fill32(a.tab_min, INT32_MAX, cap);
    be.launch_read(KR_GROUPS, blocks_for(R, read_block[KR_GROUPS]), read_block[KR_GROUPS], a);
    be.launch_read(KR_CHR_LIST, blocks_for(cap, read_block[KR_CHR_LIST]), read_block[KR_CHR_LIST], a);
    be.d2h(words, a.words, sizeof words);
    if (!be.ok()) return be.code();
    const int64_t n_chr = words[RW_CHR];
    std::vector<int64_t> info((size_t)n_chr * 3);
    be.d2h(info.data(), a.chr_info, info.size() * 8);
    if (!be.ok()) return be.code();
    std::vector<int64_t> order((size_t)n_chr);
    for (int64_t j = 0; j < n_chr; j++) order[(size_t)j] = j;
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return info[(size_t)x * 3] < info[(size_t)y * 3]; });
    std::vector<int32_t> sorted((size_t)n_chr);
    for (int64_t j = 0; j < n_chr; j++) sorted[(size_t)j] = (int32_t)info[(size_t)order[(size_t)j] * 3];
    int32_t *d_sorted = i32s(n_chr);
    be.h2d(d_sorted, sorted.data(), sorted.size() * 4);
    a.chr_sorted = d_sorted; a.n_chr = (int32_t)n_chr;
    be.launch_read(KR_REF_IDS, blocks_for(R, read_block[KR_REF_IDS]), read_block[KR_REF_IDS], a);
    // ---- the tags, back to back
    be.stage("pack");
    a.cs_text = (char *)u8s(cs_bytes);
    be.launch_read(KR_PACK, blocks_for(R, read_block[KR_PACK] / AASM_READ_PACK_LANES), read_block[KR_PACK], a);
    // ---- the row columns: names back to back (contigs, then references by first appearance), row_index, cord_type
    int64_t *ctg_name_off = nullptr, *chr_name_off = nullptr;
    int64_t names_bytes = 0;
    if (row_cols) {
        be.stage("names");
        ctg_name_off = i64s(C + 1); chr_name_off = i64s(n_chr + 1);
        int64_t *chr_pos = i64s(n_chr);
        be.scan_i32(a.ctg_len, C, ctg_name_off);
        int64_t ctg_bytes = 0;
        be.d2h(&ctg_bytes, ctg_name_off + C, 8);
        if (!be.ok()) return be.code();
        std::vector<int64_t> off((size_t)n_chr + 1, ctg_bytes), pos((size_t)n_chr);
        for (int64_t j = 0; j < n_chr; j++) { pos[(size_t)j] = info[(size_t)order[(size_t)j] * 3 + 1]; off[(size_t)j + 1] = off[(size_t)j] + info[(size_t)order[(size_t)j] * 3 + 2]; }
        names_bytes = off[(size_t)n_chr];
        be.h2d(chr_name_off, off.data(), off.size() * 8); be.h2d(chr_pos, pos.data(), pos.size() * 8);
        a.C = C; a.ctg_name_off = ctg_name_off; a.chr_name_off = chr_name_off; a.chr_pos = chr_pos;
        a.names = (char *)u8s(names_bytes); a.row_index = i32s(R); a.cord_type = u8s(R);
        be.launch_read(KR_NAMES, blocks_for(C + n_chr, read_block[KR_NAMES] / AASM_READ_PACK_LANES), read_block[KR_NAMES], a);
        be.launch_read(KR_ROW_IDS, blocks_for(R, read_block[KR_ROW_IDS]), read_block[KR_ROW_IDS], a);
    }
    if (on_dev) { int64_t w = 0; be.d2h(&w, cs_off, 8); }             // (the caller's text: nothing is released, the launches are waited for)
    else be.release(d_text);                                              // (waits for the launches; nothing reads the raw text on the device any more)
    be.stage("container");
    if (!be.ok()) return be.code();
    // ---- the writers' container: columns and offsets from the device, names and tags from the host's own text
    if (paf) {
        paf->device_ranges = true; paf->has_cs = true;
#define AASM_X(T_, name) paf->name.resize((size_t)R);
        AASM_PAF_RECORD_COLUMNS(AASM_X)
#undef AASM_X
        paf->cs_off.resize((size_t)R + 1); paf->rec_rng_off.resize((size_t)R + 1); paf->ctg_rec_off.resize((size_t)C + 1);
        std::vector<int64_t> tag_start((size_t)R), ctg_pos((size_t)C);
        std::vector<int32_t> ctg_len((size_t)C);
        be.d2h(paf->qry_str.data(), a.qs, (size_t)R * 8); be.d2h(paf->qry_end.data(), a.qe, (size_t)R * 8);
        be.d2h(paf->ref_str.data(), a.rs, (size_t)R * 8); be.d2h(paf->ref_end.data(), a.re, (size_t)R * 8);
        be.d2h(paf->qry_total.data(), a.qtot, (size_t)R * 8); be.d2h(paf->ref_total.data(), a.rtot, (size_t)R * 8);
        be.d2h(paf->ref_chr.data(), a.ref_chr, (size_t)R * 4); be.d2h(paf->mat_num.data(), a.mat, (size_t)R * 4); be.d2h(paf->aln_len.data(), a.aln, (size_t)R * 4);
        be.d2h(paf->aln_fwd.data(), a.fwd, (size_t)R); be.d2h(paf->map_qul.data(), a.mq, (size_t)R);
        be.d2h(paf->cs_off.data(), cs_off, (size_t)(R + 1) * 8); be.d2h(paf->rec_rng_off.data(), rng_off, (size_t)(R + 1) * 8);
        be.d2h(paf->ctg_rec_off.data(), a.ctg_rec_off, (size_t)(C + 1) * 8);
        be.d2h(tag_start.data(), a.tag_start, (size_t)R * 8); be.d2h(ctg_pos.data(), a.ctg_pos, (size_t)C * 8); be.d2h(ctg_len.data(), a.ctg_len, (size_t)C * 4);
        if (!be.ok()) return be.code();
        paf->cs_pool.resize((size_t)cs_bytes);
        int T = host_threads();
        if (len < (1 << 16)) T = 1;
        std::vector<std::thread> th;
        auto fill = [&](int t) {                                     // (the packed text never comes back from the device)
            for (int64_t r = R * t / T; r < R * (t + 1) / T; r++) {
                std::memcpy(paf->cs_pool.data() + paf->cs_off[(size_t)r], text + tag_start[(size_t)r], (size_t)(paf->cs_off[(size_t)r + 1] - paf->cs_off[(size_t)r]));
                paf->row_index[(size_t)r] = (int32_t)r;              // (cord_type: TYPE_MAIN, the resize's zero)
            }
        };
        for (int t = 1; t < T; t++) th.emplace_back(fill, t);
        fill(0);
        for (auto &x : th) x.join();
        paf->ctg_name.clear(); paf->chr_name.clear();
        for (int64_t c = 0; c < C; c++) paf->ctg_name.emplace_back(text + ctg_pos[(size_t)c], (size_t)ctg_len[(size_t)c]);
        for (int64_t j = 0; j < n_chr; j++) paf->chr_name.emplace_back(text + info[(size_t)order[(size_t)j] * 3 + 1], (size_t)info[(size_t)order[(size_t)j] * 3 + 2]);
    }
    out.C = C; out.R = R; out.n_ranges = n_ranges; out.cs_bytes = cs_bytes; out.slow_rows = n_slow;
    if (want_dev) {
        out.ctg_rec_off = a.ctg_rec_off; out.qry_str = a.qs; out.qry_end = a.qe; out.ref_str = a.rs; out.ref_end = a.re; out.qry_total = a.qtot;
        out.rec_rng_off = rng_off; out.rec_cs_off = cs_off; out.ref_chr = a.ref_chr; out.aln_fwd = a.fwd; out.map_qul = a.mq; out.cs_text = a.cs_text;
        for (void *p : {(void *)a.ctg_rec_off, (void *)a.qs, (void *)a.qe, (void *)a.rs, (void *)a.re, (void *)a.qtot, (void *)rng_off, (void *)cs_off,
                        (void *)a.ref_chr, (void *)a.fwd, (void *)a.mq, (void *)a.cs_text})
            be.keep(p);
        if (row_cols) {
            out.n_chr = n_chr; out.names_bytes = names_bytes;
            out.ref_total = a.rtot; out.mat_num = a.mat; out.aln_len = a.aln; out.row_index = a.row_index; out.cord_type = a.cord_type;
            out.names = a.names; out.ctg_name_off = ctg_name_off; out.chr_name_off = chr_name_off;
            for (void *p : {(void *)a.rtot, (void *)a.mat, (void *)a.aln, (void *)a.row_index, (void *)a.cord_type, (void *)a.names, (void *)ctg_name_off, (void *)chr_name_off})
                be.keep(p);
        }
    }
    be.stage("free");
    return be.ok() ? AASM_OK : be.code();
}

// AASM_READ_FALLBACK: the host reader on the same text, whose code and message are the entry's
static inline int read_host_verdict(const char *text, int64_t len) {
    aasm_paf *hp = nullptr;
    const int rc = aasm_paf_parse_mem_opts(text, len, AASM_READ_DEVICE_RANGES, &hp);
    if (rc != AASM_OK) return rc;
    aasm_paf_free(hp);
    set_last_error("aasm_paf_parse_device: the device found fault with a text the host reader takes");
    return AASM_E_INTERNAL;
}

}  // namespace aasm
