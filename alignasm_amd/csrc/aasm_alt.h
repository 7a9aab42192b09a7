// aasm_alt.h -- the --alt merge on the device (aasm_paf_merge_alt_device): kernel bodies, kernel table, host driver.
//
// merge_alt_text (aasm_paf.cpp; alignasm.cpp:203-332) on a batch that is resident in its cs form with its row columns: the rows
// of the second PAF are framed and parsed by the reader's own kernels (read_front, aasm_read.h), then
//   pieces     a lane per alt row: the piece name up to its first ':', the shift (the digits between that ':' and the next '-' or
//              the name's end, minus 1; 1 - 18 digits, anything else declines), the piece's hash, aln_len / qry_total as an IEEE
//              double division of the row's own columns 11 and 2
//   tables     two linear-probing tables built as read_ref_slot is: the contig names of the resident `names` (a slot keeps the
//              HIGHEST contig of equal names: a repeated name resolves to its last contig, :136), and the reference names - the
//              resident ones first, then the alt rows whose name is none of them, lowest row per slot.  The new names are few:
//              they are listed, ordered by first row on the host and numbered behind the main file's
//   lookup     a lane per alt row: its contig (0 where the piece's name is unknown, operator[] at :269), its reference id
//   groups     a row heads a group iff piece or shift differ from the row before; a scan numbers the groups; two atomic passes
//              give a group its rows over the baseline and the first row of its largest positive ratio.  A group with neither
//              lowers the decline word: its zeroed stand-in (and what the reference makes of it one row late) is the host's
//   keep       flags scanned into the list of kept rows
//   placement  the kept list splits into maximal runs of one contig; the run table goes to the host, which gives every run its
//              base among its contig's added rows (file order) and every contig its added count; main counts + added counts are
//              scanned into the new ctg_rec_off
//   build      a lane per main record and a lane per kept row write the merged columns, the tag's length, ':' count and source;
//              two scans make rec_cs_off and rec_rng_off; sixteen lanes per record copy its tag from the old cs_text or the alt
//              text in kb_read_pack's steps; sixteen lanes per name write the merged `names`
// No lane's work grows with a group's or a contig's length.  No load leaves the alt text or the resident arrays.
// The driver (alt_merge_run) is shared by the product backend (aasm_gpu.hip) and the 1-lane host emulation (tests/host_emul/alt_emul.cpp).
#pragma once
#include "aasm_read.h"

namespace aasm {

enum { AW_NEW = 0, AW_CHR, AW_N };                                   // AltArgs::words: alt rows with a changed reference name, new table entries
enum AltWhy { ALT_WHY_ROW = 1, ALT_WHY_NO_COLON, ALT_WHY_PIECE_NUMBER, ALT_WHY_ZEROED, ALT_WHY_TOO_MANY };   // low 3 bits of the decline word
static inline const char *alt_why_text(int why) {
    switch (why) {
        case ALT_WHY_ROW: return "a row off the device reader's path";
        case ALT_WHY_NO_COLON: return "a piece name without ':'";
        case ALT_WHY_PIECE_NUMBER: return "a piece start that is not 1 - 18 digits";
        case ALT_WHY_ZEROED: return "a group without a positive ratio";
        case ALT_WHY_TOO_MANY: return "more than 2147483647 records";
    }
    return "?";
}

struct AltArgs {
    ReadArgs r;                          // the alt text and its rows' columns (r.R alt rows)
    // the resident batch and its row columns: read only
    int64_t C, R, n_chr;
    const int64_t *m_ctg_off, *m_qs, *m_qe, *m_rs, *m_re, *m_qtot, *m_rng_off, *m_cs_off, *m_rtot, *m_ctg_name_off, *m_chr_name_off;
    const int32_t *m_ref_chr, *m_mat, *m_aln, *m_row_index;
    const uint8_t *m_fwd, *m_mq, *m_cord;
    const char *m_cs_text, *m_names;
    double baseline;
    // per alt row
    int32_t *piece_len, *a_ctg, *a_chr;  // [Ra]
    int64_t *shift;
    uint64_t *phash;
    double *ratio;
    uint8_t *ghead, *rnew, *keep;        // [Ra] heads a group; another reference name than the row before; kept
    const int64_t *grp_off, *keep_off;   // [Ra + 1] exclusive scans of ghead, keep
    int64_t *fault;                      // [1] the decline word: min of (row << 3 | AltWhy)
    int32_t *words;                      // [AW_N]
    // the name tables
    uint64_t *ctg_hash, *chr_hash;       // [C], [n_chr]
    int32_t *ct_owner, *ct_max;          // [ct_mask + 1] owner: a contig whose name is the key, -1 empty; the highest contig of that name
    int32_t *rt_owner, *rt_min;          // [rt_mask + 1] owner: alt row >= 0, resident name j as -(j + 2), -1 empty; the lowest alt row
    int64_t ct_mask, rt_mask;
    int64_t *chr_info;                   // {first row, name start, name length} per new name
    const int32_t *chr_sorted;           // [n_new] the new names' first rows, ascending
    int32_t n_new;
    // groups
    int32_t *g_over, *g_best;            // [G] rows over the baseline; first row of the largest positive ratio
    int64_t *g_max;                      // [G] that ratio's bits (positive doubles order as integers), 0: none
    // kept rows and their runs
    int64_t K, NR;
    int32_t *kept_row;                   // [K]
    uint8_t *run_head;                   // [K]
    const int64_t *run_off;              // [K + 1]
    int64_t *run_info;                   // {contig, first kept} per run
    const int64_t *run_base;             // [NR] the run's first place among its contig's added rows
    const int32_t *added;                // [C]
    int32_t *new_cnt;                    // [C]
    const int64_t *new_ctg_off;          // [C + 1]
    // the merged batch
    int64_t *o_qs, *o_qe, *o_rs, *o_re, *o_qtot, *o_rtot, *o_src;   // o_src: the tag in the old cs_text (>= 0) or in the alt text (-1 - position)
    int32_t *o_ref_chr, *o_mat, *o_aln, *o_row_index, *o_tag_len, *o_colon;
    uint8_t *o_fwd, *o_mq, *o_cord;
    const int64_t *o_cs_off;             // [R' + 1]
    char *o_cs_text, *o_names;
    int64_t *o_ctg_name_off, *o_chr_name_off;
    const int64_t *new_pos;              // [n_new] the new names in the alt text, in first-appearance order
};

AASM_DEV void atomic_max_neg_i32(int32_t *p, int32_t v) { atomic_min_i32(p, -v); }   // a maximum kept as the minimum of the negatives

struct AltKey { const uint8_t *p; int64_t n; uint64_t h; };
AASM_DEV bool alt_key_eq(const AltKey &x, const AltKey &y) {
    if (x.n != y.n || x.h != y.h) return false;
    for (int64_t t = 0; t < x.n; t++) if (x.p[t] != y.p[t]) return false;
    return true;
}
AASM_DEV uint64_t alt_hash(const AltArgs &a, const uint8_t *p, int64_t n) {
    if (a.r.weak_hash) return (uint64_t)(n & 3);
    uint64_t h = AASM_READ_HASH0;
    for (int64_t t = 0; t < n; t++) h = (h ^ (uint64_t)p[t]) * AASM_READ_HASH_MUL;
    return h;
}
AASM_DEV int64_t alt_slot0(uint64_t h, int64_t mask) { return (int64_t)(h * 0x9e3779b97f4a7c15ull >> 20) & mask; }

// ---- pieces: "<name>:<start>[-<end>]" -> the name's length, start - 1 (split_piece_name, aasm_paf.cpp), hash, ratio
AASM_DEV void kb_alt_pieces(const KCtx &k, const AltArgs &a) {
    for (int64_t i = k.bid * k.nthreads + k.tid; i < a.r.R; i += k.nblocks * k.nthreads) {
        const uint8_t *q = a.r.text + a.r.row_start[i];
        const int64_t n = a.r.qn_len[i];
        int64_t t = 0;
        while (t < n && q[t] != ':') t++;
        int why = t == n ? ALT_WHY_NO_COLON : 0;
        int64_t val = 0;
        int nd = 0;
        bool bad = false;
        for (int64_t u = t + 1; u < n && q[u] != '-'; u++) {          // (a '-' ends the span, so no sign is ever inside it)
            const unsigned dg = (unsigned)(q[u] - '0');
            if (dg > 9u) bad = true;
            else if (++nd <= 18) val = val * 10 + (int64_t)dg;
        }
        if (!why && (bad || nd < 1 || nd > 18)) why = ALT_WHY_PIECE_NUMBER;
        if (why) atomic_min_i64(a.fault, (i << 3) | why);
        a.piece_len[i] = (int32_t)t; a.shift[i] = val - 1; a.phash[i] = alt_hash(a, q, t);
        a.ratio[i] = (double)a.r.aln64[i] / (double)a.r.qtot[i];
    }
}

// ---- the contig names' table
AASM_DEV AltKey alt_ctg_key(const AltArgs &a, int64_t c) {
    return AltKey{(const uint8_t *)a.m_names + a.m_ctg_name_off[c], a.m_ctg_name_off[c + 1] - a.m_ctg_name_off[c], a.ctg_hash[c]};
}
AASM_DEV void kb_alt_ctg_hash(const KCtx &k, const AltArgs &a) {
    for (int64_t c = k.bid * k.nthreads + k.tid; c < a.C + a.n_chr; c += k.nblocks * k.nthreads) {
        const int64_t j = c - a.C;
        const int64_t *off = j < 0 ? a.m_ctg_name_off + c : a.m_chr_name_off + j;
        const uint64_t h = alt_hash(a, (const uint8_t *)a.m_names + off[0], off[1] - off[0]);
        if (j < 0) a.ctg_hash[c] = h; else a.chr_hash[j] = h;
    }
}
AASM_DEV AltKey alt_ref_key(const AltArgs &a, int32_t o) {
    if (o <= -2) { const int64_t j = -((int64_t)o + 2); return AltKey{(const uint8_t *)a.m_names + a.m_chr_name_off[j], a.m_chr_name_off[j + 1] - a.m_chr_name_off[j], a.chr_hash[j]}; }
    return AltKey{a.r.text + a.r.rn_start[o], (int64_t)a.r.rn_len[o], a.r.rn_hash[o]};
}
// the slot of reference name `me` (an alt row, or resident name j as -(j + 2)); claim: an empty slot met on the way becomes the name's
AASM_DEV int64_t alt_ref_slot(const AltArgs &a, int32_t me, bool claim) {
    const AltKey key = alt_ref_key(a, me);
    int64_t s = alt_slot0(key.h, a.rt_mask);
    for (int64_t n = 0; n <= a.rt_mask; n++, s = (s + 1) & a.rt_mask) {
        int32_t o = a.rt_owner[s];
        if (o == -1) {
            if (!claim) return -1;
            o = atomic_cas_i32(&a.rt_owner[s], -1, me);
            if (o == -1) o = me;
        }
        if (o == me || alt_key_eq(key, alt_ref_key(a, o))) return s;
    }
    return -1;
}
// a lane per contig name, then per resident reference name: into their tables
AASM_DEV void kb_alt_tables(const KCtx &k, const AltArgs &a) {
    for (int64_t c = k.bid * k.nthreads + k.tid; c < a.C + a.n_chr; c += k.nblocks * k.nthreads) {
        if (c >= a.C) { (void)alt_ref_slot(a, (int32_t)(-(c - a.C) - 2), true); continue; }
        const AltKey key = alt_ctg_key(a, c);
        int64_t s = alt_slot0(key.h, a.ct_mask);
        for (int64_t n = 0; n <= a.ct_mask; n++, s = (s + 1) & a.ct_mask) {
            int32_t o = a.ct_owner[s];
            if (o < 0) {
                o = atomic_cas_i32(&a.ct_owner[s], -1, (int32_t)c);
                if (o < 0) o = (int32_t)c;
            }
            if (o == (int32_t)c || alt_key_eq(key, alt_ctg_key(a, o))) { atomic_max_neg_i32(&a.ct_max[s], (int32_t)c); break; }
        }
    }
}
// Row i against row i - 1: a new group (equal piece bytes and equal shift make one, merge_alt_text)?  another reference name?
AASM_DEV void kb_alt_heads(const KCtx &k, const AltArgs &a) {
    for (int64_t i = k.bid * k.nthreads + k.tid; i < a.r.R; i += k.nblocks * k.nthreads) {
        bool head = i == 0 || a.piece_len[i] != a.piece_len[i - 1] || a.shift[i] != a.shift[i - 1] || a.phash[i] != a.phash[i - 1];
        if (!head) head = !read_same_bytes(a.r.text, a.r.row_start[i], a.r.row_start[i - 1], a.piece_len[i]);
        const bool rnew = i == 0 || !read_same_ref(a.r, i, i - 1);
        a.ghead[i] = head ? 1 : 0; a.rnew[i] = rnew ? 1 : 0;
        if (rnew) atomic_add(&a.words[AW_NEW], (int32_t)1);
    }
}
// the alt rows' reference names enter the table behind the resident ones (a launch of its own)
AASM_DEV void kb_alt_ref_rows(const KCtx &k, const AltArgs &a) {
    for (int64_t i = k.bid * k.nthreads + k.tid; i < a.r.R; i += k.nblocks * k.nthreads)
        if (a.rnew[i]) {
            const int64_t s = alt_ref_slot(a, (int32_t)i, true);
            if (s >= 0 && a.rt_owner[s] >= 0) atomic_min_i32(&a.rt_min[s], (int32_t)i);
        }
}
AASM_DEV void kb_alt_chr_list(const KCtx &k, const AltArgs &a) {
    for (int64_t s = k.bid * k.nthreads + k.tid; s <= a.rt_mask; s += k.nblocks * k.nthreads)
        if (a.rt_owner[s] >= 0) {
            const int64_t j = atomic_add(&a.words[AW_CHR], (int32_t)1), r = a.rt_min[s];
            a.chr_info[3 * j] = r; a.chr_info[3 * j + 1] = a.r.rn_start[r]; a.chr_info[3 * j + 2] = a.r.rn_len[r];
        }
}
// ---- lookup: the row's contig and reference id
AASM_DEV void kb_alt_lookup(const KCtx &k, const AltArgs &a) {
    for (int64_t i = k.bid * k.nthreads + k.tid; i < a.r.R; i += k.nblocks * k.nthreads) {
        const AltKey key{a.r.text + a.r.row_start[i], (int64_t)a.piece_len[i], a.phash[i]};
        int32_t ctg = 0;
        int64_t s = alt_slot0(key.h, a.ct_mask);
        for (int64_t n = 0; n <= a.ct_mask; n++, s = (s + 1) & a.ct_mask) {
            const int32_t o = a.ct_owner[s];
            if (o < 0) break;
            if (alt_key_eq(key, alt_ctg_key(a, o))) { ctg = -a.ct_max[s]; break; }
        }
        a.a_ctg[i] = ctg;
        const int64_t rs = alt_ref_slot(a, (int32_t)i, false);
        const int32_t o = rs >= 0 ? a.rt_owner[rs] : -2;
        if (o <= -2) a.a_chr[i] = (int32_t)(-((int64_t)o + 2));
        else {
            const int32_t first = a.rt_min[rs];
            int32_t lo = 0, hi = a.n_new;
            while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if (a.chr_sorted[mid] < first) lo = mid + 1; else hi = mid; }
            a.a_chr[i] = (int32_t)a.n_chr + lo;
        }
    }
}
// ---- groups: rows over the baseline, the largest positive ratio; then its first row, and the verdict on a group that has neither
AASM_DEV int64_t alt_ratio_bits(double x) { int64_t b; __builtin_memcpy(&b, &x, 8); return b; }
AASM_DEV void kb_alt_group_max(const KCtx &k, const AltArgs &a) {
    for (int64_t i = k.bid * k.nthreads + k.tid; i < a.r.R; i += k.nblocks * k.nthreads) {
        const int64_t g = a.grp_off[i + 1] - 1;
        const double x = a.ratio[i];
        if (x > a.baseline) atomic_add(&a.g_over[g], (int32_t)1);
        if (x > 0.0) atomic_max_i64(&a.g_max[g], alt_ratio_bits(x));
    }
}
AASM_DEV void kb_alt_group_best(const KCtx &k, const AltArgs &a) {
    for (int64_t i = k.bid * k.nthreads + k.tid; i < a.r.R; i += k.nblocks * k.nthreads) {
        const int64_t g = a.grp_off[i + 1] - 1;
        const double x = a.ratio[i];
        if (x > 0.0 && alt_ratio_bits(x) == a.g_max[g]) atomic_min_i32(&a.g_best[g], (int32_t)i);
        if (a.ghead[i] && a.g_over[g] == 0 && a.g_max[g] == 0) atomic_min_i64(a.fault, (i << 3) | ALT_WHY_ZEROED);
    }
}
// ---- keep: a group with rows over the baseline keeps exactly those, else its best row
AASM_DEV void kb_alt_keep(const KCtx &k, const AltArgs &a) {
    for (int64_t i = k.bid * k.nthreads + k.tid; i < a.r.R; i += k.nblocks * k.nthreads) {
        const int64_t g = a.grp_off[i + 1] - 1;
        a.keep[i] = (a.g_over[g] > 0 ? a.ratio[i] > a.baseline : a.g_best[g] == (int32_t)i) ? 1 : 0;
    }
}
AASM_DEV void kb_alt_kept(const KCtx &k, const AltArgs &a) {
    for (int64_t i = k.bid * k.nthreads + k.tid; i < a.r.R; i += k.nblocks * k.nthreads)
        if (a.keep[i]) a.kept_row[a.keep_off[i]] = (int32_t)i;
}
// ---- placement: runs of one contig among the kept rows
AASM_DEV void kb_alt_run_heads(const KCtx &k, const AltArgs &a) {
    for (int64_t j = k.bid * k.nthreads + k.tid; j < a.K; j += k.nblocks * k.nthreads)
        a.run_head[j] = (j == 0 || a.a_ctg[a.kept_row[j]] != a.a_ctg[a.kept_row[j - 1]]) ? 1 : 0;
}
AASM_DEV void kb_alt_runs(const KCtx &k, const AltArgs &a) {
    for (int64_t j = k.bid * k.nthreads + k.tid; j < a.K; j += k.nblocks * k.nthreads)
        if (a.run_head[j]) { const int64_t r = a.run_off[j]; a.run_info[2 * r] = a.a_ctg[a.kept_row[j]]; a.run_info[2 * r + 1] = j; }
}
AASM_DEV void kb_alt_counts(const KCtx &k, const AltArgs &a) {
    for (int64_t c = k.bid * k.nthreads + k.tid; c < a.C; c += k.nblocks * k.nthreads)
        a.new_cnt[c] = (int32_t)(a.m_ctg_off[c + 1] - a.m_ctg_off[c]) + a.added[c];
}
// ---- build
// a lane per main record (its contig by bisection of ctg_rec_off), and per name offset of the row columns
AASM_DEV void kb_alt_build_main(const KCtx &k, const AltArgs &a) {
    const int64_t n_off = a.C + 1 + a.n_chr + 1;
    for (int64_t m = k.bid * k.nthreads + k.tid; m < a.R + n_off; m += k.nblocks * k.nthreads) {
        if (m >= a.R) {
            const int64_t j = m - a.R;
            if (j <= a.C) a.o_ctg_name_off[j] = a.m_ctg_name_off[j]; else a.o_chr_name_off[j - a.C - 1] = a.m_chr_name_off[j - a.C - 1];
            continue;
        }
        int64_t lo = 0, hi = a.C;                                     // the last contig whose first record is <= m
        while (hi - lo > 1) { const int64_t mid = (lo + hi) >> 1; if (a.m_ctg_off[mid] <= m) lo = mid; else hi = mid; }
        const int64_t d = m + (a.new_ctg_off[lo] - a.m_ctg_off[lo]);
        a.o_qs[d] = a.m_qs[m]; a.o_qe[d] = a.m_qe[m]; a.o_rs[d] = a.m_rs[m]; a.o_re[d] = a.m_re[m]; a.o_qtot[d] = a.m_qtot[m]; a.o_rtot[d] = a.m_rtot[m];
        a.o_ref_chr[d] = a.m_ref_chr[m]; a.o_mat[d] = a.m_mat[m]; a.o_aln[d] = a.m_aln[m]; a.o_row_index[d] = a.m_row_index[m];
        a.o_fwd[d] = a.m_fwd[m]; a.o_mq[d] = a.m_mq[m]; a.o_cord[d] = a.m_cord[m];
        a.o_tag_len[d] = (int32_t)(a.m_cs_off[m + 1] - a.m_cs_off[m]); a.o_colon[d] = (int32_t)(a.m_rng_off[m + 1] - a.m_rng_off[m]);
        a.o_src[d] = a.m_cs_off[m];
    }
}
// a lane per kept row: behind its contig's main records, at its run's base; coordinates in the contig's, qry_total the contig's
AASM_DEV void kb_alt_build_alt(const KCtx &k, const AltArgs &a) {
    for (int64_t j = k.bid * k.nthreads + k.tid; j < a.K; j += k.nblocks * k.nthreads) {
        const int64_t i = a.kept_row[j], r = a.run_off[j + 1] - 1, c = a.run_info[2 * r];
        const int64_t n_main = a.m_ctg_off[c + 1] - a.m_ctg_off[c];
        const int64_t d = a.new_ctg_off[c] + n_main + a.run_base[r] + (j - a.run_info[2 * r + 1]);
        a.o_qs[d] = a.r.qs[i] + a.shift[i]; a.o_qe[d] = a.r.qe[i] + a.shift[i]; a.o_rs[d] = a.r.rs[i]; a.o_re[d] = a.r.re[i];
        a.o_qtot[d] = a.m_qtot[a.m_ctg_off[c + 1] - 1]; a.o_rtot[d] = a.r.rtot[i];
        a.o_ref_chr[d] = a.a_chr[i]; a.o_mat[d] = a.r.mat[i]; a.o_aln[d] = a.r.aln[i]; a.o_row_index[d] = (int32_t)i;
        a.o_fwd[d] = a.r.fwd[i]; a.o_mq[d] = a.r.mq[i]; a.o_cord[d] = 1;
        a.o_tag_len[d] = a.r.tag_len[i]; a.o_colon[d] = a.r.n_colon[i];
        a.o_src[d] = -1 - a.r.tag_start[i];
    }
}
// AASM_READ_PACK_LANES lanes per merged record: kb_read_pack's steps, from the old cs_text or from the alt text
AASM_DEV void kb_alt_pack(const KCtx &k, const AltArgs &a) {
    const int G = AASM_READ_PACK_LANES, gl = k.tid % G;
    const int64_t per_block = k.nthreads / G, n_rec = a.R + a.K;
    for (int64_t d = k.bid * per_block + k.tid / G; d < n_rec; d += k.nblocks * per_block) {
        const int64_t s = a.o_src[d];
        const uint8_t *src = s >= 0 ? (const uint8_t *)a.m_cs_text + s : a.r.text + (-1 - s);
        char *dst = a.o_cs_text + a.o_cs_off[d];
        const int64_t n = a.o_tag_len[d];
        for (int64_t o = (int64_t)gl * 8; o + 8 <= n; o += G * 8) read_copy8(dst + o, src + o);
        for (int64_t o = (n & ~(int64_t)7) + gl; o < n; o += G) dst[o] = (char)src[o];
    }
}
// ... per name: the resident names where they were, the new reference names behind them
AASM_DEV void kb_alt_names(const KCtx &k, const AltArgs &a) {
    const int G = AASM_READ_PACK_LANES, gl = k.tid % G;
    const int64_t per_block = k.nthreads / G, n_old = a.C + a.n_chr, n_names = n_old + a.n_new;
    for (int64_t i = k.bid * per_block + k.tid / G; i < n_names; i += k.nblocks * per_block) {
        const int64_t j = i - n_old;
        const int64_t *off = i < a.C ? a.m_ctg_name_off + i : a.o_chr_name_off + (i - a.C);   // (o_chr_name_off: the resident offsets, then the new ones)
        const int64_t d0 = off[0], n = off[1] - d0;
        const uint8_t *src = j < 0 ? (const uint8_t *)a.m_names + d0 : a.r.text + a.new_pos[j];
        char *dst = a.o_names + d0;
        for (int64_t o = (int64_t)gl * 8; o + 8 <= n; o += G * 8) read_copy8(dst + o, src + o);
        for (int64_t o = (n & ~(int64_t)7) + gl; o < n; o += G) dst[o] = (char)src[o];
    }
}

// The merge's kernels (row shapes: aasm_dev.h), body called as body(k, a).  One lane per block in the host emulation.
#define AASM_ALT_KERNELS(K, ...) \
    K(KA_PIECES, aasm_alt_pieces, 256, 1, kb_alt_pieces) \
    K(KA_CTG_HASH, aasm_alt_ctg_hash, 256, 1, kb_alt_ctg_hash) \
    K(KA_TABLES, aasm_alt_tables, 256, 1, kb_alt_tables) \
    K(KA_HEADS, aasm_alt_heads, 256, 1, kb_alt_heads) \
    K(KA_REF_ROWS, aasm_alt_ref_rows, 256, 1, kb_alt_ref_rows) \
    K(KA_CHR_LIST, aasm_alt_chr_list, 256, 1, kb_alt_chr_list) \
    K(KA_LOOKUP, aasm_alt_lookup, 256, 1, kb_alt_lookup) \
    K(KA_GROUP_MAX, aasm_alt_group_max, 256, 1, kb_alt_group_max) \
    K(KA_GROUP_BEST, aasm_alt_group_best, 256, 1, kb_alt_group_best) \
    K(KA_KEEP, aasm_alt_keep, 256, 1, kb_alt_keep) \
    K(KA_KEPT, aasm_alt_kept, 256, 1, kb_alt_kept) \
    K(KA_RUN_HEADS, aasm_alt_run_heads, 256, 1, kb_alt_run_heads) \
    K(KA_RUNS, aasm_alt_runs, 256, 1, kb_alt_runs) \
    K(KA_COUNTS, aasm_alt_counts, 256, 1, kb_alt_counts) \
    K(KA_BUILD_MAIN, aasm_alt_build_main, 256, 1, kb_alt_build_main) \
    K(KA_BUILD_ALT, aasm_alt_build_alt, 256, 1, kb_alt_build_alt) \
    K(KA_PACK, aasm_alt_pack, 256, 1, kb_alt_pack) \
    K(KA_NAMES, aasm_alt_names, 256, 1, kb_alt_names)
enum AltKern { AASM_ALT_KERNELS(AASM_ROW_ID, AASM_ROW_ID) KA_N };
constexpr int alt_block[] = {AASM_ALT_KERNELS(AASM_ROW_BLOCK, AASM_ROW_BLOCK)};
AASM_KERNEL_BODY(run_alt_body, AASM_ALT_KERNELS, AltArgs)

// ---- driver ----------------------------------------------------------------------------------------------------------------
// What a merge leaves: the merged batch's arrays and row columns (device memory the caller now owns) and the counts.
struct AltOut {
    int64_t C = 0, R = 0, n_ranges = 0, n_chr = 0, names_bytes = 0, kept = 0, slow_rows = 0;
    int64_t *ctg_rec_off = nullptr, *qry_str = nullptr, *qry_end = nullptr, *ref_str = nullptr, *ref_end = nullptr, *qry_total = nullptr;
    int64_t *rec_rng_off = nullptr, *rec_cs_off = nullptr, *ref_total = nullptr, *ctg_name_off = nullptr, *chr_name_off = nullptr;
    int32_t *ref_chr = nullptr, *mat_num = nullptr, *aln_len = nullptr, *row_index = nullptr;
    uint8_t *aln_fwd = nullptr, *map_qul = nullptr, *cord_type = nullptr;
    char *cs_text = nullptr, *names = nullptr;
    int why = 0;                         // AASM_ALT_DECLINED: AltWhy and the alt row
    int64_t why_row = 0;
};
// the arrays of a merge's result, in aasm_batch_in's order and then aasm_row_cols'
static inline std::vector<void *> alt_out_arrays(const AltOut &o) {
    return {o.ctg_rec_off, o.qry_str, o.qry_end, o.ref_str, o.ref_end, o.qry_total, o.ref_chr, o.aln_fwd, o.map_qul, o.rec_rng_off, o.cs_text, o.rec_cs_off,
            o.ref_total, o.mat_num, o.aln_len, o.row_index, o.cord_type, o.names, o.ctg_name_off, o.chr_name_off};
}
#define AASM_ALT_DECLINED 1              // alt_merge_run: the device does not merge this text; the host says whether it would

// alt_merge_run(be, ...) over read_run's backend, with launch_alt(kernel, blocks, threads, AltArgs) beside launch_read.
// in / cols: the resident batch in its cs form and its row columns (device memory, read only).  text: HOST memory.
// Returns AASM_OK, AASM_ALT_DECLINED (nothing was built), or the backend's failure as AASM_E_NOMEM / AASM_E_HIP through be.code().
template <class B> int alt_merge_run(B &be, const aasm_batch_in &in, const aasm_row_cols &cols, const char *text, int64_t len, double baseline, int flags, AltOut &out) {
    const int64_t max_blocks = (flags & AASM_READ_H_FEW_BLOCKS) ? 3 : AASM_READ_MAX_BLOCKS;
    auto blocks_for = [&](int64_t items, int per_block) { return read_blocks_for(items, per_block, max_blocks); };
    auto i64s = [&](int64_t n) { return (int64_t *)be.alloc((size_t)n * 8); };
    auto i32s = [&](int64_t n) { return (int32_t *)be.alloc((size_t)n * 4); };
    auto u8s = [&](int64_t n) { return (uint8_t *)be.alloc((size_t)n); };
    AltArgs a;
    std::memset(&a, 0, sizeof a);
    auto run = [&](int ka, int64_t items, int lanes_per_item = 1) { be.launch_alt(ka, blocks_for(items, alt_block[ka] / lanes_per_item), alt_block[ka], a); };
    auto cap_for = [](int64_t entries) { int64_t cap = 64; while (cap < 2 * entries) cap <<= 1; return cap; };
    auto declined = [&](int why, int64_t row) { out.why = why; out.why_row = row; return AASM_ALT_DECLINED; };
    const int64_t C = in.n_contigs, R = in.n_records, n_chr = cols.n_chr;
    a.C = C; a.R = R; a.n_chr = n_chr; a.baseline = baseline;
    a.m_ctg_off = in.ctg_rec_off; a.m_qs = in.qry_str; a.m_qe = in.qry_end; a.m_rs = in.ref_str; a.m_re = in.ref_end; a.m_qtot = in.qry_total;
    a.m_rng_off = in.rec_rng_off; a.m_cs_off = in.rec_cs_off; a.m_cs_text = in.cs_text; a.m_ref_chr = in.ref_chr; a.m_fwd = in.aln_fwd; a.m_mq = in.map_qul;
    a.m_rtot = cols.ref_total; a.m_mat = cols.mat_num; a.m_aln = cols.aln_len; a.m_row_index = cols.row_index; a.m_cord = cols.cord_type;
    a.m_names = cols.names; a.m_ctg_name_off = cols.ctg_name_off; a.m_chr_name_off = cols.chr_name_off;
    int64_t old_names_bytes = 0;
    be.d2h(&old_names_bytes, cols.chr_name_off + n_chr, 8);
    if (!be.ok()) return be.code();

    int64_t Ra = 0, K = 0, n_new = 0;
    std::vector<int64_t> new_end, new_pos;                           // the new reference names: their ends in `names`, their places in the alt text
    std::vector<int32_t> added;
    uint8_t *d_text = nullptr;
    if (len > 0) {
        // ---- the alt rows: framed and parsed as the main file's
        be.stage("upload");
        d_text = u8s(len);
        be.h2d(d_text, text, (size_t)len);
        a.r.text = d_text; a.r.len = len; a.r.weak_hash = (flags & AASM_READ_H_WEAK_HASH) ? 1 : 0;
        int32_t rwords[RW_N] = {INT32_MAX, 0, 0, 0};
        const int frc = read_front(be, a.r, text, false, max_blocks, rwords, true, [] {});
        if (frc < 0) return frc;
        Ra = a.r.R;
        if (frc != AASM_OK && Ra != 0) return declined(ALT_WHY_ROW, rwords[RW_FAULT] != INT32_MAX ? rwords[RW_FAULT] : 0);
        out.slow_rows = rwords[RW_SLOW];
    }
    if (Ra > 0) {
        be.stage("pieces");
        a.piece_len = i32s(Ra); a.a_ctg = i32s(Ra); a.a_chr = i32s(Ra); a.shift = i64s(Ra); a.phash = (uint64_t *)i64s(Ra); a.ratio = (double *)i64s(Ra);
        a.ghead = u8s(Ra); a.rnew = u8s(Ra); a.keep = u8s(Ra);
        int64_t *grp_off = i64s(Ra + 1), *keep_off = i64s(Ra + 1);
        a.grp_off = grp_off; a.keep_off = keep_off;
        a.fault = i64s(1); a.words = i32s(AW_N);
        int64_t fault = INT64_MAX;
        int32_t words[AW_N] = {0, 0};
        be.h2d(a.fault, &fault, 8); be.h2d(a.words, words, sizeof words);
        run(KA_PIECES, Ra);
        run(KA_HEADS, Ra);
        be.scan_u8(a.ghead, Ra, grp_off);
        be.stage("name tables");
        a.ctg_hash = (uint64_t *)i64s(C); a.chr_hash = (uint64_t *)i64s(n_chr);
        const int64_t ct_cap = cap_for(C);
        a.ct_mask = ct_cap - 1; a.ct_owner = i32s(ct_cap); a.ct_max = i32s(ct_cap);
        be.fill32(a.ct_owner, -1, ct_cap); be.fill32(a.ct_max, INT32_MAX, ct_cap);
        run(KA_CTG_HASH, C + n_chr);
        int64_t G = 0;
        be.d2h(&fault, a.fault, 8); be.d2h(words, a.words, sizeof words); be.d2h(&G, grp_off + Ra, 8);
        if (!be.ok()) return be.code();
        if (fault != INT64_MAX) return declined((int)(fault & 7), fault >> 3);   // a piece name: the first one in file order
        const int64_t rt_cap = cap_for(n_chr + words[AW_NEW]);
        a.rt_mask = rt_cap - 1; a.rt_owner = i32s(rt_cap); a.rt_min = i32s(rt_cap); a.chr_info = i64s(3 * (int64_t)words[AW_NEW]);
        be.fill32(a.rt_owner, -1, rt_cap); be.fill32(a.rt_min, INT32_MAX, rt_cap);
        run(KA_TABLES, C + n_chr);
        run(KA_REF_ROWS, Ra);
        run(KA_CHR_LIST, rt_cap);
        be.d2h(words, a.words, sizeof words);
        if (!be.ok()) return be.code();
        n_new = words[AW_CHR];
        std::vector<int64_t> info((size_t)n_new * 3);
        be.d2h(info.data(), a.chr_info, info.size() * 8);
        if (!be.ok()) return be.code();
        std::vector<int64_t> order((size_t)n_new);
        for (int64_t j = 0; j < n_new; j++) order[(size_t)j] = j;
        std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return info[(size_t)x * 3] < info[(size_t)y * 3]; });
        std::vector<int32_t> sorted((size_t)n_new);
        new_end.resize((size_t)n_new); new_pos.resize((size_t)n_new);
        int64_t end = old_names_bytes;
        for (int64_t j = 0; j < n_new; j++) {
            const int64_t *e = &info[(size_t)order[(size_t)j] * 3];
            sorted[(size_t)j] = (int32_t)e[0]; new_pos[(size_t)j] = e[1]; new_end[(size_t)j] = end += e[2];
        }
        int32_t *d_sorted = i32s(n_new);
        be.h2d(d_sorted, sorted.data(), sorted.size() * 4);
        a.chr_sorted = d_sorted; a.n_new = (int32_t)n_new;
        be.stage("lookup");
        run(KA_LOOKUP, Ra);
        be.stage("groups");
        a.g_over = i32s(G); a.g_best = i32s(G); a.g_max = i64s(G);
        be.fill32(a.g_over, 0, G); be.fill32(a.g_best, INT32_MAX, G); be.fill32(a.g_max, 0, 2 * G);
        run(KA_GROUP_MAX, Ra);
        run(KA_GROUP_BEST, Ra);
        be.stage("keep");
        run(KA_KEEP, Ra);
        be.scan_u8(a.keep, Ra, keep_off);
        be.d2h(&fault, a.fault, 8); be.d2h(&K, keep_off + Ra, 8);
        if (!be.ok()) return be.code();
        if (fault != INT64_MAX) return declined((int)(fault & 7), fault >> 3);   // a group that keeps the zeroed stand-in
        if (R + K > INT32_MAX) return declined(ALT_WHY_TOO_MANY, 0);
    }
    a.K = K;
    if (K > 0) {
        be.stage("placement");
        a.kept_row = i32s(K); a.run_head = u8s(K);
        int64_t *run_off = i64s(K + 1);
        a.run_off = run_off;
        run(KA_KEPT, Ra);
        run(KA_RUN_HEADS, K);
        be.scan_u8(a.run_head, K, run_off);
        int64_t NR = 0;
        be.d2h(&NR, run_off + K, 8);
        if (!be.ok()) return be.code();
        a.NR = NR; a.run_info = i64s(2 * NR);
        run(KA_RUNS, K);
        std::vector<int64_t> info((size_t)NR * 2), base((size_t)NR);
        be.d2h(info.data(), a.run_info, info.size() * 8);
        if (!be.ok()) return be.code();
        added.assign((size_t)C, 0);
        for (int64_t r = 0; r < NR; r++) {                            // file order: a contig's runs stay in the order of their rows
            const int64_t c = info[(size_t)r * 2], n = (r + 1 < NR ? info[(size_t)r * 2 + 3] : K) - info[(size_t)r * 2 + 1];
            base[(size_t)r] = added[(size_t)c]; added[(size_t)c] += (int32_t)n;
        }
        int64_t *d_base = i64s(NR);
        be.h2d(d_base, base.data(), base.size() * 8);
        a.run_base = d_base;
    }
    // ---- the merged batch
    be.stage("build");
    const int64_t R2 = R + K, n_chr2 = n_chr + n_new;
    int32_t *d_added = i32s(C);
    if (K > 0) be.h2d(d_added, added.data(), (size_t)C * 4); else be.fill32(d_added, 0, C);
    a.added = d_added; a.new_cnt = i32s(C);
    int64_t *new_ctg_off = i64s(C + 1), *cs_off = i64s(R2 + 1), *rng_off = i64s(R2 + 1), *d_new_pos = i64s(n_new);
    a.new_ctg_off = new_ctg_off; a.o_cs_off = cs_off; a.new_pos = d_new_pos;
    run(KA_COUNTS, C);
    be.scan_i32(a.new_cnt, C, new_ctg_off);
    a.o_qs = i64s(R2); a.o_qe = i64s(R2); a.o_rs = i64s(R2); a.o_re = i64s(R2); a.o_qtot = i64s(R2); a.o_rtot = i64s(R2); a.o_src = i64s(R2);
    a.o_ref_chr = i32s(R2); a.o_mat = i32s(R2); a.o_aln = i32s(R2); a.o_row_index = i32s(R2); a.o_tag_len = i32s(R2); a.o_colon = i32s(R2);
    a.o_fwd = u8s(R2); a.o_mq = u8s(R2); a.o_cord = u8s(R2);
    a.o_ctg_name_off = i64s(C + 1); a.o_chr_name_off = i64s(n_chr2 + 1);
    run(KA_BUILD_MAIN, R + C + n_chr + 2);
    if (K > 0) run(KA_BUILD_ALT, K);
    if (n_new > 0) { be.h2d(a.o_chr_name_off + n_chr + 1, new_end.data(), (size_t)n_new * 8); be.h2d(d_new_pos, new_pos.data(), (size_t)n_new * 8); }
    be.scan_i32(a.o_tag_len, R2, cs_off);
    be.scan_i32(a.o_colon, R2, rng_off);
    int64_t cs_bytes = 0, n_ranges = 0;
    be.d2h(&cs_bytes, cs_off + R2, 8); be.d2h(&n_ranges, rng_off + R2, 8);
    if (!be.ok()) return be.code();
    be.stage("pack");
    const int64_t names_bytes = n_new > 0 ? new_end.back() : old_names_bytes;
    a.o_cs_text = (char *)u8s(cs_bytes); a.o_names = (char *)u8s(names_bytes);
    run(KA_PACK, R2, AASM_READ_PACK_LANES);
    run(KA_NAMES, C + n_chr2, AASM_READ_PACK_LANES);
    { int64_t w = 0; be.d2h(&w, cs_off, 8); }                         // (the launches are waited for: nothing reads the alt text any more)
    if (!be.ok()) return be.code();
    out.C = C; out.R = R2; out.n_ranges = n_ranges; out.n_chr = n_chr2; out.names_bytes = names_bytes; out.kept = K;
    out.ctg_rec_off = new_ctg_off; out.qry_str = a.o_qs; out.qry_end = a.o_qe; out.ref_str = a.o_rs; out.ref_end = a.o_re; out.qry_total = a.o_qtot;
    out.rec_rng_off = rng_off; out.rec_cs_off = cs_off; out.ref_total = a.o_rtot; out.ctg_name_off = a.o_ctg_name_off; out.chr_name_off = a.o_chr_name_off;
    out.ref_chr = a.o_ref_chr; out.mat_num = a.o_mat; out.aln_len = a.o_aln; out.row_index = a.o_row_index;
    out.aln_fwd = a.o_fwd; out.map_qul = a.o_mq; out.cord_type = a.o_cord; out.cs_text = a.o_cs_text; out.names = a.o_names;
    for (void *p : alt_out_arrays(out)) be.keep(p);
    be.stage("free");
    return AASM_OK;
}

static inline void alt_out_views(const AltOut &o, aasm_batch_in &v, aasm_row_cols &c) {
    std::memset(&v, 0, sizeof v);
    v.n_contigs = o.C; v.n_records = o.R; v.n_ranges = o.n_ranges;
    v.ctg_rec_off = o.ctg_rec_off; v.qry_str = o.qry_str; v.qry_end = o.qry_end; v.ref_str = o.ref_str; v.ref_end = o.ref_end; v.qry_total = o.qry_total;
    v.ref_chr = o.ref_chr; v.aln_fwd = o.aln_fwd; v.map_qul = o.map_qul; v.rec_rng_off = o.rec_rng_off; v.cs_text = o.cs_text; v.rec_cs_off = o.rec_cs_off;
    c.n_chr = o.n_chr; c.ref_total = o.ref_total; c.mat_num = o.mat_num; c.aln_len = o.aln_len; c.row_index = o.row_index; c.cord_type = o.cord_type;
    c.names = o.names; c.ctg_name_off = o.ctg_name_off; c.chr_name_off = o.chr_name_off;
}
// AASM_ALT_DECLINED: the host's own scan of the text says whether it is bad (its code and message) or merely the host's to merge
static inline int alt_host_says(const char *text, int64_t len, const AltOut &o) {
    std::string err;
    const int rc = alt_host_verdict(text, len, err);
    if (rc != AASM_OK) { set_last_error(err); return rc; }
    set_last_error(std::string("aasm_paf_merge_alt_device: the device does not merge this alt text (") + alt_why_text(o.why) + ", alt row " + std::to_string(o.why_row) + "); merge on the host");
    return AASM_E_PARSE;
}

}  // namespace aasm
