// aasm_rows.h -- output rows on the device (aasm_rows_sizes_device / aasm_rows_format_device): kernel bodies, kernel table, launch.
//
// emit_line + put_columns (aasm_paf.cpp) for a lane: an element, its record and its cut plan become the bytes of a .aln.paf row,
//   name \t qry_total \t qs \t qe+1 \t strand \t ref name \t ref_total \t A \t B+1 \t mat \t aln \t mapq \t tp:A:x \t xi:Z:x_n \t TAG \n
// A row is made of six pieces: the name, the columns before the reference name (for .all behind the name's ".n"), the reference
// name, the columns behind it with "cs:Z:" and a shortened head run, ONE stretch of the record's own tag, and the shortened tail
// run with the line feed.  Three of them lie in device memory as they are (names, tag); the three others are a few numbers.
//   lengths  one thread per element, chunked like the cut plans (aasm_cut.h): the element's contig and path, its record, the
//            checks of emit_line, and the row's exact byte length into row_off[i + 1]; an element that cannot be formatted gets
//            length 0, is counted, and lowers the first-fault word.  The caller scans row_off in place.
//   fill     a workgroup takes AASM_ROWS_CHUNK consecutive rows: a lane per row renders the three small pieces into the row's LDS
//            slot and leaves the pieces' ends and sources beside it; then the chunk's output, one contiguous byte range, is
//            written in the FLAT form - every lane owns aligned eight-byte words of it, finds the word's row by binary search
//            over the chunk's offsets in LDS and the piece inside the row, gathers the bytes (an eight-byte load where eight are
//            left in a piece, else byte by byte) and issues one aligned store.  The bytes before the first and behind the last
//            aligned word of a chunk are written one by one, so no store carries a byte of another chunk or outside the text.
//            A row of any length is nothing special: the loop strides over the chunk's words, not over rows.
//   irregular rows (AASM_CUT_IRREGULAR: a kept ':' run that is not written as it stands) are rendered by their own lane, the
//            walk of cut_walk_lane with edit_cs's visitor, bytewise at the tag's place in the text before the chunk's copy; the
//            copy reads those bytes back behind a barrier, so every word still has one writer.
// Reads of a tag stay inside [rec_cs_off[r], rec_cs_off[r + 1]), reads of a name inside its span.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "aasm_cut.h"
#include "aasm_paf.hpp"

namespace aasm {

#define AASM_ROWS_CHUNK 128              // rows of a fill chunk
// a row's LDS slot: the three rendered pieces at fixed places, each sized for its worst case (an int64 column: sign + 19 digits,
// an int32 column: 11 characters)
#define AASM_ROWS_I64 20
#define AASM_ROWS_I32 11
#define AASM_ROWS_A_MAX (1 + AASM_ROWS_I64 + 1 + 3 * (AASM_ROWS_I64 + 1) + 2)                            // [.n] \t qtot \t qs \t qe \t s \t
#define AASM_ROWS_B_MAX (1 + 3 * (AASM_ROWS_I64 + 1) + 2 * (AASM_ROWS_I32 + 1) + 4 + 7 + 7 + AASM_ROWS_I32 + 1 + 5 + 1 + AASM_ROWS_I64)
#define AASM_ROWS_C_MAX (1 + AASM_ROWS_I64 + 1)                                                          // [:tail] \n
#define AASM_ROWS_A_AT 0
#define AASM_ROWS_B_AT 88
#define AASM_ROWS_C_AT 232
#define AASM_ROWS_SLOT 256
static_assert(AASM_ROWS_A_MAX <= AASM_ROWS_B_AT - AASM_ROWS_A_AT, "piece A outgrows its place in the slot");
static_assert(AASM_ROWS_B_MAX <= AASM_ROWS_C_AT - AASM_ROWS_B_AT, "piece B outgrows its place in the slot");
static_assert(AASM_ROWS_C_MAX <= AASM_ROWS_SLOT - AASM_ROWS_C_AT, "piece C outgrows its place in the slot");

// pieces of a row, in order; end[s]: where piece s ends inside the row, src[]: where the three global pieces start
enum { RP_NAME = 0, RP_A, RP_CHR, RP_B, RP_TAG, RP_C, RP_N };
#define AASM_ROWS_IN_PLACE INT64_MIN
struct RowsSeg {
    int64_t end[RP_N];
    int64_t src[3];                      // name, reference name: offsets into names; tag: offset into cs_text, AASM_ROWS_IN_PLACE: rendered in place
    int64_t rec;                         // the row's record
};
struct RowsLds {
    int64_t p_lo, p_hi, c_lo, c_hi;      // the chunk's search bounds, found by one thread
    int32_t bad, pad;                    // a row's length is not what row_off says: the chunk is not written
    int64_t roff[AASM_ROWS_CHUNK + 1];   // row starts relative to the chunk's first byte
    RowsSeg seg[AASM_ROWS_CHUNK];
    char slot[AASM_ROWS_CHUNK][AASM_ROWS_SLOT];
};
#define AASM_ROWS_LDS_BYTES (40 + (AASM_ROWS_CHUNK + 1) * 8 + AASM_ROWS_CHUNK * (80 + AASM_ROWS_SLOT))
static_assert(sizeof(RowsLds) <= AASM_ROWS_LDS_BYTES, "LDS budget");
static_assert(AASM_ROWS_LDS_BYTES <= 65536, "LDS budget");
struct RowsLenLds { int64_t p_lo, p_hi, c_lo, c_hi; };
#define AASM_ROWS_LEN_LDS_BYTES 32

#define AASM_ROWS_CUT_ERRORS (AASM_CUT_E_TAG | AASM_CUT_E_INS_CLIP | AASM_CUT_E_EDIT | AASM_CUT_E_RECORD)
enum { RW_FLAGGED = 0, RW_FIRST, RW_WORDS };                        // RowsArgs::words: flagged elements; the first one's key
#define AASM_ROWS_NO_KEY INT64_MAX
// list : 2 | element : 49 | flags : 12 - the smallest key is the first flagged element in file order
AASM_DEV int64_t rows_key(int l, int64_t i, int32_t flags) { return (int64_t)(((uint64_t)l << 61) | ((uint64_t)i << 12) | (uint64_t)(flags & 0xfff)); }

struct RowsArgs {
    CutArgs c;                           // the batch, the element lists and their plans (dst), chunked for the length pass
    const int64_t *qtot, *rtot;
    const int32_t *ref_chr, *mat, *aln, *row_index;
    const uint8_t *mq, *cord;
    const char *names;
    const int64_t *ctg_name_off, *chr_name_off;
    int64_t n_chr;
    int64_t *row_off[3];
    int64_t *words;                      // [RW_WORDS]
    // fill: rows [e0, e1) of list `list` into text, whose byte 0 is file offset row_off[list][e0]
    int32_t list, pad;
    int64_t e0, e1;
    char *text;
};

// ---- numbers ----------------------------------------------------------------------------------------------------------------
AASM_DEV int rows_digits(uint64_t u) {                               // decimal digits of u, by compares
    if (u >= 10000000000000000ull)
        return 17 + (u >= 100000000000000000ull) + (u >= 1000000000000000000ull) + (u >= 10000000000000000000ull);
    if (u >= 100000000ull)
        return 9 + (u >= 1000000000ull) + (u >= 10000000000ull) + (u >= 100000000000ull) + (u >= 1000000000000ull) +
               (u >= 10000000000000ull) + (u >= 100000000000000ull) + (u >= 1000000000000000ull);
    return 1 + (u >= 10ull) + (u >= 100ull) + (u >= 1000ull) + (u >= 10000ull) + (u >= 100000ull) + (u >= 1000000ull) + (u >= 10000000ull);
}
// put_i64 (aasm_paf.cpp): a sign, no padding; W: the characters go to p (straight into LDS or the text), else they are counted
template <bool W> AASM_DEV int rows_put(char *p, int64_t v) {
    uint64_t u = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    const int neg = v < 0 ? 1 : 0, nd = rows_digits(u);
    if (W) {
        if (neg) p[0] = '-';
        for (int k = nd - 1; k >= 0; k--) { p[neg + k] = (char)('0' + (int)(u % 10)); u /= 10; }
    }
    return neg + nd;
}

// ---- the irregular tag: edit_cs's walk (aasm_paf.cpp:236-252) for a lane -----------------------------------------------------------
// cut_walk_lane's loop (aasm_cut.h) with a visitor: every surviving ':' run is written as ":" + decimal(kept), every other
// surviving operation is copied as it stands.  Returns the bytes behind "cs:Z:"; W: they are written to dst.
template <bool W> AASM_DEV int64_t rows_render(const CutArgs &a, const OutElem &e, int64_t r, char *dst) {
    const int64_t p0 = a.cs_off[r], len = a.cs_off[r + 1] - p0;
    const uint8_t *cs = (const uint8_t *)a.cs_text + p0;
    CutScan s;
    s.fwd = a.fwd[r] != 0;
    s.q = s.fwd ? a.qs[r] : cut_add(a.qe[r], 1);
    s.eq_s = e.qs; s.eq_e = e.qe;
    s.val = 0; s.op0 = 0; s.q_bases = 0; s.r_bases = 0; s.keep_lo = 0; s.keep_hi = 0; s.head = 0; s.tail = 0;
    s.mat = 0; s.aln = 0; s.plen = 0; s.t = 0;
    s.ins = false; s.irregular = false; s.any = false; s.lead0 = false; s.past = false;
    s.bad = len < 5;
    int64_t n = 0;
    auto close = [&](int64_t end) {                                  // the open operation ends at byte `end`: clipped by cut_close_op
        const int64_t q0 = s.q_bases, r0 = s.r_bases, op0 = s.op0;
        const int t = s.t;
        cut_close_op(s, end);
        if (s.bad || (s.q_bases == q0 && s.r_bases == r0)) return;   // nothing of it survives
        if (t == ':') {
            if (W) dst[n] = ':';
            n++;
            n += rows_put<W>(W ? dst + n : nullptr, cut_sub(s.q_bases, q0));
        } else {
            if (W) for (int64_t j = op0; j < end; j++) dst[n + (j - op0)] = (char)cs[j];
            n += end - op0;
        }
    };
    bool stop = s.bad;
    for (int64_t pos = 5; pos < len && !stop; ) {
        int nb;
        uint64_t wd = cs_next_word(cs, pos, len, nb);
        for (int t = 0; t < nb && !stop; t++) {
            const int c = (int)(wd & 0xff);
            wd >>= 8;
            if (cs_is_op(c)) {
                if (s.t) close(pos + t);
                if (s.bad || s.past) { s.t = 0; stop = true; break; }
                s.t = c; s.op0 = pos + t; s.plen = 0; s.val = 0; s.lead0 = false;
            } else if (s.t == ':') {
                const unsigned dg = (unsigned)(c - '0');
                if (dg > 9u) { s.bad = true; stop = true; }
                else { s.val = cs_add_digit(s.val, dg); s.plen = 1; }
            } else if (s.t && cs_is_alpha(c)) s.plen++;
            else { s.bad = true; stop = true; }
        }
        pos += nb;
    }
    if (!s.bad && s.t) close(len);
    return n;
}

// ---- one row ----------------------------------------------------------------------------------------------------------------------
// emit_line's checks on element e of contig c with plan p, in its order: 0, or why the row cannot be formatted (the plan's own
// AASM_CUT_E_* flags, AASM_ROWS_E_PLAN, AASM_ROWS_E_STRETCH).  r: the record; uncut: the element spans it.
AASM_DEV int32_t rows_check(const RowsArgs &a, const OutElem &e, const aasm_cut_plan &p, int64_t c, int64_t &r, bool &uncut) {
    r = a.c.rec_off[c] + e.ctg_index;
    uncut = false;
    if (e.ctg_index < 0 || r < 0 || r >= a.c.rec_off[c + 1] || r >= a.c.R) return AASM_CUT_E_RECORD;
    if (a.ref_chr[r] < 0 || (int64_t)a.ref_chr[r] >= a.n_chr) return AASM_CUT_E_RECORD;   // (a record without a reference name: no container holds one)
    const int32_t f = p.flags;
    if (f & AASM_ROWS_CUT_ERRORS) return f & AASM_ROWS_CUT_ERRORS;
    uncut = e.qs == a.c.qs[r] && e.qe == a.c.qe[r];
    if (((f & AASM_CUT_IS_CUT) == 0) != uncut) return AASM_ROWS_E_PLAN;
    if (!uncut && !(f & AASM_CUT_IRREGULAR)) {
        const int64_t tag_len = a.c.cs_off[r + 1] - a.c.cs_off[r];
        const bool some = p.keep_lo != p.keep_hi;
        if (p.head_keep < 0 || p.tail_keep < 0 || (some && (p.keep_lo < 5 || p.keep_lo > p.keep_hi || p.keep_hi > tag_len))) return AASM_ROWS_E_STRETCH;
    }
    return 0;
}
// The row of a checked element: its length; W: the small pieces are rendered into the slot and sg says where every piece ends
// and where the global ones start.  path_no: the .all path's number inside its contig, from 1 (list 2 only).
template <bool W> AASM_DEV int64_t rows_layout(const RowsArgs &a, int l, const OutElem &e, const aasm_cut_plan &p, int64_t c, int64_t r, bool uncut,
                                               int64_t path_no, RowsSeg *sg, char *slot) {
    const bool fwd = a.c.fwd[r] != 0;
    const int64_t name0 = a.ctg_name_off[c], name_len = a.ctg_name_off[c + 1] - name0;
    const int64_t chr0 = a.chr_name_off[a.ref_chr[r]], chr_len = a.chr_name_off[a.ref_chr[r] + 1] - chr0;
    char *A = W ? slot + AASM_ROWS_A_AT : nullptr, *B = W ? slot + AASM_ROWS_B_AT : nullptr, *Cp = W ? slot + AASM_ROWS_C_AT : nullptr;
    int na = 0, nb = 0, nc = 0;
#define ROWS_CH(buf, n, ch) do { if (W) (buf)[n] = (ch); (n)++; } while (0)
    if (l == 2) { ROWS_CH(A, na, '.'); na += rows_put<W>(W ? A + na : nullptr, path_no); }
    ROWS_CH(A, na, '\t');
    na += rows_put<W>(W ? A + na : nullptr, a.qtot[r]); ROWS_CH(A, na, '\t');
    na += rows_put<W>(W ? A + na : nullptr, e.qs); ROWS_CH(A, na, '\t');
    na += rows_put<W>(W ? A + na : nullptr, cut_add(e.qe, 1)); ROWS_CH(A, na, '\t');
    ROWS_CH(A, na, fwd ? '+' : '-'); ROWS_CH(A, na, '\t');
    const int32_t mat = uncut ? a.mat[r] : p.mat_num, aln = uncut ? a.aln[r] : p.aln_len;
    ROWS_CH(B, nb, '\t');
    nb += rows_put<W>(W ? B + nb : nullptr, a.rtot[r]); ROWS_CH(B, nb, '\t');
    nb += rows_put<W>(W ? B + nb : nullptr, fwd ? e.rs : e.re); ROWS_CH(B, nb, '\t');
    nb += rows_put<W>(W ? B + nb : nullptr, cut_add(fwd ? e.re : e.rs, 1)); ROWS_CH(B, nb, '\t');
    nb += rows_put<W>(W ? B + nb : nullptr, mat); ROWS_CH(B, nb, '\t');
    nb += rows_put<W>(W ? B + nb : nullptr, aln); ROWS_CH(B, nb, '\t');
    nb += rows_put<W>(W ? B + nb : nullptr, a.mq[r]); ROWS_CH(B, nb, '\t');
    ROWS_CH(B, nb, 't'); ROWS_CH(B, nb, 'p'); ROWS_CH(B, nb, ':'); ROWS_CH(B, nb, 'A'); ROWS_CH(B, nb, ':'); ROWS_CH(B, nb, e.is_alt ? 'S' : 'P'); ROWS_CH(B, nb, '\t');
    ROWS_CH(B, nb, 'x'); ROWS_CH(B, nb, 'i'); ROWS_CH(B, nb, ':'); ROWS_CH(B, nb, 'Z'); ROWS_CH(B, nb, ':'); ROWS_CH(B, nb, a.cord[r] == 0 ? 'P' : 'A'); ROWS_CH(B, nb, '_');
    nb += rows_put<W>(W ? B + nb : nullptr, a.row_index[r]); ROWS_CH(B, nb, '\t');
    int64_t tag_src = a.c.cs_off[r], tag_len = a.c.cs_off[r + 1] - a.c.cs_off[r];
    if (!uncut) {
        ROWS_CH(B, nb, 'c'); ROWS_CH(B, nb, 's'); ROWS_CH(B, nb, ':'); ROWS_CH(B, nb, 'Z'); ROWS_CH(B, nb, ':');
        if (p.flags & AASM_CUT_IRREGULAR) { tag_src = AASM_ROWS_IN_PLACE; tag_len = rows_render<false>(a.c, e, r, nullptr); }
        else {
            if (p.head_keep) { ROWS_CH(B, nb, ':'); nb += rows_put<W>(W ? B + nb : nullptr, p.head_keep); }
            tag_src += p.keep_lo; tag_len = p.keep_hi - p.keep_lo;
            if (p.tail_keep) { ROWS_CH(Cp, nc, ':'); nc += rows_put<W>(W ? Cp + nc : nullptr, p.tail_keep); }
        }
    }
    ROWS_CH(Cp, nc, '\n');
#undef ROWS_CH
    const int64_t total = name_len + na + chr_len + nb + tag_len + nc;
    if (W) {
        sg->end[RP_NAME] = name_len; sg->end[RP_A] = name_len + na; sg->end[RP_CHR] = sg->end[RP_A] + chr_len; sg->end[RP_B] = sg->end[RP_CHR] + nb;
        sg->end[RP_TAG] = sg->end[RP_B] + tag_len; sg->end[RP_C] = total;
        sg->src[0] = name0; sg->src[1] = chr0; sg->src[2] = tag_src; sg->rec = r;
    }
    return total;
}

// the chunk's search bounds (kb_cut_plan's): the contigs - for .all the paths, then the contigs - of its first and last element
AASM_DEV void rows_bounds(const CutArgs &a, int l, int64_t g0, int64_t n, int64_t &p_lo, int64_t &p_hi, int64_t &c_lo, int64_t &c_hi) {
    p_lo = 0; p_hi = 0;
    if (l == 2) {
        p_lo = cut_owner(a.off[2], 0, a.NP - 1, g0); p_hi = cut_owner(a.off[2], p_lo, a.NP - 1, g0 + n - 1);
        c_lo = cut_owner(a.path_off, 0, a.C - 1, p_lo); c_hi = cut_owner(a.path_off, c_lo, a.C - 1, p_hi);
    } else {
        c_lo = cut_owner(a.off[l], 0, a.C - 1, g0); c_hi = cut_owner(a.off[l], c_lo, a.C - 1, g0 + n - 1);
    }
}
// contig of element g of list l, and for .all the number of its path inside the contig
AASM_DEV int64_t rows_owner(const CutArgs &a, int l, int64_t g, int64_t p_lo, int64_t p_hi, int64_t c_lo, int64_t c_hi, int64_t &path_no) {
    path_no = 0;
    if (l != 2) return cut_owner(a.off[l], c_lo, c_hi, g);
    const int64_t pth = cut_owner(a.off[2], p_lo, p_hi, g), c = cut_owner(a.path_off, c_lo, c_hi, pth);
    path_no = pth - a.path_off[c] + 1;
    return c;
}

// ---- length pass: a workgroup per chunk of AASM_CUT_CHUNK elements of one list (grid-stride), a thread per element ----
AASM_DEV void kb_rows_len(const KCtx &k, const RowsArgs &a) {
    RowsLenLds *L = (RowsLenLds *)k.lds;
    for (int64_t ch = k.bid; ch < a.c.ch0[3]; ch += k.nblocks) {
        const int l = ch >= a.c.ch0[2] ? 2 : ch >= a.c.ch0[1] ? 1 : 0;
        const int64_t g0 = (ch - a.c.ch0[l]) * AASM_CUT_CHUNK;
        const int64_t n = a.c.n[l] - g0 < AASM_CUT_CHUNK ? a.c.n[l] - g0 : AASM_CUT_CHUNK;
        if (k.tid == 0) rows_bounds(a.c, l, g0, n, L->p_lo, L->p_hi, L->c_lo, L->c_hi);
        block_barrier();
        const int64_t p_lo = L->p_lo, p_hi = L->p_hi, c_lo = L->c_lo, c_hi = L->c_hi;
        for (int64_t i = k.tid; i < n; i += k.nthreads) {
            const int64_t g = g0 + i;
            const OutElem e = a.c.el[l][g];
            const aasm_cut_plan p = a.c.dst[l][g];
            int64_t path_no, r;
            bool uncut;
            const int64_t c = rows_owner(a.c, l, g, p_lo, p_hi, c_lo, c_hi, path_no);
            const int32_t bad = rows_check(a, e, p, c, r, uncut);
            int64_t len = 0;
            if (bad) { atomic_add(&a.words[RW_FLAGGED], (int64_t)1); atomic_min_i64(&a.words[RW_FIRST], rows_key(l, g, bad)); }
            else len = rows_layout<false>(a, l, e, p, c, r, uncut, path_no, nullptr, nullptr);
            a.row_off[l][g + 1] = len;
        }
        block_barrier();                                             // (the bounds are the next chunk's from here on)
    }
}

// ---- fill ---------------------------------------------------------------------------------------------------------------------------
AASM_DEV uint64_t rows_load8(const uint8_t *p) { uint64_t w; __builtin_memcpy(&w, p, 8); return w; }
// `want` <= 8 bytes of the chunk's output from byte d of it on, first byte lowest.  n: rows of the chunk; out: the chunk's place in
// the text (an irregular tag is read back from there).
AASM_DEV uint64_t rows_gather(const RowsArgs &a, const RowsLds *L, int n, int64_t d, int want, const char *out) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = lo + ((hi - lo + 1) >> 1);
        if (L->roff[mid] <= d) lo = mid; else hi = mid - 1;
    }
    int row = lo, got = 0;
    int64_t o = d - L->roff[row];
    uint64_t v = 0;
    while (got < want && row < n) {
        const RowsSeg &sg = L->seg[row];
        int s = 0;
        while (s < RP_C && o >= sg.end[s]) s++;
        const int64_t in = o - (s ? sg.end[s - 1] : 0), left = sg.end[s] - o;
        const int take = (int)(left < want - got ? left : want - got);
        uint64_t w = 0;
        if (s == RP_A || s == RP_B || s == RP_C) {
            const char *p = L->slot[row] + (s == RP_A ? AASM_ROWS_A_AT : s == RP_B ? AASM_ROWS_B_AT : AASM_ROWS_C_AT) + in;
            for (int t = 0; t < take; t++) w |= (uint64_t)(uint8_t)p[t] << (8 * t);
        } else {
            const uint8_t *p = s == RP_NAME ? (const uint8_t *)a.names + sg.src[0] + in
                               : s == RP_CHR ? (const uint8_t *)a.names + sg.src[1] + in
                               : sg.src[2] != AASM_ROWS_IN_PLACE ? (const uint8_t *)a.c.cs_text + sg.src[2] + in
                                                : (const uint8_t *)out + L->roff[row] + o;
            if (take == 8) w = rows_load8(p);                        // (only where eight bytes are left in the piece)
            else for (int t = 0; t < take; t++) w |= (uint64_t)p[t] << (8 * t);
        }
        v |= w << (8 * got);
        got += take; o += take;
        if (o >= sg.end[RP_C]) { row++; o = 0; }
    }
    return v;
}
AASM_DEV void kb_rows_fill(const KCtx &k, const RowsArgs &a) {
    RowsLds *L = (RowsLds *)k.lds;
    const int l = a.list;
    const int64_t *roff = a.row_off[l];
    const int64_t n_ch = (a.e1 - a.e0 + AASM_ROWS_CHUNK - 1) / AASM_ROWS_CHUNK, base = a.e1 > a.e0 ? roff[a.e0] : 0;
    for (int64_t ch = k.bid; ch < n_ch; ch += k.nblocks) {
        const int64_t g0 = a.e0 + ch * AASM_ROWS_CHUNK;
        const int n = (int)(a.e1 - g0 < AASM_ROWS_CHUNK ? a.e1 - g0 : AASM_ROWS_CHUNK);
        const int64_t first = roff[g0];
        if (k.tid == 0) { rows_bounds(a.c, l, g0, n, L->p_lo, L->p_hi, L->c_lo, L->c_hi); L->bad = 0; }
        for (int i = k.tid; i <= n; i += k.nthreads) L->roff[i] = roff[g0 + i] - first;
        block_barrier();
        const int64_t p_lo = L->p_lo, p_hi = L->p_hi, c_lo = L->c_lo, c_hi = L->c_hi;
        // a lane per row: the small pieces into the row's slot
        for (int i = k.tid; i < n; i += k.nthreads) {
            const int64_t g = g0 + i;
            const OutElem e = a.c.el[l][g];
            const aasm_cut_plan p = a.c.dst[l][g];
            int64_t path_no, r;
            bool uncut;
            const int64_t c = rows_owner(a.c, l, g, p_lo, p_hi, c_lo, c_hi, path_no);
            int64_t len = -1;
            if (!rows_check(a, e, p, c, r, uncut)) len = rows_layout<true>(a, l, e, p, c, r, uncut, path_no, &L->seg[i], L->slot[i]);
            if (len != L->roff[i + 1] - L->roff[i]) L->bad = 1;      // (row_off is not this result's: nothing of the chunk is written)
        }
        block_barrier();
        if (!L->bad) {
            char *out = a.text + (first - base);
            // irregular tags, by their row's lane, at their place in the text
            for (int i = k.tid; i < n; i += k.nthreads)
                if (L->seg[i].src[2] == AASM_ROWS_IN_PLACE) rows_render<true>(a.c, a.c.el[l][g0 + i], L->seg[i].rec, out + L->roff[i] + L->seg[i].end[RP_B]);
            block_barrier();
            // the chunk's bytes: aligned eight-byte words, one lane each; the bytes before and behind them one by one
            const int64_t nbytes = L->roff[n];
            int64_t head = (int64_t)((8 - ((uintptr_t)out & 7)) & 7);
            if (head > nbytes) head = nbytes;
            const int64_t words = (nbytes - head) >> 3, tail0 = head + words * 8;
            for (int64_t w = k.tid; w < words; w += k.nthreads) {
                const uint64_t v = rows_gather(a, L, n, head + w * 8, 8, out);
                *(uint64_t *)(out + head + w * 8) = v;
            }
            for (int64_t j = k.tid; j < head + (nbytes - tail0); j += k.nthreads) {
                const int64_t d = j < head ? j : tail0 + (j - head);
                out[d] = (char)rows_gather(a, L, n, d, 1, out);
            }
        }
        block_barrier();                                             // (the slots are the next chunk's from here on)
    }
}

// The rows kernels (row shapes: aasm_dev.h), body called as body(k, a).  All rows are KL rows (AASM_CUT_KERNELS' expansion).
// One lane per block in the host emulation: the bodies' barriers need the block's threads one after the other.
#define AASM_ROWS_ROWS(KL) \
    KL(KW_LEN, aasm_rows_len, 256, 1, AASM_ROWS_LEN_LDS_BYTES, 0, kb_rows_len) \
    KL(KW_FILL, aasm_rows_fill, 256, 1, AASM_ROWS_LDS_BYTES, 0, kb_rows_fill)
#define AASM_ROWS_KERNELS(...) AASM_ROWS_ROWS(AASM_CUT_SECOND(__VA_ARGS__, __VA_ARGS__))
enum RowsKern { AASM_ROWS_KERNELS(AASM_ROW_ID, AASM_ROW_ID) };
constexpr int rows_block[] = {AASM_ROWS_KERNELS(AASM_ROW_BLOCK, AASM_ROW_BLOCK)};
AASM_KERNEL_BODY(run_rows_body, AASM_ROWS_KERNELS, RowsArgs)
#define AASM_ROWS_MAX_BLOCKS 4096        // the length pass: as the cut plans
#define AASM_ROWS_FILL_BLOCKS 2048       // the fill: three workgroups of 44 KB LDS per CU, a few rounds of them

// ---- host side, shared by the product (aasm_gpu.hip) and the emulation (tests/host_emul/rows_emul.cpp) ---------------------------
// The arguments of a call whose arrays the caller has checked; false: the sizes do not fit the batch.
static inline bool rows_args(const aasm_batch_in &in, const aasm_row_cols &cols, const aasm_out_sizes &sz, const aasm_dev_out &o, const aasm_dev_cuts &d,
                             const aasm_dev_rows &ro, RowsArgs &a) {
    std::memset(&a, 0, sizeof a);
    if (!cut_args(in, sz, o, d, a.c) || cols.n_chr < 0) return false;
    a.qtot = in.qry_total; a.ref_chr = in.ref_chr; a.mq = in.map_qul;
    a.rtot = cols.ref_total; a.mat = cols.mat_num; a.aln = cols.aln_len; a.row_index = cols.row_index; a.cord = cols.cord_type;
    a.names = cols.names; a.ctg_name_off = cols.ctg_name_off; a.chr_name_off = cols.chr_name_off; a.n_chr = cols.n_chr;
    a.row_off[0] = ro.main_off; a.row_off[1] = ro.alt_off; a.row_off[2] = ro.all_off;
    return true;
}
static inline int64_t rows_grid_cap(int flags, int64_t cap) { return (flags & AASM_ROWS_H_FEW_BLOCKS) ? 3 : cap; }
// backends provide launch_rows(kernel, blocks, threads, RowsArgs)
template <class B> void rows_launch_len(B &be, const RowsArgs &a, int flags) {
    if (a.c.ch0[3] > 0) be.launch_rows(KW_LEN, std::min<int64_t>(a.c.ch0[3], rows_grid_cap(flags, AASM_ROWS_MAX_BLOCKS)), rows_block[KW_LEN], a);
}
template <class B> void rows_launch_fill(B &be, RowsArgs a, int list, int64_t e0, int64_t e1, char *text, int flags) {
    a.list = list; a.e0 = e0; a.e1 = e1; a.text = text;
    const int64_t n_ch = (e1 - e0 + AASM_ROWS_CHUNK - 1) / AASM_ROWS_CHUNK;
    if (n_ch > 0) be.launch_rows(KW_FILL, std::min<int64_t>(n_ch, rows_grid_cap(flags, AASM_ROWS_FILL_BLOCKS)), rows_block[KW_FILL], a);
}
// what the length pass left in words[] as the caller's info (bytes[] are the scans' totals, set by the caller)
static inline void rows_info_of(const int64_t words[RW_WORDS], aasm_rows_info &info) {
    info.n_flagged = words[RW_FLAGGED];
    info.bad_elem = -1; info.bad_list = 0; info.bad_flags = 0;
    if (words[RW_FLAGGED] > 0 && words[RW_FIRST] != AASM_ROWS_NO_KEY) {
        const uint64_t key = (uint64_t)words[RW_FIRST];
        info.bad_list = (int32_t)(key >> 61); info.bad_elem = (int64_t)((key >> 12) & (((uint64_t)1 << 49) - 1)); info.bad_flags = (int32_t)(key & 0xfff);
    }
}
// aasm_rows_format_device's range check: nullptr, or why the call is refused
static inline const char *rows_format_refusal(const RowsArgs &a, const aasm_rows_info &info, int list, int64_t e0, int64_t e1) {
    if (info.n_flagged != 0) return "the result holds elements that cannot be formatted (aasm_rows_info.n_flagged)";
    if (list < 0 || list > 2) return "list is not 0 (main), 1 (alt) or 2 (all)";
    if (e0 < 0 || e0 > e1 || e1 > a.c.n[list]) return "[e0, e1) is no range of the list's elements";
    return nullptr;
}

// ---- aasm_writer_append_device's pieces ------------------------------------------------------------------------------------------
struct RowsPiece { int list; int64_t e0, e1, b0, b1; };              // rows [e0, e1) of a list, bytes [b0, b1) of its text
#define AASM_ROWS_SAMPLE 1024            // piece cut points are looked for among every 1024th row offset first
// The pieces of one list of n rows and `total` bytes: runs of rows of at most `limit` bytes (a longer row alone), cut at sampled
// offsets where that will do and at single rows inside a block of samples that is too large.  fetch(first, stride, count, dst)
// reads row_off[first + k * stride], k < count, into dst (the product: copies from the device); false: a fetch failed.
template <class F> bool rows_cut_pieces(F &&fetch, int64_t n, int64_t total, int list, int64_t limit, std::vector<RowsPiece> &out) {
    if (n <= 0) return true;
    const int64_t ns = n / AASM_ROWS_SAMPLE;                         // samples 0, S, 2 S, .. ns S; then n itself
    std::vector<int64_t> at, off((size_t)ns + 1);
    if (!fetch((int64_t)0, (int64_t)AASM_ROWS_SAMPLE, ns + 1, off.data())) return false;
    for (int64_t j = 0; j <= ns; j++) at.push_back(j * AASM_ROWS_SAMPLE);
    if (at.back() != n) { at.push_back(n); off.push_back(total); }
    std::vector<int64_t> fine;
    size_t cur = 0;
    while (cur + 1 < at.size()) {
        size_t j = cur + 1;
        while (j + 1 < at.size() && off[j + 1] - off[cur] <= limit) j++;
        if (off[j] - off[cur] <= limit || at[j] - at[cur] == 1) { out.push_back({list, at[cur], at[j], off[cur], off[j]}); cur = j; continue; }
        // one block of samples beyond the limit: its rows' own offsets
        const int64_t e0 = at[cur], m = at[j] - e0;
        fine.resize((size_t)m + 1);
        if (!fetch(e0, (int64_t)1, m + 1, fine.data())) return false;
        for (int64_t x = 0; x < m; ) {
            int64_t y = x + 1;
            while (y < m && fine[(size_t)y + 1] - fine[(size_t)x] <= limit) y++;
            out.push_back({list, e0 + x, e0 + y, fine[(size_t)x], fine[(size_t)y]});
            x = y;
        }
        cur = j;
    }
    return true;
}

// What an output row prints beyond aasm_batch_in, for contigs [c0, c1) of a container, as host arrays in aasm_row_cols' layout
struct RowsHostCols {
    std::vector<int64_t> ref_total, ctg_name_off, chr_name_off;
    std::vector<int32_t> mat_num, aln_len, row_index;
    std::vector<uint8_t> cord_type;
    std::string names;
};
static inline bool rows_host_cols(const aasm_paf &paf, int64_t c0, int64_t c1, RowsHostCols &h) {
    if (c0 < 0 || c0 >= c1 || c1 > paf.n_contigs()) return false;
    const int64_t r0 = paf.ctg_rec_off[(size_t)c0], r1 = paf.ctg_rec_off[(size_t)c1];
    h.ref_total.assign(paf.ref_total.begin() + r0, paf.ref_total.begin() + r1);
    h.mat_num.assign(paf.mat_num.begin() + r0, paf.mat_num.begin() + r1);
    h.aln_len.assign(paf.aln_len.begin() + r0, paf.aln_len.begin() + r1);
    h.row_index.assign(paf.row_index.begin() + r0, paf.row_index.begin() + r1);
    h.cord_type.assign(paf.cord_type.begin() + r0, paf.cord_type.begin() + r1);
    h.names.clear(); h.ctg_name_off.assign(1, 0); h.chr_name_off.clear();
    for (int64_t c = c0; c < c1; c++) { h.names += paf.ctg_name[(size_t)c]; h.ctg_name_off.push_back((int64_t)h.names.size()); }
    h.chr_name_off.push_back((int64_t)h.names.size());
    for (const std::string &s : paf.chr_name) { h.names += s; h.chr_name_off.push_back((int64_t)h.names.size()); }
    return true;
}

}  // namespace aasm
