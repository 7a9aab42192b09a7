// aasm_cut.h -- cut plans of exported results (aasm_cut_plans_device): kernel body, kernel table, launch.
//
// get_edited_paf_data (paf_data.cpp:125-220) without the text: the host codec's cut_walk + plan_cut (aasm_paf.cpp) restated for a
// lane.  What a re-cut keeps of a record's tag is one stretch of whole operations between at most two shortened ':' runs, so an
// element's plan is six numbers (aasm_cut_plan) and the row's writer copies the stretch.
//
// The entry is a pure function over the caller's device arrays: it may not allocate, so there is no global list of the re-cut
// elements.  A workgroup takes a chunk of AASM_CUT_CHUNK consecutive elements of one list instead and does both steps on it:
//   classify  every lane takes elements at copy speed: finds the element's contig (a search between the contigs of the chunk's
//             first and last element, found once), compares the element with its record, writes the zero plan of an element that
//             spans the whole record (two thirds of a result) and leaves the chunk-relative index and the record of a re-cut one
//             in an LDS list, compacted by ballot + prefix count;
//   walk      lane j takes entry j of the list, so the walking waves are full whatever the mix (the last one of a chunk apart).
//             One lane per tag, K0's tokenizer state machine (aasm_kernels.h, kb_cs_ranges: eight bytes per load; a
//             wave-cooperative parse of one tag was 6x slower there).  Every closed operation is clipped against
//             [edited_qry_str, edited_qry_end]; the walk ends once the cursor has left that interval - nothing behind it can be
//             kept, and the final checks only involve what was kept.
// Reads of a tag stay inside [rec_cs_off[r], rec_cs_off[r + 1]): the eight-byte load is taken only where eight bytes are left.
#pragma once
#include <algorithm>
#include "aasm_dev.h"
#include "../../include/alignasm_amd.h"

namespace aasm {

#define AASM_CUT_CHUNK 2048
struct CutLds {
    int32_t n_cut, pad;
    int64_t p_lo, p_hi, c_lo, c_hi;      // the chunk's search bounds, found by one thread
    int64_t rec[AASM_CUT_CHUNK];
    int32_t idx[AASM_CUT_CHUNK];
};
#define AASM_CUT_LDS_BYTES (40 + AASM_CUT_CHUNK * 12)
static_assert(sizeof(CutLds) <= AASM_CUT_LDS_BYTES, "LDS budget");
static_assert(sizeof(aasm_cut_plan) == 48, "layout");

// list l: 0 main, 1 alt, 2 .all
struct CutArgs {
    int64_t C, R, NP;
    const int64_t *rec_off, *qs, *qe, *cs_off;
    const uint8_t *fwd;
    const char *cs_text;
    int64_t n[3];                        // elements of list l
    int64_t ch0[4];                      // list l owns the chunks [ch0[l], ch0[l + 1])
    const OutElem *el[3];
    const int64_t *off[3];               // main_off, alt_off (per contig), all_elem_off (per path)
    const int64_t *path_off;             // all_path_off
    aasm_cut_plan *dst[3];
};

// the largest i in [lo, hi] with off[i] <= g (lo where there is none): the owner of item g under the offsets off
AASM_DEV int64_t cut_owner(const int64_t *off, int64_t lo, int64_t hi, int64_t g) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo + 1) >> 1);
        if (off[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}
AASM_DEV void cut_store(aasm_cut_plan *p, int64_t keep_lo, int64_t keep_hi, int64_t head, int64_t tail, int32_t mat, int32_t aln, int32_t flags) {
    int64_t *w = (int64_t *)p;           // (48 bytes at an 8-byte aligned address: six words)
    w[0] = keep_lo; w[1] = keep_hi; w[2] = head; w[3] = tail; w[4] = (int64_t)mk64(mat, aln); w[5] = (int64_t)(uint32_t)flags;
}
// int64 sums that wrap where the host's overflow (a run length near 2^63 that the coordinates cannot hold)
AASM_DEV int64_t cut_add(int64_t a, int64_t b) { return (int64_t)((uint64_t)a + (uint64_t)b); }
AASM_DEV int64_t cut_sub(int64_t a, int64_t b) { return (int64_t)((uint64_t)a - (uint64_t)b); }

struct CutScan {
    int64_t q;                           // CsCursor::q: fwd the next query base, '-' strand the exclusive upper end of what is left
    int64_t val, op0;                    // open ':' run: its value (-1: beyond int64); byte offset of the open operation in the tag
    int64_t eq_s, eq_e, q_bases, r_bases, keep_lo, keep_hi, head, tail;
    uint32_t mat, aln;                   // (the host's int32 counters: they wrap)
    int32_t plen;
    int t;                               // open operation (its character), 0: none
    bool fwd, bad, ins, irregular, any, lead0, past;
};
// plan_cut's visitor for an operation kept whole, text [op0, end)
AASM_DEV void cut_keep_whole(CutScan &s, int64_t end) {
    if (s.t == ':' && s.lead0) s.irregular = true;                  // ":007" comes out as ":7"
    if (s.tail) s.irregular = true;
    if (s.keep_lo == s.keep_hi) { s.keep_lo = s.op0; s.keep_hi = end; }
    else if (s.op0 == s.keep_hi) s.keep_hi = end;
    else s.irregular = true;
    s.any = true;
}
// the open operation is complete, its text ends at byte `end`: cut_walk's visitor (aasm_paf.cpp)
AASM_DEV void cut_close_op(CutScan &s, int64_t end) {
    int64_t n;
    if (s.t == ':') { if (s.plen < 1 || s.val <= 0) { s.bad = true; return; } n = s.val; }
    else if (s.t == '*') { if (s.plen != 2) { s.bad = true; return; } n = 1; }
    else { if (s.plen < 1) { s.bad = true; return; } n = s.plen; }
    if (s.t == '-') {                                                // between query bases: kept when both neighbours stay (:171-177)
        if (s.eq_s < s.q && s.q <= s.eq_e) { cut_keep_whole(s, end); s.r_bases = cut_add(s.r_bases, n); s.aln += (uint32_t)n; }
        return;
    }
    const int64_t lo = s.fwd ? s.q : cut_sub(s.q, n), hi = cut_add(lo, n - 1);
    const int64_t a = lo > s.eq_s ? lo : s.eq_s, b = hi < s.eq_e ? hi : s.eq_e;
    s.q = s.fwd ? cut_add(s.q, n) : lo;
    s.past = s.fwd ? s.q > s.eq_e : s.q <= s.eq_s;                   // nothing behind this operation can be kept
    if (a > b) return;
    if (s.t == ':') {                                                // :144-152
        const int64_t kept = b - a + 1;
        if (kept < n) {                                              // a shortened run: the first or the last one kept
            if (!s.any) { s.head = kept; s.any = true; }
            else if (!s.tail) s.tail = kept;
            else s.irregular = true;
        } else cut_keep_whole(s, end);
        s.mat += (uint32_t)kept; s.aln += (uint32_t)kept; s.q_bases = cut_add(s.q_bases, kept); s.r_bases = cut_add(s.r_bases, kept);
    } else if (s.t == '+') {                                         // :153-164: all of it or an error
        if (a != lo || b != hi) { s.ins = true; return; }
        cut_keep_whole(s, end); s.q_bases = cut_add(s.q_bases, n); s.aln += (uint32_t)n;
    } else {                                                         // '*', :165-170
        cut_keep_whole(s, end); s.q_bases += 1; s.r_bases += 1; s.aln += 1;
    }
}
// the plan of element e of record r (an element that does not span the record)
AASM_DEV void cut_walk_lane(const CutArgs &a, const OutElem &e, int64_t r, aasm_cut_plan *dst) {
    const int64_t p0 = a.cs_off[r], len = a.cs_off[r + 1] - p0;
    const uint8_t *cs = (const uint8_t *)a.cs_text + p0;
    CutScan s;
    s.fwd = a.fwd[r] != 0;
    s.q = s.fwd ? a.qs[r] : cut_add(a.qe[r], 1);
    s.eq_s = e.qs; s.eq_e = e.qe;
    s.val = 0; s.op0 = 0; s.q_bases = 0; s.r_bases = 0; s.keep_lo = 0; s.keep_hi = 0; s.head = 0; s.tail = 0;
    s.mat = 0; s.aln = 0; s.plen = 0; s.t = 0;
    s.ins = false; s.irregular = false; s.any = false; s.lead0 = false; s.past = false;
    s.bad = len < 5 || cs[0] != 'c' || cs[1] != 's' || cs[2] != ':' || cs[3] != 'Z' || cs[4] != ':';
    bool stop = s.bad;
    for (int64_t pos = 5; pos < len && !stop; ) {
        int nb;
        uint64_t wd = cs_next_word(cs, pos, len, nb);                // the next <= 8 bytes, first byte lowest (K0's loader)
        for (int t = 0; t < nb && !stop; t++) {
            const int c = (int)(wd & 0xff);
            wd >>= 8;
            if (cs_is_op(c)) {
                if (s.t) cut_close_op(s, pos + t);
                if (s.bad || s.past) { s.t = 0; stop = true; break; }
                s.t = c; s.op0 = pos + t; s.plen = 0; s.val = 0; s.lead0 = false;
            } else if (s.t == ':') {
                const unsigned dg = (unsigned)(c - '0');
                if (dg > 9u) { s.bad = true; stop = true; }
                else {
                    if (!s.plen) s.lead0 = dg == 0;
                    s.val = cs_add_digit(s.val, dg); s.plen = 1;
                }
            } else if (s.t && cs_is_alpha(c)) s.plen++;
            else { s.bad = true; stop = true; }                      // not a cs character, or payload before any operation
        }
        pos += nb;
    }
    if (!s.bad && s.t) cut_close_op(s, len);
    int32_t err = 0;
    if (s.bad) err = AASM_CUT_E_TAG;
    else if (s.ins) err = AASM_CUT_E_INS_CLIP;
    else {                                                           // :209-218
        const int64_t dr = cut_sub(e.re, e.rs), want_r = cut_add(dr < 0 ? cut_sub(0, dr) : dr, 1);
        if (s.q_bases != cut_add(cut_sub(s.eq_e, s.eq_s), 1) || s.r_bases != want_r) err = AASM_CUT_E_EDIT;
    }
    if (err) cut_store(dst, 0, 0, 0, 0, 0, 0, AASM_CUT_IS_CUT | err);
    else cut_store(dst, s.keep_lo, s.keep_hi, s.head, s.tail, (int32_t)s.mat, (int32_t)s.aln, AASM_CUT_IS_CUT | (s.irregular ? AASM_CUT_IRREGULAR : 0));
}

// A workgroup per chunk of one list's elements (grid-stride over the chunks): classify, then walk from the LDS list.
AASM_DEV void kb_cut_plan(const KCtx &k, const CutArgs &a) {
    CutLds *L = (CutLds *)k.lds;
    for (int64_t ch = k.bid; ch < a.ch0[3]; ch += k.nblocks) {
        const int l = ch >= a.ch0[2] ? 2 : ch >= a.ch0[1] ? 1 : 0;
        const int64_t g0 = (ch - a.ch0[l]) * AASM_CUT_CHUNK;
        const int64_t n = a.n[l] - g0 < AASM_CUT_CHUNK ? a.n[l] - g0 : AASM_CUT_CHUNK;
        const OutElem *el = a.el[l] + g0;
        aasm_cut_plan *dst = a.dst[l] + g0;
        // the contigs (for .all: the paths, then the contigs) of the chunk's first and last element bound every lane's search:
        // one thread finds them, the block reads them from LDS
        if (k.tid == 0) {
            int64_t p_lo = 0, p_hi = 0, c_lo, c_hi;
            if (l == 2) {
                p_lo = cut_owner(a.off[2], 0, a.NP - 1, g0); p_hi = cut_owner(a.off[2], p_lo, a.NP - 1, g0 + n - 1);
                c_lo = cut_owner(a.path_off, 0, a.C - 1, p_lo); c_hi = cut_owner(a.path_off, c_lo, a.C - 1, p_hi);
            } else {
                c_lo = cut_owner(a.off[l], 0, a.C - 1, g0); c_hi = cut_owner(a.off[l], c_lo, a.C - 1, g0 + n - 1);
            }
            L->p_lo = p_lo; L->p_hi = p_hi; L->c_lo = c_lo; L->c_hi = c_hi; L->n_cut = 0;
        }
        block_barrier();
        const int64_t p_lo = L->p_lo, p_hi = L->p_hi, c_lo = L->c_lo, c_hi = L->c_hi;
        for (int64_t base = 0; base < n; base += k.nthreads) {
            const int64_t i = base + k.tid;
            bool cut = false;
            int64_t r = -1;
            if (i < n) {
                const int64_t e_qs = el[i].qs, e_qe = el[i].qe;
                const int32_t ci = el[i].ctg_index;
                const int64_t c = l == 2 ? cut_owner(a.path_off, c_lo, c_hi, cut_owner(a.off[2], p_lo, p_hi, g0 + i)) : cut_owner(a.off[l], c_lo, c_hi, g0 + i);
                r = a.rec_off[c] + ci;
                if (ci < 0 || r < 0 || r >= a.rec_off[c + 1] || r >= a.R) cut_store(dst + i, 0, 0, 0, 0, 0, 0, AASM_CUT_E_RECORD);
                else if (e_qs == a.qs[r] && e_qe == a.qe[r]) cut_store(dst + i, 0, 0, 0, 0, 0, 0, 0);   // not cut: the record's own tag (:131-136)
                else cut = true;
            }
            const uint64_t m = wave_ballot(cut);
            int32_t wbase = 0;
            if (k.lane == 0 && m) wbase = atomic_add(&L->n_cut, (int32_t)popc64(m));
            wbase = wave_bcast(wbase, 0);
            if (cut) {
                const int32_t j = wbase + popc64(m & lanemask_lt(k.lane));
                L->idx[j] = (int32_t)i; L->rec[j] = r;
            }
        }
        block_barrier();
        const int32_t nc = L->n_cut;
        for (int32_t j = k.tid; j < nc; j += k.nthreads) {
            const int32_t i = L->idx[j];
            cut_walk_lane(a, el[i], L->rec[j], dst + i);
        }
        block_barrier();                                             // (the list is the next chunk's from here on)
    }
}

// The cut kernels (row shapes: aasm_dev.h; no register budget), body called as body(k, a).  All rows are KL rows: expanded as
// AASM_CUT_KERNELS(K, KL) or with one macro, AASM_CUT_KERNELS(X), they go to the last macro given.
// One lane per block in the host emulation: the body's barriers and its LDS list need the block's threads one after the other.
#define AASM_CUT_ROWS(KL) \
    KL(KC_PLAN, aasm_cut_plans, 256, 1, AASM_CUT_LDS_BYTES, 0, kb_cut_plan)
#define AASM_CUT_SECOND(K, KL, ...) KL
#define AASM_CUT_KERNELS(...) AASM_CUT_ROWS(AASM_CUT_SECOND(__VA_ARGS__, __VA_ARGS__))
enum CutKern { AASM_CUT_KERNELS(AASM_ROW_ID, AASM_ROW_ID) };
constexpr int cut_block[] = {AASM_CUT_KERNELS(AASM_ROW_BLOCK, AASM_ROW_BLOCK)};
AASM_KERNEL_BODY(run_cut_body, AASM_CUT_KERNELS, CutArgs)
#define AASM_CUT_MAX_BLOCKS 4096         // 256-thread blocks: beyond 16 per CU the chunks are taken grid-stride

// The arguments of a call whose arrays the caller has checked; false: the sizes do not fit the batch.
static inline bool cut_args(const aasm_batch_in &in, const aasm_out_sizes &sz, const aasm_dev_out &o, const aasm_dev_cuts &d, CutArgs &a) {
    if (sz.n_contigs != in.n_contigs || in.n_contigs <= 0 || in.n_records < 0 || sz.n_main < 0 || sz.n_alt < 0 || sz.n_all_paths < 0 || sz.n_all_elems < 0) return false;
    if (sz.n_all_elems > 0 && sz.n_all_paths == 0) return false;
    a.C = in.n_contigs; a.R = in.n_records; a.NP = sz.n_all_paths;
    a.rec_off = in.ctg_rec_off; a.qs = in.qry_str; a.qe = in.qry_end; a.cs_off = in.rec_cs_off; a.fwd = in.aln_fwd; a.cs_text = in.cs_text;
    a.n[0] = sz.n_main; a.n[1] = sz.n_alt; a.n[2] = sz.n_all_elems;
    a.ch0[0] = 0;
    for (int l = 0; l < 3; l++) a.ch0[l + 1] = a.ch0[l] + (a.n[l] + AASM_CUT_CHUNK - 1) / AASM_CUT_CHUNK;
    a.el[0] = (const OutElem *)o.main_elems; a.el[1] = (const OutElem *)o.alt_elems; a.el[2] = (const OutElem *)o.all_elems;
    a.off[0] = o.main_off; a.off[1] = o.alt_off; a.off[2] = o.all_elem_off; a.path_off = o.all_path_off;
    a.dst[0] = d.main; a.dst[1] = d.alt; a.dst[2] = d.all;
    return true;
}
// backends provide launch_cut(kernel, blocks, threads, CutArgs)
template <class B> void cut_launch(B &be, const CutArgs &a) {
    if (a.ch0[3] > 0) be.launch_cut(KC_PLAN, std::min<int64_t>(a.ch0[3], AASM_CUT_MAX_BLOCKS), cut_block[KC_PLAN], a);
}

}  // namespace aasm
