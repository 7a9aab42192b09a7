// aasm_pipeline.h -- launch sequence of the per-contig path-inference pipeline.
//
// Templated on a Backend that provides memory, launches, scans and scalar read-back:
//   * GpuBackend (aasm_gpu.hip): HIP stream, pooled device arena, HIP-event phase timers.
//   * tests/host_emul/emul.cpp: malloc + loops, for CPU-side logic tests only.
// Sizes are data dependent (slots S, vertices VT, edges ET, heap arena HT), so the
// sequence is count -> exclusive scan -> read total -> allocate -> fill, with five small
// device->host scalar reads per batch.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/alignasm_amd.h"
#include "aasm_kernels.h"
#include "aasm_enum.h"

namespace aasm {

enum Kern {
// The pipeline's kernels, in id order (row shapes: aasm_dev.h); bodies are called as body(k, w).  A KL row's registers are budgeted
// for `waves` waves per SIMD: residency per CU is min(4 * waves, 160 KB / LDS bytes) blocks, and these kernels are latency-bound, so it
// is throughput.
// (The table stands inside the enum of its ids, so that the enum's text still lists every id in order for readers of this header.)
#define AASM_PIPELINE_KERNELS(K, KL)                                                                                                  \
    K(KN_CS_RANGES, aasm_k0_cs_ranges, 256, ALL_LANES, kb_cs_ranges)                                                                  \
    KL(KN_SORT, aasm_k1_sort, 256, 1, AASM_SORT_LDS_BYTES, 2, kb_sort)                                                                \
    K(KN_SORT_RANK, aasm_k1_sort_rank, 256, ALL_LANES, kb_sort_rank)                                                                  \
    KL(KN_SORT_FIX, aasm_k1_sort_fix, AASM_WAVE, 1, AASM_SORTFIX_LDS_BYTES, 1, kb_sort_fix)                                           \
    K(KN_GATHER_PARTS, aasm_k1_gather_parts, AASM_WAVE, 1, kb_gather_parts)                                                           \
    K(KN_OV_COUNT, aasm_k2_ov_count, 256, ALL_LANES, kb_ov_count)                                                                     \
    K(KN_OV_MERGE, aasm_k2_ov_merge, 256, ALL_LANES, kb_ov_merge)                                                                     \
    K(KN_VCOUNT, aasm_k2_vcount, 256, ALL_LANES, kb_vcount)                                                                           \
    K(KN_VFILL_REC, aasm_k2_vfill_rec, 256, ALL_LANES, kb_vfill_rec)                                                                  \
    K(KN_VFILL_SLOT, aasm_k2_vfill_slot, 256, ALL_LANES, kb_vfill_slot)                                                               \
    K(KN_NSL, aasm_k4_nsl, 256, ALL_LANES, kb_nsl)                                                                                    \
    K(KN_ROW_COUNT, aasm_k4_row_count, 256, ALL_LANES, kb_row_count)                                                                  \
    K(KN_ROW_FILL, aasm_k4_row_fill, AASM_WAVE, 1, kb_row_fill)                                                                       \
    /* rows + reversed CSR + sweep headers of one contig: 31.8 KB of LDS, 5 workgroups (20 waves) per CU */                           \
    KL(KN_GRAPH, aasm_k46_graph, GB_TPB, 1, AASM_GB_LDS_BYTES, 5, kb_graph_build<GB_MAXV, GB_MAXE>)                                   \
    /* contigs of up to 3 584 vertices / 8 192 edges: 62 KB, two workgroups per CU */                                                 \
    KL(KN_GRAPH_L, aasm_k46_graph_l, GB_TPB, 1, AASM_GB_LDS_BYTES_T(GB_MAXV_L, GB_MAXE_L), 2, kb_graph_build<GB_MAXV_L, GB_MAXE_L>)   \
    K(KN_REV_FILL, aasm_k6_rev_fill, 256, ALL_LANES, kb_rev_fill)                                                                     \
    KL(KN_REV_FILL_W, aasm_k6_rev_fill_w, AASM_WAVE, 1, AASM_REVF_LDS_BYTES, 8, kb_rev_fill_w)                                        \
    /* 25 KB of LDS per block: 6 blocks per CU, i.e. at most 2 waves per SIMD; contigs of <= 3 072 vertices: 6.7 KB */                \
    KL(KN_REV_FILL_ORD, aasm_k6_rev_fill_ord, AASM_WAVE, 1, AASM_REVO_LDS_BYTES, 2, kb_rev_fill_ord)                                  \
    KL(KN_REV_FILL_ORD_S, aasm_k6_rev_fill_ord_s, AASM_WAVE, 1, AASM_REVO_LDS_BYTES_V(REV_ORD_MIDV), 6, kb_rev_fill_ord)              \
    KL(KN_SORT_ROWS_REV, aasm_k6_rev_place, AASM_WAVE, 1, AASM_REVP_LDS_BYTES, 4, kb_rev_place)                                       \
    K(KN_REV_HDR, aasm_k6_rev_hdr, 256, ALL_LANES, kb_rev_hdr)                                                                        \
    KL(KN_REV_SWEEP, aasm_k6_rev_sweep, AASM_WAVE, 1, AASM_REV_LDS_BYTES, 8, kb_rev_sweep<AASM_WAVE>)                                 \
    KL(KN_FWD_SWEEP, aasm_k5_fwd_sweep, AASM_WAVE, 1, AASM_FWD_LDS_BYTES, 8, kb_fwd_sweep<AASM_WAVE>)                                 \
    KL(KN_REV_SWEEP_G, aasm_k6_rev_sweep_g, AASM_WAVE, 1, (AASM_WAVE / AASM_SWEEP_G) * AASM_REV_LDS_BYTES, 4, kb_rev_sweep<AASM_SWEEP_G>) \
    KL(KN_FWD_SWEEP_G, aasm_k5_fwd_sweep_g, AASM_WAVE, 1, (AASM_WAVE / AASM_SWEEP_G) * AASM_FWD_LDS_BYTES, 4, kb_fwd_sweep<AASM_SWEEP_G>) \
    K(KN_CHILDREN, aasm_k7_children, 256, ALL_LANES, kb_children)                                                                     \
    K(KN_HEAP_CAP, aasm_k7_heap_cap, 256, ALL_LANES, kb_heap_cap)                                                                     \
    KL(KN_SIDETRACK_W, aasm_k7_sidetrack_w, AASM_WAVE, 1, AASM_SIDE_LDS_BYTES, 8, kb_sidetrack_w)                                     \
    K(KN_HEAP_HDR, aasm_k7_heap_hdr, 256, ALL_LANES, kb_heap_hdr)                                                                     \
    KL(KN_HEAP, aasm_k7_heap, AASM_WAVE, 1, AASM_HEAP_LDS_BYTES, 5, kb_heap<false, HEAP_RING_1W, HEAP_QN_1W>)                         \
    KL(KN_HEAP_MW, aasm_k7_heap_mw, AASM_WAVE * 4, 1, AASM_MW_LDS_BYTES(4), 4, kb_heap_mw)                                            \
    KL(KN_HEAP_MW8, aasm_k7_heap_mw8, AASM_WAVE * 8, 1, AASM_MW_LDS_BYTES(8), 4, kb_heap_mw)                                          \
    KL(KN_HEAP_MW16, aasm_k7_heap_mw16, AASM_WAVE * 16, 1, AASM_MW_LDS_BYTES(16), 4, kb_heap_mw)                                      \
    K(KN_MW_RANK, aasm_k7_mw_rank, 256, ALL_LANES, kb_mw_rank)                                                                        \
    /* K8's LSM queues; the 1-lane host emulation runs the d-ary heap, with its LDS, in their place */                                \
    KL(KN_ENUM, aasm_k8_enum, AASM_WAVE, 1, AASM_EMUL_OR(AASM_ENUM_LDS_BYTES, AASM_ENUM2_LDS_BYTES), 4,                               \
       AASM_EMUL_OR(kb_enum_heap, kb_enum_lsm<64>))                                                                                   \
    KL(KN_ENUM_S, aasm_k8_enum_s, AASM_WAVE, 1, AASM_EMUL_OR(AASM_ENUM_LDS_BYTES, AASM_ENUM2_LDS_BYTES_F(EQ_FSMALL)), 5,              \
       AASM_EMUL_OR(kb_enum_heap, kb_enum_lsm<EQ_FSMALL>))                                                                            \
    KL(KN_ENUM_HEAP, aasm_k8_enum_heap, AASM_WAVE, 1, AASM_ENUM_LDS_BYTES, 2, kb_enum_heap)                                           \
    KL(KN_SELECT, aasm_k9_select, AASM_WAVE, 1, AASM_SEL_LDS_BYTES, 5, kb_select)                                                     \
    K(KN_GATHER_OUT, aasm_k9_gather_out, AASM_WAVE, 1, kb_gather_out)                                                                 \
    K(KN_TOPO_COUNT, aasm_k9_topo_count, 256, ALL_LANES, kb_topo_count)                                                               \
    K(KN_TOPO_FILL, aasm_k9_topo_fill, AASM_WAVE, 1, kb_topo_fill)                                                                    \
    K(KN_SEL_PLAN, aasm_k9_sel_plan, AASM_WAVE, 1, kb_sel_plan)                                                                       \
    K(KN_SEL_PLANFILL, aasm_k9_sel_planfill, AASM_WAVE, 1, kb_sel_planfill)                                                           \
    KL(KN_SEL_RECOVER, aasm_k9_sel_recover, AASM_WAVE, 1, AASM_SELREC_LDS_BYTES, 8, kb_sel_recover)                                   \
    K(KN_SEL_CLASSIFY, aasm_k9_sel_classify, 256, ALL_LANES, kb_sel_classify)                                                         \
    KL(KN_SEL_CONVERT, aasm_k9_sel_convert, AASM_WAVE, 1, AASM_SEL_LDS_BYTES, 5, kb_sel_convert)                                      \
    K(KN_SEL_FINAL, aasm_k9_sel_final, AASM_WAVE, 1, kb_sel_final)                                                                    \
    /* sweep + pre-pass + BFS order + heaps of one contig, a wave each (96 VGPRs, 19 spilled: worth it for the fifth wave slot per    \
       SIMD); the emulation runs one lane per wave, in wave order: the sweep to its end, then the pre-pass, then the heaps */        \
    KL(KN_CHAIN, aasm_k67_chain, AASM_WAVE * CHAIN_WAVES, CHAIN_WAVES, AASM_CHAIN_LDS_BYTES, 5, kb_chain<true>)                       \
    /* ... without the order wave (the heap wave keeps its own queue): classes of more than AASM_CHAIN_ORD_MAX contigs */             \
    KL(KN_CHAIN3, aasm_k67_chain3, AASM_WAVE * (CHAIN_WAVES - 1), CHAIN_WAVES - 1, AASM_CHAIN_LDS_BYTES, 5, kb_chain<false>)          \
    K(KN_K7_PREP, aasm_k7_prep, 256, ALL_LANES, kb_k7_prep)                                                                           \
    K(KN_TNX, aasm_k9_tnx, 256, ALL_LANES, kb_tnx)                                                                                    \
    K(KN_TNX16, aasm_k9_tnx16, 256, ALL_LANES, kb_tnx16)                                                                              \
    /* the 16-hop jump records of a small contig from its tree in LDS */                                                              \
    KL(KN_TNX16_WG, aasm_k9_tnx16_wg, TNX_TPB, 1, AASM_TNXWG_LDS_BYTES, 4, kb_tnx16_wg)
    AASM_PIPELINE_KERNELS(AASM_ROW_ID, AASM_ROW_ID)
};
constexpr int kern_block[] = {AASM_PIPELINE_KERNELS(AASM_ROW_BLOCK, AASM_ROW_BLOCK)};
AASM_KERNEL_BODY(run_kernel_body, AASM_PIPELINE_KERNELS, WS)

// A launch of `nblocks` blocks of the kernel's own size: backends take (kernel, blocks, threads, args), and every launch but
// AASM_H2_LAUNCH_FAILURE's (run_pipeline) goes through here.
template <class B> void launch(B &be, int kn, int64_t nblocks, const WS &w) { be.launch(kn, nblocks, kern_block[kn], w); }

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
#ifndef AASM_CHAIN_ORD_MAX
#define AASM_CHAIN_ORD_MAX 1024         // contigs of the chain class up to which its workgroups run the order wave (four four-wave workgroups per CU; measured: 1 000 contigs 4.28 against 4.40 ms, 1 150 contigs 5.3 against 4.58)
#endif
#define AASM_CHAIN_SMALL_BATCH 1536      // contigs: up to here every contig of a sparse batch is in the class.  1 280 workgroups are resident at once (256 CUs x 5 three-wave workgroups; the kernels are held to 96 VGPRs - 5 waves / SIMD - so that the forward sweep beside them finds slots: at 4 waves / SIMD a 1 250-contig class took a second round, 5.55 against 4.64 ms); a partial second round still beats the three launches up to ~1 600 contigs (measured: 1 400 contigs 4.85 against 6.3 ms, 1 500: 5.9 / 6.5, 1 600: 6.55 / 6.64, 1 800: 6.7 / 6.8, 2 200: 7.4 / 7.2)

#ifndef AASM_GROUPED_MIN
#define AASM_GROUPED_MIN 2560
#endif
struct PipelineSizes { int64_t C = 0, R = 0, S = 0, VT = 0, ET = 0, HT = 0, bad_record = -1; };

// The test hooks of aasm_opts.reserved (AASM_H0_* / AASM_H2_*, include/alignasm_amd.h), decoded once; all zero in production.
struct Hooks {
    bool seq_select, enum_heap, enum_small, grid_order, graph_launches, chain_half, launch_failure, wrap_devices, dirty_scan, chain_own_queue;
    int32_t heap_mw, chain, chain_test, root_ring, sort_depth;   // WS::mw_mode, chain_mode, chain_test, chain_rn, sort_depth_test
    int32_t mw;                   // K7's several-waves kernel: AASM_H0_MW_INPUT_ORDER, or 4 / 8 / 16 waves per contig
    int64_t range_limit;          // > 0: longer contig ranges "do not fit"
};
static inline Hooks decode_hooks(const aasm_opts &o) {
    const int32_t h0 = o.reserved[0], h2 = o.reserved[2], ch = h0 & AASM_H0_CHAIN_MASK;
    Hooks h;
    h.seq_select = h0 & AASM_H0_SEQ_SELECT; h.enum_heap = h0 & AASM_H0_ENUM_HEAP; h.enum_small = h0 & AASM_H0_ENUM_SMALL;
    h.grid_order = h0 & AASM_H0_GRID_ORDER; h.graph_launches = h0 & AASM_H0_GRAPH_LAUNCHES; h.chain_half = ch == AASM_H0_CHAIN_HALF;
    h.heap_mw = (h0 & AASM_H0_HEAP_MW_ALL) ? 1 : (h0 & AASM_H0_HEAP_MW_NONE) ? 2 : 0;       // every contig / none / by graph density
    h.chain = ch == AASM_H0_CHAIN_ALL ? 1 : ch == AASM_H0_CHAIN_NONE ? 2 : 0;              // every sparse contig / none / by batch shape
    h.mw = (h0 & AASM_H0_MW_MASK) >> AASM_H0_MW_SHIFT; h.range_limit = o.reserved[1];
    h.launch_failure = h2 & AASM_H2_LAUNCH_FAILURE; h.wrap_devices = h2 & AASM_H2_WRAP_DEVICES; h.dirty_scan = h2 & AASM_H2_DIRTY_SCAN;
    h.chain_test = (h2 & AASM_H2_CHAIN_DONE_LOST) ? 2 : (h2 & AASM_H2_CHAIN_HDR_LOST) ? 1 : 0; h.chain_own_queue = h2 & AASM_H2_CHAIN_OWN_QUEUE;
    h.root_ring = (h2 & AASM_H2_SMALL_ROOT_RING) ? 4 : 0; h.sort_depth = (h2 & AASM_H2_SORT_DEPTH_MASK) >> AASM_H2_SORT_DEPTH_SHIFT;
    return h;
}

// The launch forms, from the sizes known once the edges are counted.  MAXV: most vertices of one contig; NCHAIN: contigs of the chain
// class; HTM / NMW: provisional arena and contigs of K7's several-waves class; MAXN: most records of one contig.
struct FormSizes { int64_t C, R, K, VT, ET, MAXV, NCHAIN, HTM, NMW, MAXN; };
struct Forms {
    bool grouped, dense, mw_ranked;   // sweeps two contigs per wave; mean degree > 6; K7's several-waves class by rank, largest node bound first
    int rev_fill, chain, mw_kern, enum_kern;   // the kernels of the reversed CSR's fill, the chain class, K7's class, K8's queue
};
static inline Forms choose_forms(const FormSizes &s, const Hooks &h, bool host_emulation) {
    Forms f;
    f.dense = s.ET > 6 * s.VT;
    // big sparse batches (mean degree <= 6, thousands of contigs: bound by instruction issue): two contigs per wave, AASM_SWEEP_G lanes
    // each; dense ones and small batches (bound by the chain per contig): a wave per contig (the scalar-uniform variant has the shorter
    // chain per pop)
    f.grouped = !f.dense && s.C >= AASM_GROUPED_MIN;
    // dense, no giant contig: the in-lists in order from one pass per contig (every contig of <= REV_ORD_MIDV vertices - C5's have 2 500 -:
    // the launch with 6.7 KB of LDS counters instead of 25 KB, i.e. 6 waves per SIMD instead of 2); else dense: lanes over the edges of 64 rows
    f.rev_fill = f.dense && s.MAXV <= REV_ORD_MAXV ? (s.MAXV <= REV_ORD_MIDV ? KN_REV_FILL_ORD_S : KN_REV_FILL_ORD) : f.dense ? KN_REV_FILL_W : KN_REV_FILL;
    // the class's BFS order from a wave of its own while four waves a contig fit the chip beside the forward sweep (four workgroups per CU);
    // beyond that the three-role kernel, where the heap wave keeps its own queue
    f.chain = !h.chain_own_queue && s.NCHAIN <= AASM_CHAIN_ORD_MAX ? KN_CHAIN : KN_CHAIN3;
    // 16, 8 or 4 waves a contig, by how many of them share the chip's ~8 k wave slots
    const int mw_waves = (h.mw == 4 || h.mw == 8 || h.mw == 16) ? h.mw : s.NMW * 16 <= 6144 ? 16 : s.NMW * 8 <= 6144 ? 8 : 4;
    f.mw_kern = mw_waves == 16 ? KN_HEAP_MW16 : mw_waves == 8 ? KN_HEAP_MW8 : KN_HEAP_MW;
    f.mw_ranked = h.mw != AASM_H0_MW_INPUT_ORDER && s.NMW >= 2 && s.NMW <= 32768;   // (ranked by counting: NMW^2 compares)
    // K8: sorted front + sorted runs (aasm_enum.h) unless a contig is too long for its packed ratio key; the d-ary heap is also what the
    // 1-lane host emulation runs.  More contigs than the 64-entry front keeps resident (14 waves per CU = 3 584): the 40-entry front (20 per
    // CU = 5 120) runs them in one residency round (round 4, with the far tier: 5 000 contigs 23.85 -> 23.1 ms; round 3, without it, the
    // extra refills and flushes of the small front cost more than the second round: 30.2 vs 31.5 ms); beyond 5 120 both take a second round
    const bool enum_heap = host_emulation || h.enum_heap || s.MAXN > AASM_ENUM_MAX_N;
    f.enum_kern = enum_heap ? KN_ENUM_HEAP : ((s.C > 14 * 256 && s.C <= 20 * 256 && s.K > 21) || h.enum_small) ? KN_ENUM_S : KN_ENUM;
    return f;
}

// Runs the pipeline for contigs [0, C) described by `in` (device pointers; ctg_rec_off
// already offset to the chunk).  Leaves all intermediates in the backend's arena and
// returns the filled WS (so fetch / debug can read them).
template <class B>
int run_pipeline(B &be, const aasm_batch_in &in, const aasm_opts &opts, WS &w, PipelineSizes &sz) {
    std::memset(&w, 0, sizeof(w));
    const int64_t C = in.n_contigs;
    int64_t rr[2];
    be.read_i64s({in.ctg_rec_off, in.ctg_rec_off + C}, rr);
    const int64_t R0 = rr[0], R1 = rr[1];
    const int64_t R = R1 - R0;
    w.C = C; w.R = R; w.R0 = R0;
    w.K = opts.max_paths > 0 ? opts.max_paths : 10000;
    w.nsl = opts.non_skip_linkable ? 1 : 0;
    const Hooks h = decode_hooks(opts);
    // the hooks' WS fields, and the inputs of the per-contig classes kb_heap_cap picks on the device
    w.xcd_map = h.grid_order ? 0 : 1; w.sort_depth_test = h.sort_depth;
    // the chain class (kb_chain: sweep, pre-pass and heaps of a contig beside each other), by shape: every contig of a batch too small
    // to fill the chip (its step is its slowest contig's chain), and the long tail of a big one (contigs of >= 4x the mean and >= 2048
    // records: each a chain many times the batch's own step).  AASM_H0_CHAIN_HALF: the contigs of at least the batch's mean size - a
    // class that is part of the batch whatever its shape, so that the class's workgroups and the three launches of the others run
    // beside each other
    w.chain_mode = h.chain; w.chain_test = h.chain_test; w.chain_rn = h.root_ring;
    w.chain_ord = h.chain_own_queue ? 0 : 1;                          // (decided below by the size of the class)
    w.chain_all = (!h.chain_half && C <= AASM_CHAIN_SMALL_BATCH) ? 1 : 0;
    w.chain_minN = (int32_t)std::min<int64_t>(std::max<int64_t>(2048, 4 * (R / std::max<int64_t>(C, 1))), INT32_MAX);
    if (h.chain_half) w.chain_minN = (int32_t)std::min<int64_t>(std::max<int64_t>(1, cdiv(R, std::max<int64_t>(C, 1))), INT32_MAX);
    w.rec_off = in.ctg_rec_off; w.in_qs = in.qry_str; w.in_qe = in.qry_end; w.in_rs = in.ref_str; w.in_re = in.ref_end;
    w.in_qt = in.qry_total; w.in_chr = in.ref_chr; w.in_fwd = in.aln_fwd; w.in_mq = in.map_qul;
    w.in_rng_off = in.rec_rng_off; w.rql = in.rng_qry_l; w.rqr = in.rng_qry_r; w.rrl = in.rng_ref_l; w.rng_stride = 1;
    sz.C = C; sz.R = R;
    if (C <= 0 || R <= 0) return AASM_E_INVAL;

#define A(field, type, n, name) w.field = (type *)be.alloc(name, sizeof(type) * (size_t)((n) > 0 ? (n) : 1))
#define AZ(field, type, n, name) do { A(field, type, n, name); be.zero_alloc(w.field, sizeof(type) * (size_t)((n) > 0 ? (n) : 1)); } while (0)
// out of device memory -> AASM_E_NOMEM (the caller may split the contig range); any other HIP failure (launch,
// memset, scan, read-back) -> AASM_E_HIP with the original error text, never retried
#define CHECK_ALLOC() do { if (be.oom()) return AASM_E_NOMEM; if (be.failed()) return AASM_E_HIP; } while (0)

    AZ(status, int32_t, C, "status");
    AZ(prof_heap, int64_t, C * 8, "prof_heap"); AZ(prof_sel, int64_t, C * 8, "prof_sel"); AZ(prof_gb, int64_t, C * 8, "prof_gb");
    AZ(counters, int64_t, CNT_N, "counters");
    // every zero-initialised per-contig array of the pipeline, one behind the other: one fill for all of them (they used to be zeroed where
    // they were first needed: five more fill dispatches per step)
    AZ(dupflag, int32_t, C, "dupflag");
    AZ(main_len, int32_t, C, "main_len"); AZ(alt_len, int32_t, C, "alt_len"); AZ(all_gen, int32_t, C, "all_gen"); AZ(all_seq, int32_t, C, "all_seq");
    AZ(kfound, int32_t, C, "kfound"); AZ(anom_dest, int32_t, C, "anom_dest"); AZ(h_cnt, int32_t, C, "h_cnt");
    AZ(nconv, int32_t, C, "nconv");

    // ---- K0 (optional): match ranges from the cs tags, on the device
    if (!in.rng_qry_l && in.cs_text && in.rec_cs_off) {
        if (R > INT32_MAX) return AASM_E_INVAL;
        int64_t gg[2];
        be.read_i64s({in.rec_rng_off + R0, in.rec_rng_off + R1}, gg);
        const int64_t G0 = gg[0], G1 = gg[1];
        be.phase_begin(AASM_PH_CS);
        w.cs_text = in.cs_text; w.cs_off = in.rec_cs_off;
        A(rng_rec, int64_t, 4 * (G1 - G0), "rng_rec"); A(cs_bad, int32_t, 2, "cs_bad");
        CHECK_ALLOC();
        w.rng_rec -= 4 * G0;                                         // indexed with the batch's own range offsets
        be.zero(w.cs_bad, 8);
        launch(be, KN_CS_RANGES, cdiv(R, 256), w);
        be.phase_end(AASM_PH_CS);
        const int32_t badv = (int32_t)(uint32_t)(uint64_t)be.read_i64((const int64_t *)w.cs_bad);   // 0 = none, else record - INT32_MAX
        if (badv != 0) { sz.bad_record = R0 + ((int64_t)badv + INT32_MAX); return AASM_E_PARSE; }
        w.rql = w.rng_rec; w.rqr = w.rng_rec + 1; w.rrl = w.rng_rec + 2; w.rng_stride = 4;
    } else if (!in.rng_qry_l) return AASM_E_INVAL;

    // ---- K1 sort + parts
    be.phase_begin(AASM_PH_SORT);
    A(perm, int32_t, R, "perm"); A(np, int32_t, C, "np"); A(pstart, int32_t, R + C, "pstart");
    A(s_qs, int64_t, R, "s_qs"); A(s_qe, int64_t, R, "s_qe"); A(s_rs, int64_t, R, "s_rs"); A(s_re, int64_t, R, "s_re");
    A(s_qt, int64_t, R, "s_qt"); A(s_rb, int64_t, R, "s_rb"); A(s_rn, int32_t, R, "s_rn"); A(s_chr, int32_t, R, "s_chr");
    A(s_orig, int32_t, R, "s_orig"); A(s_ctg, int32_t, R, "s_ctg"); A(s_pid, int32_t, R, "s_pid"); A(s_fl, uint8_t, R, "s_fl");
    CHECK_ALLOC();
    if (h.launch_failure) be.launch(KN_SORT, C, 4096, w);           // the one block size off the table: an invalid launch configuration (> 1024)
    launch(be, KN_SORT, C, w);
    launch(be, KN_SORT_RANK, cdiv(R, 256), w);
    launch(be, KN_SORT_FIX, C, w);
    launch(be, KN_GATHER_PARTS, C, w);
    be.phase_end(AASM_PH_SORT);

    // ---- K2 overlap slots
    be.phase_begin(AASM_PH_PAIRS);
    A(ov_cnt, int32_t, R, "ov_cnt"); A(ov_off, int64_t, R + 1, "ov_off");
    CHECK_ALLOC();
    launch(be, KN_OV_COUNT, cdiv(R, 256), w);
    be.scan_i32(w.ov_cnt, R, w.ov_off);
    const int64_t S = be.read_i64(w.ov_off + R);
    w.S = S; sz.S = S;
    A(ov_rec, int32_t, S, "ov_rec"); A(ov_vid, int32_t, S, "ov_vid"); A(ov_rank, int64_t, S + 1, "ov_rank");
    A(ov_peq, int64_t, S, "ov_peq"); A(ov_per, int64_t, S, "ov_per"); A(ov_stq, int64_t, S, "ov_stq"); A(ov_str, int64_t, S, "ov_str");
    A(ov_ok, uint8_t, S, "ov_ok");
    CHECK_ALLOC();
    if (S > 0) launch(be, KN_OV_MERGE, cdiv(S, 256), w);
    be.scan_u8(w.ov_ok, S, w.ov_rank);
    A(ctgV, int32_t, C, "ctgV"); A(voff, int64_t, C + 1, "voff");
    CHECK_ALLOC();
    launch(be, KN_VCOUNT, cdiv(C, 256), w);
    be.scan_i32(w.ctgV, C, w.voff);
    const int64_t VT = be.read_i64(w.voff + C);
    w.VT = VT; sz.VT = VT;
    A(v_i, int32_t, VT, "v_i"); A(v_j, int32_t, VT, "v_j"); A(v_ctg, int32_t, VT, "v_ctg"); A(v_slot, int64_t, VT, "v_slot");
    CHECK_ALLOC();
    launch(be, KN_VFILL_REC, cdiv(R, 256), w);
    if (S > 0) launch(be, KN_VFILL_SLOT, cdiv(S, 256), w);
    be.phase_end(AASM_PH_PAIRS);

    // main/alt outputs exist even when no contig has a graph (all single-record contigs)
    A(cur_out, OutElem, R, "cur_out"); A(main_out, OutElem, R, "main_out"); A(alt_out, OutElem, R, "alt_out");
    A(main_off, int64_t, C + 1, "main_off"); A(alt_off, int64_t, C + 1, "alt_off");
    w.pool_cap = R + 1024; w.ar_cap = C + R / 4 + 1024;
    A(pool, OutElem, w.pool_cap, "pool");
    A(ar_ctg, int32_t, w.ar_cap, "ar_ctg"); A(ar_gen, int32_t, w.ar_cap, "ar_gen"); A(ar_seq, int32_t, w.ar_cap, "ar_seq");
    A(ar_len, int32_t, w.ar_cap, "ar_len"); A(ar_off, int64_t, w.ar_cap, "ar_off");
    CHECK_ALLOC();

    if (VT > 0) {
        // ---- K3/K4 CSR
        be.phase_begin(AASM_PH_EDGES);
        if (w.nsl) {
            A(dis_end, int32_t, R, "dis_end"); AZ(next_cnt, int32_t, R, "next_cnt");
            CHECK_ALLOC();
            launch(be, KN_NSL, cdiv(R, 256), w);
        }
        A(deg, int32_t, VT, "deg"); A(rowptr, int64_t, VT + 1, "csr_rowptr");
        // (heap arena sizing + classes need only V and E per contig: sized here, so that their read-back shares the edges' one)
        A(hcap_cnt, int32_t, C, "hcap_cnt"); A(hoff, int64_t, C + 1, "hoff");
        A(mw_flag, int32_t, C, "mw_flag"); A(mw_lg, int32_t, C, "mw_lg"); A(mw_cap, int32_t, C, "mw_cap"); A(mw_off, int64_t, C + 1, "mw_off"); A(mw_list, int32_t, C, "mw_list"); A(mw_sorted, int32_t, C, "mw_sorted"); A(mw_key, int32_t, C, "mw_key");
        A(chain_flag, int32_t, C, "chain_flag"); A(chain_list, int32_t, C, "chain_list"); A(gb_flag, int32_t, C, "gb_flag");
        w.gb_off = h.graph_launches ? 1 : 0;
        w.mw_mode = h.heap_mw;
        w.mw_compact = opts.keep_debug ? 1 : 0;   // debug runs compare arena indices with the reference's allocation order
        CHECK_ALLOC();
        launch(be, KN_ROW_COUNT, cdiv(VT, 256), w);
        be.scan_i32(w.deg, VT, w.rowptr);
        launch(be, KN_HEAP_CAP, cdiv(C, 256), w);
        be.scan_i32_pair(w.hcap_cnt, w.hoff, w.mw_cap, w.mw_off, C);
        int64_t et_mv[12];
        be.read_i64s({w.rowptr + VT, w.counters + CNT_MAXV, w.hoff + C, w.mw_off + C, w.counters + CNT_MW, w.counters + CNT_MAXN, w.counters + CNT_CHAIN, w.counters + CNT_GB_S, w.counters + CNT_GB_L, w.counters + CNT_GB_REST}, et_mv);
        const int64_t ET = et_mv[0], MAXV = et_mv[1];                 // (MAXV: most vertices of one contig)
        const int64_t GB_S = et_mv[7], GB_L = et_mv[8], GB_REST = et_mv[9];   // contigs whose graph one workgroup builds (kb_graph_build, two forms) / the others
        const int64_t hh[4] = {et_mv[2], et_mv[3], et_mv[4], et_mv[5]};
        const int64_t NCHAIN = et_mv[6];
        const int64_t HT = hh[0], HTM = hh[1], NMW = HTM > 0 ? hh[2] : 0;
        const Forms f = choose_forms({C, R, w.K, VT, ET, MAXV, NCHAIN, HTM, NMW, hh[3]}, h, B::host_emulation);
        w.chain_ord = f.chain == KN_CHAIN ? 1 : 0;
        w.ET = ET; sz.ET = ET;
        A(e_col, int32_t, ET, "csr_col"); A(e_wq, int64_t, ET, "csr_w_qry"); A(e_wr, int32_t, ET, "csr_w_ref"); A(e_fl, uint8_t, ET, "csr_w_flags");
        A(rptr, int64_t, VT + 1, "rptr"); A(r_pk, I4, ET, "r_pk");
        A(rvh, I4, 3 * VT, "rvh"); A(fvh, I4, 2 * VT, "fvh");
        A(sp_d, Dist, VT, "sp_d"); A(sp_best, int32_t, VT, "sp_best"); A(cnt_tmp, int32_t, VT, "cnt_tmp"); A(cnt_tmp2, int32_t, VT, "cnt_tmp2"); A(an, int32_t, VT, "an");
        if (NCHAIN > 0) { A(pend, int32_t, VT, "pend"); A(cq, int32_t, VT, "cq"); A(bfsq, I4, VT, "bfsq"); }
        // sparse, every contig small: rows, reversed CSR and the sweeps' headers of a contig by ONE workgroup (kb_graph_build)
        // the small contigs of a sparse batch: rows, reversed CSR and the sweeps' headers of a contig by ONE workgroup (kb_graph_build: kb_heap_cap
        // picked them); the others - dense batches, contigs of more than GB_MAXV_L vertices or GB_MAXE_L edges - by the separate launches, which
        // leave the contigs of the class alone
        w.indeg = nullptr;
        if (GB_REST > 0) { AZ(indeg, int32_t, VT, "indeg"); AZ(rcur, int32_t, VT, "rcur"); }   // (two fills in one)
        CHECK_ALLOC();
        if (GB_S > 0) launch(be, KN_GRAPH, C, w);
        if (GB_L > 0) launch(be, KN_GRAPH_L, C, w);
        if (GB_REST == 0) {
            be.phase_end(AASM_PH_EDGES);
            be.phase_begin(AASM_PH_REVCSR);
            be.phase_end(AASM_PH_REVCSR);
        } else {
        launch(be, KN_ROW_FILL, cdiv(VT, AASM_WAVE), w);
        be.phase_end(AASM_PH_EDGES);

        // ---- reversed CSR
        be.phase_begin(AASM_PH_REVCSR);
        A(r_e, int32_t, ET, "r_e"); A(tmp_pk, I4, ET, "tmp_pk");
        CHECK_ALLOC();
        be.scan_i32(w.indeg, VT, w.rptr);
        if (f.rev_fill == KN_REV_FILL_ORD_S || f.rev_fill == KN_REV_FILL_ORD) launch(be, f.rev_fill, C, w);
        else {
            if (f.rev_fill == KN_REV_FILL_W) launch(be, KN_REV_FILL_W, cdiv(VT, AASM_WAVE), w);
            else launch(be, KN_REV_FILL, cdiv(VT, 256), w);
            launch(be, KN_SORT_ROWS_REV, cdiv(VT, AASM_WAVE), w);
        }
        launch(be, KN_REV_HDR, cdiv(VT, 256), w);
        be.phase_end(AASM_PH_REVCSR);
        }

        // ---- K6 / K5 sweeps.  The forward sweep + the topologically ordered CSR copy only feed
        // K9, so they run on a second stream beside rev_sweep -> heaps -> enumeration.
        A(rev_order, int32_t, VT, "rev_order"); A(fwd_order, int32_t, VT, "fwd_order"); A(fwd_pos, int32_t, VT, "fwd_pos");
        A(tp_deg, int32_t, VT, "tp_deg"); A(tp_vj, int32_t, VT, "tp_vj"); A(tp_ptr, int64_t, VT + 1, "tp_ptr");
        A(te_pk, I4, ET, "te_pk");
        CHECK_ALLOC();
        const int64_t sweep_n = AASM_WAVE / AASM_SWEEP_G;
        auto side_work = [&]() {
            be.fork();                                               // side stream waits for everything enqueued so far
            be.use_side(true);
            be.phase_begin(AASM_PH_FWD);
            if (f.grouped) launch(be, KN_FWD_SWEEP_G, cdiv(C, sweep_n), w);
            else launch(be, KN_FWD_SWEEP, C, w);
            be.phase_end(AASM_PH_FWD);
            be.phase_begin(AASM_PH_TOPO);
            launch(be, KN_TOPO_COUNT, cdiv(VT, 256), w);
            be.scan_i32(w.tp_deg, VT, w.tp_ptr);
            launch(be, KN_TOPO_FILL, cdiv(VT, AASM_WAVE), w);
            be.phase_end(AASM_PH_TOPO);
            be.use_side(false);
        };
        // (Measured in round 4, same box: started after the reverse sweep instead, or beside K7 only, the reverse sweep drops to 1.98 ms
        // but K7 beside it rises 4.10 -> 4.6 / 5.0 ms and the step 12.60 -> 12.99 / 12.91: every chain kernel is short of issue slots.)
        side_work();
        // ---- K7's arrays (the chain class fills them while its sweep still runs, so they exist before any sweep starts)
        A(ccnt, int32_t, VT, "ccnt"); A(cval, int32_t, ET, "cval");
        A(st_cost, Dist, ET, "st_cost"); A(st_n, int32_t, VT, "st_n"); A(vhdr, I4, VT, "vhdr"); A(vhdr2, I4, VT, "vhdr2"); A(cinfo, I4, ET, "cinfo"); A(tnx, I4, VT, "tnx"); A(tnx16, int32_t, 16 * VT, "tnx16");
        sz.HT = HT;
        w.avg_sidetracks = (int32_t)std::min<int64_t>((ET - VT + C) / (C > 0 ? C : 1), INT32_MAX);
        A(hnodes, HNode, HT, "hnodes"); A(h_root, int32_t, VT, "h_root"); A(bq, int32_t, VT, "bq");
        A(hprov, HNode, HTM, "hprov");
        A(mw_order, int32_t, VT, "mw_order"); A(mw_rs, int32_t, VT, "mw_rs"); A(mw_fb, int32_t, VT, "mw_fb"); A(mw_rsv, int32_t, VT, "mw_rsv"); A(mw_used, int32_t, VT, "mw_used");
        CHECK_ALLOC();
        be.fill_ff(w.h_root, sizeof(int32_t) * (size_t)VT);
        be.fill_ff(w.bq, sizeof(int32_t) * (size_t)VT);
        if (NCHAIN > 0) {
            // the class's workgroups (three waves a contig) on a stream of their own, beside the forward sweep and - when the class is
            // only the batch's long tail - beside the three launches of everybody else
            be.fill_ff(w.vhdr, sizeof(I4) * (size_t)VT);             // the marker words the heap wave waits on
            be.fill_ff(w.vhdr2, sizeof(I4) * (size_t)VT);
            be.fork2();
            be.use_side2(true);
            be.phase_begin(AASM_PH_CHAIN);
            if (f.chain == KN_CHAIN) launch(be, KN_CHAIN, NCHAIN, w);
            else launch(be, KN_CHAIN3, NCHAIN, w);   // (no order wave: three waves a contig, five workgroups a CU; 1 250 contigs 4.6 ms where four-wave workgroups took 6.0)
            be.phase_end(AASM_PH_CHAIN);
            be.use_side2(false);
        }
        if (NCHAIN < C) {
        be.phase_begin(AASM_PH_SPTREE);
        if (f.grouped) launch(be, KN_REV_SWEEP_G, cdiv(C, sweep_n), w);
        else launch(be, KN_REV_SWEEP, C, w);
        be.phase_end(AASM_PH_SPTREE);

        // ---- K7 heaps
        // the jump records of K9's recovery (the next 4 and the next 16 vertices along best[]) need nothing but the tree: they go to the
        // side stream, which finishes its topological copy about when the reverse sweep ends, and run beside the heap pre-pass
        be.fork_again();
        be.use_side(true);
        if (GB_S + GB_L > 0) launch(be, KN_TNX16_WG, C, w);  // (the small contigs of a sparse batch - kb_graph_build's class: sixteen hops through the tree in LDS)
        if (GB_REST > 0) {
            launch(be, KN_TNX, cdiv(VT, 256), w);
            launch(be, KN_TNX16, cdiv(VT, 256), w);
        }
        be.use_side(false);
        be.phase_begin(AASM_PH_HEAP_PREP);
        if (f.dense) {
            launch(be, KN_CHILDREN, cdiv(VT, 256), w);
            launch(be, KN_SIDETRACK_W, cdiv(VT, AASM_WAVE), w);   // dense: lanes over the edges of 64 rows
            launch(be, KN_HEAP_HDR, cdiv(VT, 256), w);
        } else launch(be, KN_K7_PREP, cdiv(VT, 256), w);         // child list + keys + header of a vertex: one thread, one launch
        be.phase_end(AASM_PH_HEAP_PREP);
        // Nothing may START beside the heap kernel: all its workgroups are resident for the whole launch, so whatever share of the CUs a
        // second queue holds while they are dealt out skews their placement for good (measured: the 0.2 ms jump-record kernel started
        // beside it cost it 1.8 ms, 4.05 -> 5.8; the forward sweep beside it 0.5-0.9 ms in round 4).  The side stream is done by now.
        be.join();
        be.phase_begin(AASM_PH_HEAP);
        launch(be, KN_HEAP, C, w);
        // contigs of the wide-tree class (kb_heap skips them)
        w.mw_n = (int32_t)NMW; w.mw_base = -1;
        if (HTM > 0) {
            // One block per contig of the class, the contig with the largest node bound first: block times of a dense batch go with the
            // node count (C5 share: mean 25 ms, longest 42), and in input order the heavy ones land on the CUs as they come - clumps of them
            // share a CU's issue slots and the launch ends with such a clump.  Largest first deals every CU a spread of weights and
            // starts the longest chains first: C5 share 35.5 -> 30.0 ms, 700 contigs 27.3 -> 25.5, 400 x 1 500 records 25.1 -> 22.8.
            if (f.mw_ranked) {
                launch(be, KN_MW_RANK, cdiv(NMW, 256), w);
                w.mw_base = 0;
                { const int32_t xm = w.xcd_map; w.xcd_map = 0; launch(be, f.mw_kern, NMW, w); w.xcd_map = xm; }   // (its order is its own)
                w.mw_base = -1;
            } else launch(be, f.mw_kern, C, w);
        }
        be.phase_end(AASM_PH_HEAP);
        }                                                            // (NCHAIN < C)
        be.join2();                                                  // the chain class's heaps, before anybody enumerates

        // ---- K8 enumeration
        const int64_t K = w.K;
        A(kd, Dist, C * K, "kd"); A(klast, int32_t, C * K, "klast");
        w.pq_stride = f.enum_kern == KN_ENUM_HEAP ? 3 * K + 1 : enum_stride(K);
        A(kcand, I4, 2 * C * (3 * K + 1), "kcand"); A(pq, PqK, C * w.pq_stride, "pq");
        CHECK_ALLOC();
        be.phase_begin(AASM_PH_ENUM);
        launch(be, f.enum_kern, C, w);
        be.phase_end(AASM_PH_ENUM);
    }

    be.join();                                                       // forward order / topo copy ready
    // ---- K9 selection (also emits the N == 1 contigs)
    // Default: plan -> one wave per converted path -> per-contig final pick.  Falls back to the
    // sequential one-wave-per-contig kernel when the per-conversion scratch would not fit
    // (tie-heavy inputs at large K) or when AASM_H0_SEQ_SELECT asks for it (tests).
    A(mark_time, int32_t, R, "mark_time");
    A(conv_off, int64_t, C + 1, "conv_off"); A(plan_kk, int32_t, C * 2 * SEL_PLAN_KEEP, "plan_kk");
    CHECK_ALLOC();
    be.fill_byte(w.mark_time, 0x7F, sizeof(int32_t) * (size_t)R);
    bool sequential = h.seq_select;
    int64_t NCONV = 0, SR = 0, SV = 0;
    bool nm_ready = false;                                           // the output totals have been read with the pick's pool demand
    int64_t nm[2] = {0, 0};
    if (!sequential) {
        be.phase_begin(AASM_PH_MISC);
        if (VT > 0) launch(be, KN_SEL_PLAN, C, w);
        be.scan_i32(w.nconv, C, w.conv_off);
        NCONV = be.read_i64(w.conv_off + C);
        w.NCONV = NCONV;
        if (NCONV > 0) {
            A(cv_ctg, int32_t, NCONV, "cv_ctg"); A(cv_k, int32_t, NCONV, "cv_k"); A(cv_ord, int32_t, NCONV, "cv_ord"); A(cv_kind, int32_t, NCONV, "cv_kind");
            A(cv_szr, int32_t, NCONV, "cv_szr"); A(cv_szv, int32_t, NCONV, "cv_szv"); A(cv_roff, int64_t, NCONV + 1, "cv_roff"); A(cv_voff, int64_t, NCONV + 1, "cv_voff");
            AZ(cv_n, int32_t, NCONV, "cv_n"); AZ(cv_err, int32_t, NCONV, "cv_err"); AZ(cv_cov, int64_t, NCONV, "cv_cov"); A(cv_la, int32_t, NCONV, "cv_la");
            CHECK_ALLOC();
            launch(be, KN_SEL_PLANFILL, C, w);
            be.scan_i32_pair(w.cv_szr, w.cv_roff, w.cv_szv, w.cv_voff, NCONV);
            int64_t sv[2];
            be.read_i64s({w.cv_roff + NCONV, w.cv_voff + NCONV}, sv);
            SR = sv[0]; SV = sv[1];
            const int64_t bytes = SR * (24 + (int64_t)sizeof(OutElem)) + SV * ((int64_t)sizeof(Dist) + 8);
            if (bytes > ((int64_t)24 << 30)) sequential = true;
        }
        be.phase_end(AASM_PH_MISC);
    }
    if (!sequential) {
        if (NCONV > 0) {
            A(cv_path, int32_t, 6 * SR, "cv_path"); A(cv_out, OutElem, SR, "cv_out");
            A(cv_dist2, Dist, SV, "cv_dist2"); A(cv_pre2, int32_t, SV, "cv_pre2"); AZ(cv_stamp, int32_t, SV, "cv_stamp");
            CHECK_ALLOC();
            be.phase_begin(AASM_PH_SELECT);
            launch(be, KN_SEL_RECOVER, NCONV, w);
            launch(be, KN_SEL_CLASSIFY, NCONV, w);
            launch(be, KN_SEL_CONVERT, NCONV, w);
            be.phase_end(AASM_PH_SELECT);
        }
        be.phase_begin(AASM_PH_FINAL);
        launch(be, KN_SEL_FINAL, C, w);
        // the output lengths are final with the pick: their offsets are scanned at once, and ONE read-back brings the pool demand and the
        // two totals (it was a wait for the demand, then the scans, then a wait for the totals)
        be.scan_i32_pair(w.main_len, w.main_off, w.alt_len, w.alt_off, C);
        int64_t np2[4];
        be.read_i64s({w.counters + CNT_POOL, w.counters + CNT_AR, w.main_off + C, w.alt_off + C}, np2);
        const int64_t need_pool = np2[0], need_ar = np2[1];
        nm_ready = true; nm[0] = np2[2]; nm[1] = np2[3];
        if (need_pool > w.pool_cap || need_ar > w.ar_cap) {         // .all pool overflow: exact-size re-run of the pick only
            w.pool_cap = need_pool + 16; w.ar_cap = need_ar + 16;
            A(pool, OutElem, w.pool_cap, "pool");
            A(ar_ctg, int32_t, w.ar_cap, "ar_ctg"); A(ar_gen, int32_t, w.ar_cap, "ar_gen"); A(ar_seq, int32_t, w.ar_cap, "ar_seq");
            A(ar_len, int32_t, w.ar_cap, "ar_len"); A(ar_off, int64_t, w.ar_cap, "ar_off");
            CHECK_ALLOC();
            be.zero(w.all_seq, sizeof(int32_t) * (size_t)C);
            be.zero(w.counters + CNT_POOL, sizeof(int64_t)); be.zero(w.counters + CNT_AR, sizeof(int64_t)); be.zero(w.counters + CNT_OVF, sizeof(int64_t));
            launch(be, KN_SEL_FINAL, C, w);
            nm_ready = false;                                        // (the same lengths again, but keep the one code path: scanned and read below)
        }
        be.phase_end(AASM_PH_FINAL);
    } else {
        A(pathA, int32_t, 2 * (R + 2 * C), "pathA"); A(pathB, int32_t, 2 * (R + 2 * C), "pathB"); A(pathT, int32_t, 2 * (R + 2 * C), "pathT");
        A(pre2, int32_t, VT, "pre2"); AZ(stamp, int32_t, VT, "stamp"); A(dist2, Dist, VT, "dist2");
        CHECK_ALLOC();
        be.phase_begin(AASM_PH_SELECT);
        launch(be, KN_SELECT, C, w);
        be.phase_end(AASM_PH_SELECT);
        int64_t np2[2];
        be.read_i64s({w.counters + CNT_POOL, w.counters + CNT_AR}, np2);
        const int64_t need_pool = np2[0], need_ar = np2[1];
        if (need_pool > w.pool_cap || need_ar > w.ar_cap) {         // .all pool overflow (tie-heavy inputs): one exact-size re-run
            w.pool_cap = need_pool + 16; w.ar_cap = need_ar + 16;
            A(pool, OutElem, w.pool_cap, "pool");
            A(ar_ctg, int32_t, w.ar_cap, "ar_ctg"); A(ar_gen, int32_t, w.ar_cap, "ar_gen"); A(ar_seq, int32_t, w.ar_cap, "ar_seq");
            A(ar_len, int32_t, w.ar_cap, "ar_len"); A(ar_off, int64_t, w.ar_cap, "ar_off");
            CHECK_ALLOC();
            be.zero(w.stamp, sizeof(int32_t) * (size_t)(VT > 0 ? VT : 1));
            be.fill_byte(w.mark_time, 0x7F, sizeof(int32_t) * (size_t)R);
            be.zero(w.all_gen, sizeof(int32_t) * (size_t)C); be.zero(w.all_seq, sizeof(int32_t) * (size_t)C);
            be.zero(w.counters + CNT_POOL, sizeof(int64_t)); be.zero(w.counters + CNT_AR, sizeof(int64_t));
            be.zero(w.counters + CNT_CONVERTED, sizeof(int64_t)); be.zero(w.counters + CNT_OVF, sizeof(int64_t));
            be.zero(w.counters + CNT_ISPR_E, sizeof(int64_t)); be.zero(w.counters + CNT_ISPR_V, sizeof(int64_t));
            be.zero(w.counters + CNT_PATH_E, sizeof(int64_t)); be.zero(w.counters + CNT_OUT_E, sizeof(int64_t));
            be.phase_begin(AASM_PH_MISC);
            launch(be, KN_SELECT, C, w);
            be.phase_end(AASM_PH_MISC);
        }
    }

    // ---- output compaction
    be.phase_begin(AASM_PH_GATHER);
    if (!nm_ready) {
        be.scan_i32_pair(w.main_len, w.main_off, w.alt_len, w.alt_off, C);
        be.read_i64s({w.main_off + C, w.alt_off + C}, nm);
    }
    const int64_t NM = nm[0], NA = nm[1];
    A(main_c, OutElem, NM, "main_c"); A(alt_c, OutElem, NA, "alt_c");
    CHECK_ALLOC();
    launch(be, KN_GATHER_OUT, C, w);
    be.phase_end(AASM_PH_GATHER);
#undef A
#undef AZ
#undef CHECK_ALLOC
    return AASM_OK;
}

// Pack device results into the ragged host structure (shared by both backends).
template <class B>
int fetch_results(B &be, const WS &w, const PipelineSizes &sz, aasm_batch_out *out) {
    std::memset(out, 0, sizeof(*out));
    const int64_t C = w.C;
    out->n_contigs = C;
    out->main_off = (int64_t *)calloc(C + 1, 8);
    out->alt_off = (int64_t *)calloc(C + 1, 8);
    out->all_path_off = (int64_t *)calloc(C + 1, 8);
    out->ctg_status = (int32_t *)calloc(C + 1, 4);
    be.d2h(out->main_off, w.main_off, (C + 1) * 8);
    be.d2h(out->alt_off, w.alt_off, (C + 1) * 8);
    be.d2h(out->ctg_status, w.status, C * 4);
    const int64_t NM = out->main_off[C], NA = out->alt_off[C];
    out->main_elems = (aasm_out_elem *)malloc((NM + 1) * sizeof(aasm_out_elem));      // (every element is overwritten: no zero fill of 100s of MB)
    out->alt_elems = (aasm_out_elem *)malloc((NA + 1) * sizeof(aasm_out_elem));
    static_assert(sizeof(aasm_out_elem) == sizeof(OutElem), "layout");
    if (NM) be.d2h_big(out->main_elems, w.main_c, NM * sizeof(OutElem));
    if (NA) be.d2h_big(out->alt_elems, w.alt_c, NA * sizeof(OutElem));
    int64_t cnt[CNT_N];
    be.d2h(cnt, w.counters, sizeof(cnt));
    // .all paths: keep records of the final generation, ordered by (contig, seq)
    int64_t nar = cnt[CNT_AR] < w.ar_cap ? cnt[CNT_AR] : w.ar_cap;
    int64_t npool = cnt[CNT_POOL] < w.pool_cap ? cnt[CNT_POOL] : w.pool_cap;
    std::vector<int32_t> ar_ctg(nar), ar_gen(nar), ar_seq(nar), ar_len(nar), gen(C);
    std::vector<int64_t> ar_off(nar);
    std::vector<OutElem> pool(npool);
    if (nar) {
        be.d2h(ar_ctg.data(), w.ar_ctg, nar * 4); be.d2h(ar_gen.data(), w.ar_gen, nar * 4); be.d2h(ar_seq.data(), w.ar_seq, nar * 4);
        be.d2h(ar_len.data(), w.ar_len, nar * 4); be.d2h(ar_off.data(), w.ar_off, nar * 8);
        be.d2h(pool.data(), w.pool, npool * sizeof(OutElem));
    }
    be.d2h(gen.data(), w.all_gen, C * 4);
    std::vector<std::vector<std::pair<int32_t, int64_t>>> per(C);   // (seq, record)
    for (int64_t r = 0; r < nar; r++) {
        const int32_t c = ar_ctg[r];
        if (c < 0 || c >= C || ar_gen[r] != gen[c]) continue;
        if (ar_off[r] + ar_len[r] > npool) continue;
        per[c].push_back({ar_seq[r], r});
    }
    int64_t np = 0, ne = 0;
    for (int64_t c = 0; c < C; c++) {
        std::sort(per[c].begin(), per[c].end());
        np += (int64_t)per[c].size();
        for (auto &x : per[c]) ne += ar_len[x.second];
        out->all_path_off[c + 1] = np;
    }
    out->n_all_paths = np;
    out->all_elem_off = (int64_t *)calloc(np + 1, 8);
    out->all_elems = (aasm_out_elem *)calloc(ne + 1, sizeof(aasm_out_elem));
    int64_t ip = 0, ie = 0;
    for (int64_t c = 0; c < C; c++)
        for (auto &x : per[c]) {
            std::memcpy(out->all_elems + ie, pool.data() + ar_off[x.second], sizeof(OutElem) * (size_t)ar_len[x.second]);
            ie += ar_len[x.second];
            out->all_elem_off[++ip] = ie;
        }
    // statistics
    aasm_stats &st = out->stats;
    st.n_vertices = sz.VT; st.n_edges = sz.ET;
    st.n_heap_nodes = cnt[CNT_HEAPNODES]; st.n_paths_found = cnt[CNT_PATHS]; st.n_paths_converted = cnt[CNT_CONVERTED];
    st.n_unconnectable = cnt[CNT_UNCONN]; st.range_steps = cnt[CNT_RANGE_STEPS];
    st.ispr_edges = cnt[CNT_ISPR_E]; st.ispr_vertices = cnt[CNT_ISPR_V]; st.path_edges = cnt[CNT_PATH_E]; st.out_elems = cnt[CNT_OUT_E];
    st.pq_pushes = cnt[CNT_PQ_PUSH];
    std::vector<int32_t> ctgV(C);
    be.d2h(ctgV.data(), w.ctgV, C * 4);
    std::vector<int64_t> roff(C + 1);
    be.d2h(roff.data(), w.rec_off, (C + 1) * 8);
    for (int64_t c = 0; c < C; c++) {
        const int64_t N = roff[c + 1] - roff[c];
        if (N == 1) st.n_single++;
        if (ctgV[c] > 0) st.n_pairs += ctgV[c] - 2 - N;
        if (out->ctg_status[c] != 0) st.n_internal_errors++;
    }
    return AASM_OK;
}


// ---- device-side export (aasm_result_sizes / aasm_result_export): fetch_results' arrays built on the device ----------------
// Backends provide alloc / zero / fill_ff / scan_i32 / read_i64s as for the pipeline, and launch_pack(kernel, blocks, threads, PackArgs).
// The scratch is carved out of the result's workspace when the result is made (pack_alloc, behind run_pipeline);
// sizes = count -> scan -> place -> scan -> ONE read-back, run once per result: exports in flight read that scratch, so a later
// sizes call answers from the cached sizes and never rebuilds it; export = two launches, no read-back.
// The pack kernels (row shapes: aasm_dev.h), body called as body(k, a).
#define AASM_PACK_KERNELS(K, ...)                               \
    K(KP_COUNT, aasm_pack_count, 256, ALL_LANES, kb_pack_count) \
    K(KP_PLACE, aasm_pack_place, 256, ALL_LANES, kb_pack_place) \
    K(KP_FLAT, aasm_pack_flat, 256, ALL_LANES, kb_pack_flat)    \
    K(KP_ALL, aasm_pack_all, 256, ALL_LANES, kb_pack_all)
enum PackKern { AASM_PACK_KERNELS(AASM_ROW_ID, AASM_ROW_ID) };
constexpr int pack_block[] = {AASM_PACK_KERNELS(AASM_ROW_BLOCK, AASM_ROW_BLOCK)};
AASM_KERNEL_BODY(run_pack_body, AASM_PACK_KERNELS, PackArgs)
template <class B> void launch(B &be, int kp, int64_t nblocks, const PackArgs &a) { be.launch_pack(kp, nblocks, pack_block[kp], a); }
#define AASM_PACK_MAX_BLOCKS 2048   // 256-thread blocks of the copies: 8 waves per CU of the 256 (grid-stride beyond)

struct PackWS {
    bool ready = false;               // scratch carved
    bool sized = false;               // sizes[] holds the last aasm_result_sizes answer
    int32_t *np = nullptr, *st = nullptr, *prec = nullptr, *plen = nullptr;
    int64_t *poff = nullptr, *eoff = nullptr;
    int64_t sizes[5] = {0, 0, 0, 0, 0};   // n_contigs, n_main, n_alt, n_all_paths, n_all_elems
};

static inline PackArgs pack_args(const WS &w, const PackWS &p) {
    PackArgs a;
    std::memset(&a, 0, sizeof(a));
    a.C = w.C; a.ar_cap = w.ar_cap; a.pool_cap = w.pool_cap; a.counters = w.counters;
    a.ar_ctg = w.ar_ctg; a.ar_gen = w.ar_gen; a.ar_seq = w.ar_seq; a.ar_len = w.ar_len; a.all_gen = w.all_gen; a.all_seq = w.all_seq;
    a.status = w.status; a.ar_off = w.ar_off; a.main_off = w.main_off; a.alt_off = w.alt_off;
    a.pool = w.pool; a.main_c = w.main_c; a.alt_c = w.alt_c;
    a.np = p.np; a.st = p.st; a.prec = p.prec; a.plen = p.plen; a.poff = p.poff; a.eoff = p.eoff;
    return a;
}

template <class B>
int pack_alloc(B &be, const WS &w, PackWS &p) {
    const int64_t C = w.C, AR = w.ar_cap;
    if (C <= 0 || AR > INT32_MAX) return AASM_OK;                   // (no export for such a result: pack_sizes reports it)
    if (!p.ready) {
        p.np = (int32_t *)be.alloc("pack_np", sizeof(int32_t) * (size_t)C);
        p.st = (int32_t *)be.alloc("pack_st", sizeof(int32_t) * (size_t)C);
        p.poff = (int64_t *)be.alloc("pack_poff", sizeof(int64_t) * (size_t)(C + 1));
        p.prec = (int32_t *)be.alloc("pack_prec", sizeof(int32_t) * (size_t)AR);
        p.plen = (int32_t *)be.alloc("pack_plen", sizeof(int32_t) * (size_t)AR);
        p.eoff = (int64_t *)be.alloc("pack_eoff", sizeof(int64_t) * (size_t)(AR + 1));
        if (be.failed()) return be.oom() ? AASM_E_NOMEM : AASM_E_HIP;
        p.ready = true;
    }
    return AASM_OK;
}

template <class B>
int pack_sizes(B &be, const WS &w, PackWS &p) {
    const int64_t C = w.C, AR = w.ar_cap;
    if (C <= 0) return AASM_E_INVAL;
    if (AR > INT32_MAX) return AASM_E_OVERFLOW;                     // (record ids are int32 in prec)
    if (p.sized) return AASM_OK;                                     // (a result's sizes do not change; its scratch may be in use)
    if (!p.ready) return AASM_E_INTERNAL;
    const PackArgs a = pack_args(w, p);
    be.zero(p.np, sizeof(int32_t) * (size_t)C);
    be.fill_ff(p.prec, sizeof(int32_t) * (size_t)AR);
    be.zero(p.plen, sizeof(int32_t) * (size_t)AR);
    launch(be, KP_COUNT, cdiv(std::max(C, AR), 256), a);
    be.scan_i32(p.np, C, p.poff);
    launch(be, KP_PLACE, cdiv(AR, 256), a);
    be.scan_i32(p.plen, AR, p.eoff);                                 // (slots past the last path are 0: eoff[NP .. AR] = NE)
    int64_t v[4];
    be.read_i64s({p.poff + C, p.eoff + AR, w.main_off + C, w.alt_off + C}, v);
    if (be.failed()) return AASM_E_HIP;
    p.sizes[0] = C; p.sizes[1] = v[2]; p.sizes[2] = v[3]; p.sizes[3] = v[0]; p.sizes[4] = v[1];
    p.sized = true;
    return AASM_OK;
}

// dst arrays as aasm_dev_out; the caller has checked them and the sizes against p.sizes
template <class B>
void pack_export(B &be, const WS &w, const PackWS &p, const aasm_dev_out &d) {
    PackArgs a = pack_args(w, p);
    a.NM = p.sizes[1]; a.NA = p.sizes[2]; a.NP = p.sizes[3]; a.NE = p.sizes[4];
    a.d_main_off = d.main_off; a.d_alt_off = d.alt_off; a.d_path_off = d.all_path_off; a.d_elem_off = d.all_elem_off;
    a.d_main = (OutElem *)d.main_elems; a.d_alt = (OutElem *)d.alt_elems; a.d_all = (OutElem *)d.all_elems; a.d_status = d.ctg_status;
    const int64_t words = std::max(std::max(w.C + 1, a.NP + 1), 5 * std::max(a.NM, a.NA));
    launch(be, KP_FLAT, std::min<int64_t>(cdiv(words, 256), AASM_PACK_MAX_BLOCKS), a);
    if (a.NP > 0) launch(be, KP_ALL, std::min<int64_t>(cdiv(a.NP, 256 / AASM_WAVE), AASM_PACK_MAX_BLOCKS), a);
}

}  // namespace aasm
