// aasm_gpu.hip -- gfx950 backend of the pipeline + the C-ABI entry points that touch the GPU.
//
// * one named __global__ per row of the kernel tables (row shapes: aasm_dev.h; tables: aasm_pipeline.h, aasm_sssp.h, aasm_ksw.h,
//   aasm_cut.h, aasm_read.h, aasm_rows.h), from ONE generator, so rocprofv3 --kernel-trace shows `aasm_k6_rev_sweep` etc., and ONE launch (launch_row);
// * the generic graph entries (dijkstra, Dial, k shortest walks): bodies, argument checks and host drivers in aasm_sssp.h and
//   aasm_ksw.h, run here through one backend (GraphGpu); their resident form (aasm_graphs.h: a checked batch on the device, device
//   pointers in and out on the caller's stream) through GraphsGpu;
// * exclusive scans (count -> offsets): ONE launch each, single pass with decoupled look-back (aasm_scan_chain);
// * a per-device arena: device memory is carved by bump allocation out of a few large
//   hipMalloc blocks that persist across solves (no hipMalloc in the steady state);
// * everything is enqueued on ONE HIP stream per device context; HIP events bracket each
//   phase on that stream when opts.collect_timing is set.
// There is NO CPU fallback here: without a usable HIP device every solve entry point
// returns AASM_E_NODEVICE.
#include <hip/hip_runtime.h>
#include <initializer_list>

#include <atomic>
#include <chrono>
#include <functional>
#include <mutex>
#include <thread>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "aasm_pipeline.h"
#include "aasm_ksw.h"
#include "aasm_graphs.h"
#include "aasm_cut.h"
#include "aasm_read.h"
#include "aasm_alt.h"
#include "aasm_rows.h"
#include "aasm_paf.hpp"

namespace aasm {

// ------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------
// XCD-aware block -> work mapping (w.xcd_map): workgroups are dealt round-robin over the 8 XCDs, each with an L2 of its own, so
// block b takes work item (b % 8) * (G / 8) + b / 8 - every XCD walks ONE contiguous eighth of the work, and neighbouring items
// (vertices of one contig, conversions of one contig) meet in one L2 instead of eight
__device__ inline int64_t xcd_bid(int64_t b, int64_t g, int on) {
    if (!on || g < 64) return b;
    const int64_t g8 = g & ~(int64_t)7;
    return b < g8 ? (b & 7) * (g8 >> 3) + (b >> 3) : b;
}
// One __global__ per row of a kernel table: sym(the family's parameters) runs the row's body as its thread's KCtx k, for block `bid`
// of the launch's work, with the block's LDS (KL rows) or nullptr.  What the kernels of a table share is its family, named by
// AASM_FAMILY while the table is expanded: the parameter list, the block's work item, the argument of the bodies, and how the body is
// called - AASM_DIRECT, or AASM_BY_ID through run_kernel_body for the pipeline, 14 of whose kernels compile to other code when called directly.
#define AASM_KCTX(bid, lds) KCtx k{(int)threadIdx.x, (int)blockDim.x, bid, (int64_t)gridDim.x, (int)(threadIdx.x & 63), lds}
#define AASM_SMEM(bytes) __shared__ __attribute__((aligned(16))) char smem[bytes]
#define AASM_XCD_BID xcd_bid((int64_t)blockIdx.x, (int64_t)gridDim.x, w.xcd_map)
#define AASM_DIRECT(arg, id, ...) __VA_ARGS__(k, arg)
#define AASM_BY_ID(arg, id, ...) run_kernel_body(id, k, arg)
#define AASM_GLOBAL(params, bid, arg, call, bounds, sym, smem_decl, lds, id, ...) \
    __global__ void bounds sym params { smem_decl AASM_KCTX(bid, lds); call(arg, id, __VA_ARGS__); }
#define AASM_GLOBAL_OF(...) AASM_GLOBAL(__VA_ARGS__)
#define K(id, sym, block, lanes, ...) AASM_GLOBAL_OF(AASM_FAMILY, __launch_bounds__(block), sym, , nullptr, id, __VA_ARGS__)
#define KL(id, sym, block, lanes, lds, waves, ...) AASM_GLOBAL_OF(AASM_FAMILY, __launch_bounds__(block, waves), sym, AASM_SMEM(lds);, smem, id, __VA_ARGS__)
// the pipeline (bodies: aasm_kernels.h, aasm_enum.h)
#define AASM_FAMILY (WS w), AASM_XCD_BID, w, AASM_BY_ID
AASM_PIPELINE_KERNELS(K, KL)
#undef AASM_FAMILY
// the device-side export of a result (aasm_result_sizes / aasm_result_export)
#define AASM_FAMILY (PackArgs a), (int64_t)blockIdx.x, a, AASM_DIRECT
AASM_PACK_KERNELS(K, KL)
#undef AASM_FAMILY
// the generic graph entries: bodies in aasm_sssp.h (★J dijkstra, ★L bellman_ford, ★M topology_sort / shortest_path_dag, K5 Dial) ...
#define AASM_FAMILY (SsspArgs a), (int64_t)blockIdx.x, a, AASM_DIRECT
AASM_SSSP_KERNELS(K, KL)
#undef AASM_FAMILY
// ... the kernels around them on a resident graph batch (aasm_graphs.h) ...
#define AASM_FAMILY (GraphsArgs a), (int64_t)blockIdx.x, a, AASM_DIRECT
AASM_GRAPHS_KERNELS(K, KL)
#undef AASM_FAMILY
// ... and aasm_ksw.h (★K: a launch covers the graphs [g0, g0 + grid))
#define AASM_FAMILY (int64_t g0, KswArgs a), g0 + (int64_t)blockIdx.x, a, AASM_DIRECT
AASM_KSW_KERNELS(K, KL)
#undef AASM_FAMILY
// the cut plans of an exported result (aasm_cut_plans_device; body in aasm_cut.h)
#define AASM_FAMILY (CutArgs a), (int64_t)blockIdx.x, a, AASM_DIRECT
AASM_CUT_KERNELS(K, KL)
#undef AASM_FAMILY
// the device reader (aasm_paf_parse_device; bodies in aasm_read.h)
#define AASM_FAMILY (ReadArgs a), (int64_t)blockIdx.x, a, AASM_DIRECT
AASM_READ_KERNELS(K, KL)
#undef AASM_FAMILY
// the --alt merge on a resident batch (aasm_paf_merge_alt_device; bodies in aasm_alt.h)
#define AASM_FAMILY (AltArgs a), (int64_t)blockIdx.x, a, AASM_DIRECT
AASM_ALT_KERNELS(K, KL)
#undef AASM_FAMILY
// output rows on the device (aasm_rows_sizes_device / aasm_rows_format_device; bodies in aasm_rows.h)
#define AASM_FAMILY (RowsArgs a), (int64_t)blockIdx.x, a, AASM_DIRECT
AASM_ROWS_KERNELS(K, KL)
#undef AASM_FAMILY
#undef K
#undef KL

// The rows of a table as {__global__, its name, its block size}, by id, and the launch of one: `nblocks` blocks of `nthreads`
// threads (0: the row's own block size) on stream s; the caller reads hipGetLastError.  An id outside the table launches nothing.
template <class... P> struct KernelSym { void (*fn)(P...); const char *name; int block; };
#define K(id, sym, block, ...) {sym, #sym, block},
static const KernelSym<WS> pipeline_syms[] = {AASM_PIPELINE_KERNELS(K, K)};
static const KernelSym<PackArgs> pack_syms[] = {AASM_PACK_KERNELS(K, K)};
static const KernelSym<SsspArgs> sssp_syms[] = {AASM_SSSP_KERNELS(K, K)};
static const KernelSym<GraphsArgs> graphs_syms[] = {AASM_GRAPHS_KERNELS(K, K)};
static const KernelSym<int64_t, KswArgs> ksw_syms[] = {AASM_KSW_KERNELS(K, K)};
static const KernelSym<CutArgs> cut_syms[] = {AASM_CUT_KERNELS(K, K)};
static const KernelSym<ReadArgs> read_syms[] = {AASM_READ_KERNELS(K, K)};
static const KernelSym<AltArgs> alt_syms[] = {AASM_ALT_KERNELS(K, K)};
static const KernelSym<RowsArgs> rows_syms[] = {AASM_ROWS_KERNELS(K, K)};
#undef K
template <size_t N, class... P> static void launch_row(const KernelSym<P...> (&rows)[N], int id, int64_t nblocks, int nthreads, hipStream_t s, const P &...args) {
    if ((size_t)id >= N) return;
    hipLaunchKernelGGL(rows[id].fn, dim3((unsigned)nblocks), dim3((unsigned)(nthreads ? nthreads : rows[id].block)), 0, s, args...);
}

// ---- T1 truth tables on the device (test entry aasm_debug_predicates) ------------------
// One thread per pair (a, b) of 5-int64 PafDistance tuples {qry, ref, anom, qul_nonzero, qul_total}.
// out bit 0: dist_lt<CALC_SUM>(a, b)   bit 1: dist_lt<QRY_SCORE>(a, b)   bit 2: dist_eq(a, b)
//     bit 3: nodeq_key_lt (heap node holding key a, against key b; K7's descent test)
//     bit 4: pq_full_less (a, b as priority-queue candidates with equal node / insertion index; K8)
//     bit 5: qe_less on K8's default-queue entries built from a, b (sum = qry + ref, qe_key2, equal node / index)
__global__ void __launch_bounds__(256) aasm_t1_predicates(const int64_t *a, const int64_t *b, int64_t n, uint8_t *out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Dist x, y;
    x.qry = a[5 * i]; x.ref = a[5 * i + 1]; x.anom = (int32_t)a[5 * i + 2]; x.qnz = (int32_t)a[5 * i + 3]; x.qtot = (int32_t)a[5 * i + 4]; x.pad = 0;
    y.qry = b[5 * i]; y.ref = b[5 * i + 1]; y.anom = (int32_t)b[5 * i + 2]; y.qnz = (int32_t)b[5 * i + 3]; y.qtot = (int32_t)b[5 * i + 4]; y.pad = 0;
    NodeQ nd;
    nd.q0.x = (int32_t)(uint32_t)(uint64_t)x.qry; nd.q0.y = (int32_t)((uint64_t)x.qry >> 32);
    nd.q0.z = (int32_t)(uint32_t)(uint64_t)x.ref; nd.q0.w = (int32_t)((uint64_t)x.ref >> 32);
    nd.q1.x = x.anom; nd.q1.y = x.qnz; nd.q1.z = x.qtot; nd.q1.w = 1;
    nd.q2.x = nd.q2.y = -1; nd.q2.z = nd.q2.w = 0;
    uint8_t r = 0;
    r |= dist_lt<CALC_SUM_MODE>(x, y) ? 1 : 0;
    r |= dist_lt<QRY_SCORE_MODE>(x, y) ? 2 : 0;
    r |= dist_eq(x, y) ? 4 : 0;
    r |= nodeq_key_lt(nd, y, y.qry + y.ref) ? 8 : 0;
    r |= pq_full_less(x, 7, 3, y, 7, 3) ? 16 : 0;
    QE ea, eb;
    ea.sum = (uint64_t)(x.qry + x.ref); ea.key2 = qe_key2(x.anom, x.qnz, x.qtot); ea.nc = ((uint64_t)7 << 32) | 3; ea.tag = 0;
    eb.sum = (uint64_t)(y.qry + y.ref); eb.key2 = qe_key2(y.anom, y.qnz, y.qtot); eb.nc = ea.nc; eb.tag = 0;
    r |= qe_less(ea, eb) ? 32 : 0;
    out[i] = r;
}

// ---- exclusive scan: T in -> int64 out[n+1] -----------------------------------------
// ONE launch per scan (the pipeline runs ~14 per batch, most over 7-15 M entries): tiles take their number from a
// ticket (so every tile's predecessors are running or done), publish their sum, and find their prefix by looking back
// over the published words, 64 tiles per look (single-pass scan with decoupled look-back).  A word is
// {state : 2, value : 62}; the sums here are counts (>= 0, far below 2^62).  The tile that finishes last clears the
// words and the counters, so the scratch buffer is ready for the next scan on the same stream.
#define SCAN_TPB 256
#define SCAN_IPT 16
#define SCAN_TILE (SCAN_TPB * SCAN_IPT)
#define SCAN_AGG 1ull
#define SCAN_PREFIX 2ull
#define SCAN_HDR 2                           // words ahead of the tile words: ticket, #tiles done
#define SCAN_STALL_S 10                      // look-back gives up after this many seconds without a published predecessor
#define SCAN_STALL_SLOT 63                   // word of DevCtx::pinned (host-pinned, device-visible) the stalled lane raises
__device__ __forceinline__ int64_t scan_wave_incl(int64_t x, int lane) {
    for (int d = 1; d < 64; d <<= 1) { const int64_t y = __shfl_up(x, d, 64); if (lane >= d) x += y; }
    return x;
}
template <class T>
__global__ void __launch_bounds__(SCAN_TPB) aasm_scan_chain(const T *in, int64_t n, int64_t *out, unsigned long long *scr, int64_t nt, int64_t *stall_flag) {
    __shared__ int64_t sh_wave[SCAN_TPB / 64];
    __shared__ int64_t sh_prefix;
    __shared__ unsigned long long sh_tile;
    __shared__ int sh_last;
    unsigned long long *words = scr + SCAN_HDR;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) sh_tile = atomicAdd(&scr[0], 1ull);
    __syncthreads();
    const int64_t tile = (int64_t)sh_tile;
    const int64_t base = tile * SCAN_TILE + (int64_t)threadIdx.x * SCAN_IPT;
    int64_t v[SCAN_IPT], s = 0;
#pragma unroll
    for (int i = 0; i < SCAN_IPT; i++) { v[i] = (base + i < n) ? (int64_t)in[base + i] : 0; s += v[i]; }
    const int64_t incl = scan_wave_incl(s, lane);
    if (lane == 63) sh_wave[wv] = incl;
    __syncthreads();
    int64_t wave_off = 0, total = 0;
#pragma unroll
    for (int i = 0; i < SCAN_TPB / 64; i++) { const int64_t t = sh_wave[i]; if (i < wv) wave_off += t; total += t; }
    // (a ticket beyond the last tile - the counter was left dirty by an aborted launch - has no elements and no slot among the
    // words the last tile clears: it publishes nothing and waits for nobody)
    if (wv == 0 && tile < nt) {                                      // the first wave publishes and looks back
        int64_t prefix = 0;
        if (tile > 0) {
            if (lane == 0) __hip_atomic_store(&words[tile], (SCAN_AGG << 62) | (unsigned long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int64_t j = tile - 1;                                    // lane i looks at tile j - i
            for (;;) {
                const int64_t mine = j - lane;
                unsigned long long x = SCAN_PREFIX << 62;            // (tiles before the first one: an empty prefix)
                if (mine >= 0) {
                    // a predecessor publishes within microseconds (it took its ticket before this tile did); the guard is for a
                    // scratch buffer left dirty by an aborted launch: after SCAN_STALL_S seconds the lane gives up, raises the
                    // host-visible flag (the host turns it into AASM_E_HIP at its next wait) and the launch drains
                    int64_t polls = 0, t0 = 0;
                    do {
                        x = __hip_atomic_load(&words[mine], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if ((x >> 62) == 0 && (++polls & 4095) == 0) {
                            const int64_t now = wave_realtime();
                            if (t0 == 0) t0 = now;
                            else if (now - t0 > (int64_t)SCAN_STALL_S * 100000000) {
                                __hip_atomic_store(stall_flag, (int64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                                x = SCAN_PREFIX << 62;
                            }
                        }
                    } while ((x >> 62) == 0);
                }
                const uint64_t pm = __ballot((x >> 62) == SCAN_PREFIX);
                const int stop = pm ? __ffsll((long long)pm) - 1 : 64;   // nearest tile that knows its prefix
                int64_t val = (lane <= stop) ? (int64_t)(x & ((1ull << 62) - 1)) : 0;
                for (int d = 32; d >= 1; d >>= 1) val += __shfl_xor(val, d, 64);
                prefix += val;
                if (pm) break;
                j -= 64;
            }
        }
        if (lane == 0) {
            __hip_atomic_store(&words[tile], (SCAN_PREFIX << 62) | (unsigned long long)(prefix + total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            sh_prefix = prefix;
            if (tile == nt - 1) out[n] = prefix + total;
        }
    }
    __syncthreads();
    int64_t run = sh_prefix + wave_off + incl - s;                   // exclusive prefix of this thread
#pragma unroll
    for (int i = 0; i < SCAN_IPT; i++) { if (base + i < n) out[base + i] = run; run += v[i]; }
    // ---- the last tile to get here resets the scratch words (every look-back is over by then)
    if (threadIdx.x == 0) sh_last = (atomicAdd(&scr[1], 1ull) == (unsigned long long)(nt - 1)) ? 1 : 0;
    __syncthreads();
    if (sh_last) {
        for (int64_t i = threadIdx.x; i < nt; i += SCAN_TPB) __hip_atomic_store(&words[i], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (threadIdx.x == 0) { __hip_atomic_store(&scr[0], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); __hip_atomic_store(&scr[1], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    }
}

// ---- fills: the memsets a solve needs between two launches (fresh arrays, counters, 0xFF / 0x7F patterns) as ONE launch ----
#define FILL_MAX 8
#define FILL_BLOCK_BYTES 65536
struct FillSegs { void *p[FILL_MAX]; uint64_t n[FILL_MAX]; uint32_t v[FILL_MAX]; uint32_t blk0[FILL_MAX + 1]; int cnt; };
__global__ void __launch_bounds__(256) aasm_multi_fill(FillSegs s) {
    const uint32_t b = blockIdx.x;
    int i = 0;
    while (i + 1 < s.cnt && b >= s.blk0[i + 1]) i++;
    const uint64_t off = (uint64_t)(b - s.blk0[i]) * FILL_BLOCK_BYTES;
    const uint64_t end = s.n[i] < off + FILL_BLOCK_BYTES ? s.n[i] : off + FILL_BLOCK_BYTES;
    char *p = (char *)s.p[i];
    const uint32_t v = s.v[i];
    if ((((uintptr_t)p) & 15) == 0) {
        uint4 q; q.x = q.y = q.z = q.w = v;
        uint64_t o = off + (uint64_t)threadIdx.x * 16;
        for (; o + 16 <= end; o += 256 * 16) *(uint4 *)(p + o) = q;
        const uint64_t tail = end & ~(uint64_t)15;                  // (off is a multiple of 16: the last partial quad of the segment)
        if (tail >= off && tail + threadIdx.x < end) p[tail + threadIdx.x] = (char)v;
    } else {
        for (uint64_t o = off + threadIdx.x; o < end; o += 256) p[o] = (char)v;
    }
}

// ---- short scans: ONE workgroup, no tickets, no look-back --------------------------------------------------------------
// Seven of a step's thirteen scans run over per-contig or per-conversion counts (5 000 - 11 000 elements on C3): two tiles of the
// single-pass scan above, which then spends 30 us on its ticket, its look-back across two workgroups and the reset of its words.
// One workgroup of 1 024 threads walks such an array 4 096 elements at a time instead; up to two arrays of the same length per
// launch (heap capacities + several-waves capacities, the conversions' two scratch sizes, main + alt output lengths).
#define SCAN_SMALL_MAX 131072
__global__ void __launch_bounds__(1024) aasm_scan_small(const int32_t *in_a, int64_t *out_a, const int32_t *in_b, int64_t *out_b, int64_t n) {
    __shared__ int64_t sh_w[2][16];
    __shared__ int64_t sh_carry[2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x < 2) sh_carry[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t base = 0; base < n; base += 4096) {
        const int64_t i0 = base + (int64_t)threadIdx.x * 4;
        int64_t va[4], vb[4], sa = 0, sb = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) { va[i] = (i0 + i < n) ? (int64_t)in_a[i0 + i] : 0; sa += va[i]; vb[i] = (in_b && i0 + i < n) ? (int64_t)in_b[i0 + i] : 0; sb += vb[i]; }
        const int64_t ia = scan_wave_incl(sa, lane), ib = scan_wave_incl(sb, lane);
        if (lane == 63) { sh_w[0][wv] = ia; sh_w[1][wv] = ib; }
        __syncthreads();
        int64_t oa = sh_carry[0], ob = sh_carry[1], ta = 0, tb = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) { const int64_t xa = sh_w[0][i], xb = sh_w[1][i]; if (i < wv) { oa += xa; ob += xb; } ta += xa; tb += xb; }
        int64_t ra = oa + ia - sa, rb = ob + ib - sb;
#pragma unroll
        for (int i = 0; i < 4; i++) { if (i0 + i < n) { out_a[i0 + i] = ra; if (in_b) out_b[i0 + i] = rb; } ra += va[i]; rb += vb[i]; }
        __syncthreads();
        if (threadIdx.x == 0) { sh_carry[0] += ta; sh_carry[1] += tb; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out_a[n] = sh_carry[0]; if (in_b) out_b[n] = sh_carry[1]; }
}

// ---- scalar read-back: up to twelve device words -> the host-mapped pinned words, ONE launch (it was a copyBuffer per word) ----
struct ScalarSrc { const int64_t *p[12]; };
__global__ void aasm_read_scalars(ScalarSrc src, int n, int64_t *dst) {
    const int i = (int)threadIdx.x;
    if (i < n) __hip_atomic_store(dst + i, *src.p[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ------------------------------------------------------------------------------------
// device context + backend
// ------------------------------------------------------------------------------------
struct ArenaBlock { char *p; size_t cap, used; };

struct DevCtx {
    int device = -1;
    bool ready = false;
    hipStream_t stream = nullptr, side = nullptr, side2 = nullptr;
    hipEvent_t ev_fork, ev_join, ev_fork2, ev_join2, ev_fork_b;
    int64_t *d_scratch2 = nullptr;      // scan tile sums of the side stream
    size_t d_scratch2_cap = 0;
    std::vector<ArenaBlock> blocks;
    int64_t *pinned = nullptr;          // host-pinned scalar read-back buffer (word SCAN_STALL_SLOT: raised by a scan whose look-back stalled)
    int64_t *pinned_dev = nullptr;      // the same buffer as the device addresses it
    char *stage[2] = {nullptr, nullptr};   // host-pinned staging chunks of the result fetch (created on first use)
    int64_t *d_scratch = nullptr;       // scan tile sums
    size_t d_scratch_cap = 0;
    uint64_t generation = 0;
    std::atomic<int> input_arrived{0};  // an upload for this context has begun: a warm-up that has not allocated yet stands back
    std::mutex mu;
    hipEvent_t ev_b[AASM_N_PHASES], ev_e[AASM_N_PHASES], ev_t0, ev_t1;
    int n_events_made = 0;              // ev_fork, ev_join, then timing_event(0 ..); ev_fork2 / ev_join2 are counted by n_events2
    int n_events2 = 0;
    hipEvent_t *timing_event(int i) { return i < AASM_N_PHASES ? &ev_b[i] : i < 2 * AASM_N_PHASES ? &ev_e[i - AASM_N_PHASES] : i == 2 * AASM_N_PHASES ? &ev_t0 : &ev_t1; }
    bool events = false;
    size_t peak_bytes = 0;
    std::vector<hipEvent_t> export_events;   // recorded behind each export in flight: the next reuse of the arena waits for them
};

// wait for the exports in flight (they read the arena); under cx.mu
static void drain_exports(DevCtx &cx) {
    for (hipEvent_t e : cx.export_events) { (void)hipEventSynchronize(e); (void)hipEventDestroy(e); }
    cx.export_events.clear();
}
static DevCtx g_ctx[16];
static std::mutex g_init_mu;
static std::atomic<int64_t> g_n_range_splits{0}, g_n_device_mallocs{0}, g_n_stream_syncs{0}, g_n_read_slow_rows{0}, g_n_read_fallbacks{0}, g_n_read_containers{0}, g_n_alt_verdicts{0}, g_n_alt_merges{0};

// aasm_debug_poison: 0 = off (production), 1..255 = the byte the three allocators below fill fresh working memory with, so that
// a kernel reading a cell nobody wrote meets it instead of a harmless left-over.  Left alone: the scans' ticket / tile words
// (d_scratch, d_scratch2: zero between solves by contract), the pinned buffers, g_rows_words, aasm_upload memory (written whole by H2D).
static std::atomic<int> g_poison{0};
static inline int poison_byte() { return g_poison.load(std::memory_order_relaxed); }

static std::string hip_err(const char *what, hipError_t e) {
    return std::string(what) + ": " + hipGetErrorString(e);
}

static int ctx_init(int device) {
    if (device < 0 || device >= 16) { set_last_error("device ordinal out of range"); return AASM_E_INVAL; }
    std::lock_guard<std::mutex> lk(g_init_mu);
    DevCtx &cx = g_ctx[device];
    if (cx.ready) return AASM_OK;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { set_last_error("no HIP device available (this library has no CPU fallback)"); return AASM_E_NODEVICE; }
    if (device >= n) { set_last_error("device ordinal beyond hipGetDeviceCount"); return AASM_E_NODEVICE; }
    if ((e = hipSetDevice(device)) != hipSuccess) { set_last_error(hip_err("hipSetDevice", e)); return AASM_E_NODEVICE; }
    // everything or nothing: a failure leaves no half-made context behind (the next call starts over)
    auto fail = [&](const char *what, hipError_t err) {
        set_last_error(hip_err(what, err));
        if (cx.pinned) { hipHostFree(cx.pinned); cx.pinned = nullptr; }
        if (cx.n_events_made > 0) { hipEventDestroy(cx.ev_fork); }
        if (cx.n_events_made > 1) { hipEventDestroy(cx.ev_join); }
        for (int i = 2; i < cx.n_events_made; i++) hipEventDestroy(*cx.timing_event(i - 2));
        cx.n_events_made = 0;
        if (cx.n_events2 > 0) { hipEventDestroy(cx.ev_fork2); }
        if (cx.n_events2 > 1) { hipEventDestroy(cx.ev_join2); }
        if (cx.n_events2 > 2) { hipEventDestroy(cx.ev_fork_b); }
        cx.n_events2 = 0;
        if (cx.side2) { hipStreamDestroy(cx.side2); cx.side2 = nullptr; }
        if (cx.side) { hipStreamDestroy(cx.side); cx.side = nullptr; }
        if (cx.stream) { hipStreamDestroy(cx.stream); cx.stream = nullptr; }
        return AASM_E_NODEVICE;
    };
    if ((e = hipStreamCreateWithFlags(&cx.stream, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", e);
    if ((e = hipStreamCreateWithFlags(&cx.side, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", e);
    if ((e = hipStreamCreateWithFlags(&cx.side2, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreate", e);
    if ((e = hipEventCreateWithFlags(&cx.ev_fork2, hipEventDisableTiming)) != hipSuccess) return fail("hipEventCreate", e);
    cx.n_events2 = 1;
    if ((e = hipEventCreateWithFlags(&cx.ev_join2, hipEventDisableTiming)) != hipSuccess) return fail("hipEventCreate", e);
    cx.n_events2 = 2;
    if ((e = hipEventCreateWithFlags(&cx.ev_fork_b, hipEventDisableTiming)) != hipSuccess) return fail("hipEventCreate", e);
    cx.n_events2 = 3;
    if ((e = hipEventCreateWithFlags(&cx.ev_fork, hipEventDisableTiming)) != hipSuccess) return fail("hipEventCreate", e);
    cx.n_events_made = 1;
    if ((e = hipEventCreateWithFlags(&cx.ev_join, hipEventDisableTiming)) != hipSuccess) return fail("hipEventCreate", e);
    cx.n_events_made = 2;
    for (int i = 0; i < 2 * AASM_N_PHASES + 2; i++) {
        if ((e = hipEventCreate(cx.timing_event(i))) != hipSuccess) return fail("hipEventCreate", e);
        cx.n_events_made++;
    }
    if ((e = hipHostMalloc((void **)&cx.pinned, 64 * sizeof(int64_t), hipHostMallocMapped)) != hipSuccess) return fail("hipHostMalloc", e);
    std::memset(cx.pinned, 0, 64 * sizeof(int64_t));
    if ((e = hipHostGetDevicePointer((void **)&cx.pinned_dev, cx.pinned, 0)) != hipSuccess) return fail("hipHostGetDevicePointer", e);
    cx.events = true;
    cx.device = device;
    cx.ready = true;
    return AASM_OK;
}

struct GpuBackend {
    static constexpr bool host_emulation = false;
    DevCtx &cx;
    hipStream_t stream, main_stream;
    bool on_side = false, forked = false, forked2 = false;
    bool timing;
    bool fail = false, out_of_memory = false;
    bool phase_used[AASM_N_PHASES] = {false};
    size_t cur_block = 0, bytes = 0;
    std::map<std::string, std::pair<void *, size_t>> named;
    GpuBackend(DevCtx &c, hipStream_t s, bool t) : cx(c), stream(s), main_stream(s), timing(t) {
        drain_exports(cx);
        for (auto &b : cx.blocks) b.used = 0;
        cx.generation++;
    }
    // a backend on the CURRENT result's workspace (the export): allocates behind the solve's arrays, keeps the generation
    struct Attach {};
    GpuBackend(DevCtx &c, hipStream_t s, Attach) : cx(c), stream(s), main_stream(s), timing(false) {}
    void hip_fail(const char *what, hipError_t e) { if (!fail) set_last_error(hip_err(what, e)); fail = true; }
    void *alloc(const char *name, size_t n) {
        n = (n + 255) & ~(size_t)255;
        while (cur_block < cx.blocks.size() && cx.blocks[cur_block].used + n > cx.blocks[cur_block].cap) cur_block++;
        if (cur_block >= cx.blocks.size()) {
            // a new block doubles the arena (first block: 1 GB), so a cold start takes a handful of hipMalloc
            // calls whatever the batch needs; when the doubled size does not fit, only what is asked for
            size_t have = 0;
            for (auto &b : cx.blocks) have += b.cap;
            size_t cap = have > ((size_t)1 << 30) ? have : ((size_t)1 << 30);
            if (cap < n) cap = n;
            char *p = nullptr;
            hipError_t e = hipMalloc((void **)&p, cap);
            g_n_device_mallocs++;
            if (e == hipErrorOutOfMemory && cap > n) { (void)hipGetLastError(); cap = n; e = hipMalloc((void **)&p, cap); g_n_device_mallocs++; }
            if (e != hipSuccess) {
                if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); out_of_memory = true; if (!fail) set_last_error("out of device memory (workspace arena)"); fail = true; }
                else hip_fail("hipMalloc", e);
                return nullptr;
            }
            cx.blocks.push_back(ArenaBlock{p, cap, 0});
            cur_block = cx.blocks.size() - 1;
            if (const int pz = poison_byte()) {                      // (waits: the block's first user may be on another of the solve's streams)
                e = hipMemsetAsync(p, pz, cap, stream);
                if (e == hipSuccess) e = hipStreamSynchronize(stream);
                if (e != hipSuccess) { hip_fail("hipMemsetAsync(poison)", e); return nullptr; }
            }
        }
        ArenaBlock &b = cx.blocks[cur_block];
        void *p = b.p + b.used;
        b.used += n;
        bytes += n;
        if (bytes > cx.peak_bytes) cx.peak_bytes = bytes;
        named[name] = {p, n};
        return p;
    }
    // aasm_debug_poison: every block's whole capacity, before the solve's first allocation (used is 0 everywhere, the exports
    // have drained): the attached backends, which allocate behind the solve's arrays, start from the byte too
    void poison_arena(int pz) {
        for (auto &b : cx.blocks) {
            if (fail) return;
            hipError_t e = hipMemsetAsync(b.p, pz, b.cap, stream);
            if (e != hipSuccess) hip_fail("hipMemsetAsync(poison)", e);
        }
    }
    bool failed() const { return fail; }
    bool test_dirty_scan = false;
    // a scan's look-back gave up (aasm_scan_chain): every later size is garbage - fail the solve before anything is sized by it
    bool scan_stalled() {
        if (!cx.pinned[SCAN_STALL_SLOT]) return false;
        if (!fail) set_last_error("scan look-back stalled (scratch words left dirty by an aborted launch?)");
        fail = true;
        return true;
    }
    bool oom() const { return out_of_memory; }
    // Fills are DEFERRED: a request joins a pending list (a zero fill of an array that sits right behind the last one in the arena
    // only extends it), and whatever touches the stream next issues the list first - as ONE launch (aasm_multi_fill), or a plain
    // memset when it is a single span.  A step of the pipeline had 19 fillBufferAligned dispatches.
    FillSegs fs_;
    bool fs_fresh_[FILL_MAX] = {false};                              // span i is made of WHOLE fresh allocations only (may be extended over the allocator's padding)
    int n_fs = 0;
    void flush_zero() {
        if (n_fs == 0) return;
        const int n = n_fs;
        n_fs = 0;
        if (fail) return;
        if (n == 1) {
            hipError_t e = hipMemsetAsync(fs_.p[0], (int)(fs_.v[0] & 0xff), (size_t)fs_.n[0], stream);
            if (e != hipSuccess) hip_fail("hipMemsetAsync", e);
            return;
        }
        uint32_t blocks = 0;
        for (int i = 0; i < n; i++) { fs_.blk0[i] = blocks; blocks += (uint32_t)((fs_.n[i] + FILL_BLOCK_BYTES - 1) / FILL_BLOCK_BYTES); }
        fs_.blk0[n] = blocks; fs_.cnt = n;
        hipLaunchKernelGGL(aasm_multi_fill, dim3(blocks), dim3(256), 0, stream, fs_);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) hip_fail("fill launch", e);
    }
    void add_fill(void *p, int v, size_t n, bool fresh) {
        if (!p || n == 0 || fail) return;
        char *c = (char *)p;
        const uint32_t vv = (uint32_t)(v & 0xff) * 0x01010101u;
        bool overlap = false;                                        // spans of one launch are written concurrently: an overlapping request waits for the list
        for (int i = 0; i < n_fs; i++) overlap |= c < (char *)fs_.p[i] + fs_.n[i] && (char *)fs_.p[i] < c + n;
        // A WHOLE fresh allocation right behind the last span - itself made of whole fresh allocations, so that the gap between the
        // two is nothing but the allocator's alignment padding, nobody's data - becomes one longer span.  (A partial fill as the last
        // span - zero(counters + CNT_POOL, 8) - must never be stretched over its neighbours' live bytes.)
        if (fresh && !overlap && n_fs > 0 && fs_fresh_[n_fs - 1] && fs_.v[n_fs - 1] == vv) {
            char *hi = (char *)fs_.p[n_fs - 1] + fs_.n[n_fs - 1];
            if (c >= hi && (size_t)(c - hi) <= 256) { fs_.n[n_fs - 1] = (uint64_t)(c + n - (char *)fs_.p[n_fs - 1]); return; }
        }
        if (overlap || n_fs == FILL_MAX || n >= ((size_t)4000 << 20) * 64) flush_zero();   // (a span's block count must fit 32 bits)
        fs_.p[n_fs] = p; fs_.n[n_fs] = n; fs_.v[n_fs] = vv; fs_fresh_[n_fs] = fresh; n_fs++;
    }
    void zero_alloc(void *p, size_t n) { add_fill(p, 0, n, true); }  // a WHOLE fresh allocation
    void zero(void *p, size_t n) { add_fill(p, 0, n, false); }
    void fill_byte(void *p, int v, size_t n) { add_fill(p, v, n, false); }
    void fill_ff(void *p, size_t n) { add_fill(p, 0xFF, n, false); }
    template <class A, size_t N> void launch_on(const KernelSym<A> (&rows)[N], int id, int64_t nblocks, int nthreads, const A &a) {
        flush_zero();
        if (fail || nblocks <= 0) return;
        launch_row(rows, id, nblocks, nthreads, stream, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) hip_fail("kernel launch", e);
    }
    void launch(int kn, int64_t nblocks, int nthreads, const WS &w) { launch_on(pipeline_syms, kn, nblocks, nthreads, w); }
    void launch_pack(int kp, int64_t nblocks, int nthreads, const PackArgs &a) { launch_on(pack_syms, kp, nblocks, nthreads, a); }
    template <class T> void scan_t(const T *in, int64_t n, int64_t *out) {
        flush_zero();
        if (fail) return;
        if (n <= 0) { zero(out, 8); return; }
        const int64_t nt = cdiv(n, SCAN_TILE);
        int64_t *&scr = on_side ? cx.d_scratch2 : cx.d_scratch;
        size_t &scr_cap = on_side ? cx.d_scratch2_cap : cx.d_scratch_cap;
        if ((size_t)nt + 8 > scr_cap) {
            hipDeviceSynchronize();                                  // rare growth: nothing may still use the old buffer
            if (scr) hipFree(scr);
            scr_cap = (size_t)nt * 2 + 1024;
            hipError_t e = hipMalloc((void **)&scr, scr_cap * 8);
            if (e == hipSuccess) e = hipMemsetAsync(scr, 0, scr_cap * 8, stream);   // (the scan kernel leaves the words zero again)
            if (e != hipSuccess) { scr = nullptr; scr_cap = 0; hip_fail("hipMalloc(scan)", e); return; }
        }
        if (test_dirty_scan && nt > 1) { (void)hipMemsetAsync(scr, 1, 1, stream); test_dirty_scan = false; }   // ticket counter = 1: tile 0 never runs
        hipLaunchKernelGGL(HIP_KERNEL_NAME(aasm_scan_chain<T>), dim3((unsigned)nt), dim3(SCAN_TPB), 0, stream, in, n, out, (unsigned long long *)scr, nt, cx.pinned_dev + SCAN_STALL_SLOT);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) hip_fail("scan launch", e);
    }
    void scan_small(const int32_t *a, int64_t *oa, const int32_t *b, int64_t *ob, int64_t n) {
        flush_zero();
        if (fail) return;
        hipLaunchKernelGGL(aasm_scan_small, dim3(1), dim3(1024), 0, stream, a, oa, b, ob, n);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) hip_fail("scan launch", e);
    }
    void scan_i32(const int32_t *in, int64_t n, int64_t *out) {
        if (n > 0 && n <= SCAN_SMALL_MAX && !test_dirty_scan) scan_small(in, out, nullptr, nullptr, n);
        else scan_t<int32_t>(in, n, out);
    }
    // two arrays of the same length: one launch when they are short
    void scan_i32_pair(const int32_t *a, int64_t *oa, const int32_t *b, int64_t *ob, int64_t n) {
        if (n > 0 && n <= SCAN_SMALL_MAX && !test_dirty_scan) scan_small(a, oa, b, ob, n);
        else { scan_t<int32_t>(a, n, oa); scan_t<int32_t>(b, n, ob); }
    }
    void scan_u8(const uint8_t *in, int64_t n, int64_t *out) { scan_t<uint8_t>(in, n, out); }
    int64_t read_i64(const int64_t *p) { int64_t v = 0; read_i64s({p}, &v); return v; }
    // several scalars, ONE launch and ONE wait: the kernel queues up behind the kernels that produce them and stores into the
    // host-mapped pinned words (kernel completion at the stream sync makes system-scope stores visible to the host)
    void read_i64s(std::initializer_list<const int64_t *> ps, int64_t *out) {
        int n = 0;
        for (auto p : ps) { (void)p; out[n++] = 0; }
        flush_zero();
        if (fail) return;
        ScalarSrc src;
        int i = 0;
        for (auto p : ps) { if (i < 12) src.p[i] = p; i++; }
        for (int j = i; j < 12; j++) src.p[j] = nullptr;
        hipLaunchKernelGGL(aasm_read_scalars, dim3(1), dim3(64), 0, stream, src, n, cx.pinned_dev);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        g_n_stream_syncs++;
        if (e != hipSuccess) { hip_fail("scalar read-back", e); return; }
        if (scan_stalled()) return;
        for (i = 0; i < n; i++) out[i] = cx.pinned[i];
    }
    void d2h(void *dst, const void *src, size_t n) {
        flush_zero();
        if (fail || n == 0) return;
        hipError_t e = hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) hip_fail("hipMemcpy D2H", e);
        scan_stalled();
    }
    void h2d(void *dst, const void *src, size_t n) {
        flush_zero();
        if (fail || n == 0) return;
        hipError_t e = hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) hip_fail("hipMemcpy H2D", e);
    }
    // second stream: fork = side waits for the main stream's work so far; join = main waits for side
    void fork() { flush_zero(); if (fail) return; hipEventRecord(cx.ev_fork, main_stream); hipStreamWaitEvent(cx.side, cx.ev_fork, 0); forked = true; }
    // a second hand-over main -> side later in the pipeline, through an event of its own: re-recording ev_fork while the side stream's first
    // wait on it has not executed yet moved THAT wait to the later record (measured: the forward sweep then ran beside K7 instead of
    // beside the reverse sweep, and K7 took 5.8 ms instead of 4.1)
    void fork_again() { flush_zero(); if (fail) return; hipEventRecord(cx.ev_fork_b, main_stream); hipStreamWaitEvent(cx.side, cx.ev_fork_b, 0); forked = true; }
    void use_side(bool on) { flush_zero(); on_side = on; stream = on ? cx.side : main_stream; }
    void join() { flush_zero(); if (fail || !forked) return; hipEventRecord(cx.ev_join, cx.side); hipStreamWaitEvent(main_stream, cx.ev_join, 0); forked = false; }
    // third stream (the chain class's workgroups): same protocol; it runs no scans, so it needs no scratch of its own
    void fork2() { flush_zero(); if (fail) return; hipEventRecord(cx.ev_fork2, main_stream); hipStreamWaitEvent(cx.side2, cx.ev_fork2, 0); forked2 = true; }
    void use_side2(bool on) { flush_zero(); stream = on ? cx.side2 : main_stream; }
    void join2() { flush_zero(); if (fail || !forked2) return; hipEventRecord(cx.ev_join2, cx.side2); hipStreamWaitEvent(main_stream, cx.ev_join2, 0); forked2 = false; }
    void phase_begin(int ph) { flush_zero(); if (timing && !fail) { hipError_t e = hipEventRecord(cx.ev_b[ph], stream); if (e != hipSuccess) hip_fail("hipEventRecord", e); phase_used[ph] = true; } }
    void phase_end(int ph) { flush_zero(); if (timing && !fail) { hipError_t e = hipEventRecord(cx.ev_e[ph], stream); if (e != hipSuccess) hip_fail("hipEventRecord", e); } }
};

// The backend of the generic graph entries (dijkstra_run, dial_run, ksw_run; contract in aasm_ksw.h) and of the debug entries:
// plain hipMalloc blocks freed with it, copies and launches on the device's stream.  entry names the C-ABI entry in messages.
struct GraphGpu {
    hipStream_t stream;
    const char *entry;
    hipError_t e = hipSuccess;
    std::vector<void *> blocks;
    ~GraphGpu() { for (void *p : blocks) hipFree(p); }
    void *alloc(size_t n) {
        void *p = nullptr;
        if (e != hipSuccess) return nullptr;
        if ((e = hipMalloc(&p, n)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        blocks.push_back(p);
        if (const int pz = poison_byte()) { if ((e = hipMemsetAsync(p, pz, n, stream)) != hipSuccess) return nullptr; }
        return p;
    }
    size_t mark() const { return blocks.size(); }
    void release(size_t m) { while (blocks.size() > m) { hipFree(blocks.back()); blocks.pop_back(); } }
    bool h2d(void *d, const void *h, size_t n) { return e == hipSuccess && (e = hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, stream)) == hipSuccess; }
    bool fill(void *d, int byte, size_t n) { return e == hipSuccess && (e = hipMemsetAsync(d, byte, n, stream)) == hipSuccess; }
    bool d2h(void *h, const void *d, size_t n) {
        if (e == hipSuccess) e = hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, stream);
        return sync();
    }
    bool sync() { return e == hipSuccess && (e = hipStreamSynchronize(stream)) == hipSuccess; }
    bool launched() { return e == hipSuccess && (e = hipGetLastError()) == hipSuccess; }
    bool launch_from(int kid, int64_t g0, int64_t g1, const KswArgs &a) {
        if (e != hipSuccess) return false;
        if (g1 <= g0) return true;
        launch_row(ksw_syms, kid, g1 - g0, 0, stream, g0, a);
        return launched();
    }
    bool launch(int kid, int64_t n_graphs, const SsspArgs &a) {
        if (e != hipSuccess) return false;
        launch_row(sssp_syms, kid, n_graphs, 0, stream, a);
        return launched();
    }
    int err() {
        if (e == hipSuccess) { set_last_error(std::string(entry) + ": out of host memory"); return AASM_E_NOMEM; }
        set_last_error(hip_err(entry, e));
        return e == hipErrorOutOfMemory ? AASM_E_NOMEM : AASM_E_HIP;
    }
};

// A generic graph entry after its argument checks (rc, with their message in why): the device, then run(GraphGpu &) - the driver,
// which may set why too.  Nothing touches a device unless the checks pass.
template <class Run> static int graph_entry(const char *entry, int rc, const char *const &why, int device, Run run) {
    if (rc == AASM_OK && (rc = ctx_init(device)) == AASM_OK) {
        hipSetDevice(device);
        GraphGpu be{g_ctx[device].stream, entry};
        rc = run(be);
    }
    if (*why) set_last_error(std::string(entry) + ": " + why);
    return rc;
}

}  // namespace aasm

using namespace aasm;
static inline bool host_coord_ok(int64_t x) { return x >= 0 && x < AASM_COORD_LIMIT; }

struct aasm_result {
    int device;
    uint64_t generation;
    WS w;
    PipelineSizes sz;
    aasm_stats stats;
    std::map<std::string, std::pair<void *, size_t>> named;
    hipStream_t stream;
    PackWS pk;                           // scratch + sizes of the device-side export
};

// record (index in the batch handed to the failing solve) whose cs tag the device rejected
static thread_local int64_t g_bad_record = -1;

static int solve_on_device(DevCtx &cx, const aasm_batch_in &dev_in, const aasm_opts &opts, hipStream_t stream, aasm_result **res_out,
                           GpuBackend **be_out) {
    GpuBackend *be = *be_out;
    const bool timing = opts.collect_timing != 0;
    aasm_result *res = new aasm_result();
    res->device = cx.device; res->stream = stream;
    std::memset(&res->stats, 0, sizeof(res->stats));
    if (timing) hipEventRecord(cx.ev_t0, stream);
    be->test_dirty_scan = decode_hooks(opts).dirty_scan;            // test hook: the next scan finds a ticket counter an aborted launch left behind
    int rc = run_pipeline(*be, dev_in, opts, res->w, res->sz);
    if (rc == AASM_OK) rc = pack_alloc(*be, res->w, res->pk);       // the scratch of a later device-side export
    be->flush_zero();
    if (timing) hipEventRecord(cx.ev_t1, stream);
    be->join();
    be->join2();
    hipError_t e = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = hipStreamSynchronize(cx.side);
    if (e == hipSuccess) e = hipStreamSynchronize(cx.side2);
    be->scan_stalled();
    if (rc == AASM_OK && be->failed()) rc = be->oom() ? AASM_E_NOMEM : AASM_E_HIP;
    if (rc == AASM_OK && e != hipSuccess) { set_last_error(hip_err("pipeline", e)); rc = AASM_E_HIP; }
    if (rc == AASM_E_PARSE) {
        g_bad_record = res->sz.bad_record;
        set_last_error("malformed cs:Z tag in record " + std::to_string(res->sz.bad_record) + " of the batch");
    }
    if (rc == AASM_E_HIP || rc == AASM_E_NOMEM || be->failed() || cx.pinned[SCAN_STALL_SLOT] != 0) {
        // a scan that did not run to its end (failed launch, aborted kernel) leaves tickets / tile words behind, and the single-pass
        // scan of the NEXT solve on this context relies on finding them zero: wipe both scratch buffers before anybody else comes
        // (whatever code the solve itself ends with: a raised stall flag left behind would fail every later solve on the context)
        (void)hipDeviceSynchronize();
        if (cx.d_scratch) (void)hipMemset(cx.d_scratch, 0, cx.d_scratch_cap * 8);
        if (cx.d_scratch2) (void)hipMemset(cx.d_scratch2, 0, cx.d_scratch2_cap * 8);
        cx.pinned[SCAN_STALL_SLOT] = 0;
        (void)hipGetLastError();
    }
    if (rc != AASM_OK) { delete res; return rc; }
    if (timing) {
        for (int i = 0; i < AASM_N_PHASES; i++)
            if (be->phase_used[i]) { float ms = 0; if (hipEventElapsedTime(&ms, cx.ev_b[i], cx.ev_e[i]) == hipSuccess) res->stats.phase_ms[i] = ms; }
        float ms = 0;
        if (hipEventElapsedTime(&ms, cx.ev_t0, cx.ev_t1) == hipSuccess) res->stats.total_ms = ms;
    }
    {   // counters are tiny: read them now so stats are available without a full fetch
        int64_t cnt[CNT_N];
        std::memset(cnt, 0, sizeof(cnt));
        be->d2h(cnt, res->w.counters, sizeof(cnt));
        aasm_stats &st = res->stats;
        st.n_vertices = res->sz.VT; st.n_edges = res->sz.ET;
        st.n_pairs = res->sz.S > 0 ? be->read_i64(res->w.ov_rank + res->sz.S) : 0;
        st.n_heap_nodes = cnt[CNT_HEAPNODES]; st.n_paths_found = cnt[CNT_PATHS]; st.n_paths_converted = cnt[CNT_CONVERTED];
        st.n_unconnectable = cnt[CNT_UNCONN]; st.range_steps = cnt[CNT_RANGE_STEPS];
        st.ispr_edges = cnt[CNT_ISPR_E]; st.ispr_vertices = cnt[CNT_ISPR_V]; st.path_edges = cnt[CNT_PATH_E];
        st.out_elems = cnt[CNT_OUT_E]; st.pq_pushes = cnt[CNT_PQ_PUSH];
        if (be->failed()) { delete res; return AASM_E_HIP; }
    }
    res->stats.device_bytes = (int64_t)be->bytes;
    res->generation = cx.generation;
    res->named = be->named;
    *res_out = res;
    return AASM_OK;
}

extern "C" {

int aasm_abi_version(void) { return AASM_ABI_VERSION; }

int aasm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int aasm_init(int device) { return ctx_init(device); }

int aasm_solve_device(const aasm_batch_in *dev_in, const aasm_opts *opts, void *stream, aasm_result **res) {
    if (!dev_in || !res) return AASM_E_INVAL;
    aasm_opts o;
    std::memset(&o, 0, sizeof(o));
    if (opts) o = *opts;
    int rc = ctx_init(o.device);
    if (rc != AASM_OK) return rc;
    DevCtx &cx = g_ctx[o.device];
    std::lock_guard<std::mutex> lk(cx.mu);
    hipSetDevice(o.device);
    hipStream_t s = stream ? (hipStream_t)stream : cx.stream;
    GpuBackend be(cx, s, o.collect_timing != 0);
    if (const int pz = poison_byte()) be.poison_arena(pz);
    GpuBackend *bp = &be;
    return solve_on_device(cx, *dev_in, o, s, res, &bp);
}

int aasm_result_stats(const aasm_result *res, aasm_stats *stats) {
    if (!res || !stats) return AASM_E_INVAL;
    *stats = res->stats;
    return AASM_OK;
}

// minimal backend view for fetch (D2H only)
namespace {
#define AASM_STAGE_BYTES ((size_t)16 << 20)
struct FetchBackend {
    DevCtx &cx; hipStream_t stream; bool fail = false;
    void d2h(void *dst, const void *src, size_t n) {
        if (fail || n == 0) return;
        hipError_t e = hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) { set_last_error(hip_err("hipMemcpy D2H", e)); fail = true; }
    }
    // Large result arrays: a copy into pageable memory goes through the runtime's own staging at a few GB/s and
    // first-touches every destination page on one thread.  Here the DMA lands in two pinned 16 MB chunks in turn
    // while host threads move the chunk before it into the caller's array (page faults spread over the threads).
    void d2h_big(void *dst, const void *src, size_t n) {
        if (fail || n == 0) return;
        if (n < (AASM_STAGE_BYTES >> 2)) { d2h(dst, src, n); return; }
        for (int i = 0; i < 2; i++)
            if (!cx.stage[i] && hipHostMalloc((void **)&cx.stage[i], AASM_STAGE_BYTES) != hipSuccess) { (void)hipGetLastError(); cx.stage[i] = nullptr; d2h(dst, src, n); return; }
        const size_t nchunks = (n + AASM_STAGE_BYTES - 1) / AASM_STAGE_BYTES;
        const int T = std::max(1, std::min(host_threads(), 16));
        auto issue = [&](size_t c) {
            const size_t off = c * AASM_STAGE_BYTES, len = std::min(AASM_STAGE_BYTES, n - off);
            return hipMemcpyAsync(cx.stage[c & 1], (const char *)src + off, len, hipMemcpyDeviceToHost, stream);
        };
        hipError_t e = issue(0);
        for (size_t c = 0; c < nchunks && e == hipSuccess; c++) {
            e = hipStreamSynchronize(stream);                        // chunk c has landed
            if (e != hipSuccess) break;
            if (c + 1 < nchunks) e = issue(c + 1);                   // the next DMA runs beside the host copy of this one
            const size_t off = c * AASM_STAGE_BYTES, len = std::min(AASM_STAGE_BYTES, n - off);
            const char *from = cx.stage[c & 1];
            char *to = (char *)dst + off;
            std::vector<std::thread> th;
            for (int t = 1; t < T; t++) th.emplace_back([=] { const size_t a = len * t / T, b = len * (t + 1) / T; std::memcpy(to + a, from + a, b - a); });
            std::memcpy(to, from, len / T);
            for (auto &x : th) x.join();
        }
        if (e != hipSuccess) { set_last_error(hip_err("hipMemcpy D2H", e)); fail = true; }
    }
};
}

int aasm_result_fetch(aasm_result *res, aasm_batch_out *out) {
    if (!res || !out) return AASM_E_INVAL;
    DevCtx &cx = g_ctx[res->device];
    std::lock_guard<std::mutex> lk(cx.mu);
    if (res->generation != cx.generation) { set_last_error("result was invalidated by a later solve on the same device"); return AASM_E_INVAL; }
    hipSetDevice(res->device);
    FetchBackend fb{cx, res->stream};
    int rc = fetch_results(fb, res->w, res->sz, out);
    if (fb.fail) { aasm_free_out(out); return AASM_E_HIP; }
    if (rc != AASM_OK) return rc;
    // keep the device-side timers / sizes
    aasm_stats st = out->stats;
    std::memcpy(st.phase_ms, res->stats.phase_ms, sizeof(st.phase_ms));
    st.total_ms = res->stats.total_ms; st.device_bytes = res->stats.device_bytes;
    std::memcpy(st.reserved_f, res->stats.reserved_f, sizeof(st.reserved_f));
    out->stats = st;
    return AASM_OK;
}

// ---- results on the device (aasm_result_sizes / aasm_result_export) ----
int aasm_result_sizes(aasm_result *res, aasm_out_sizes *sz) {
    if (!res || !sz) return AASM_E_INVAL;
    DevCtx &cx = g_ctx[res->device];
    std::lock_guard<std::mutex> lk(cx.mu);
    if (res->generation != cx.generation) { set_last_error("result was invalidated by a later solve on the same device"); return AASM_E_INVAL; }
    hipSetDevice(res->device);
    GpuBackend be(cx, res->stream, GpuBackend::Attach{});
    const int rc = pack_sizes(be, res->w, res->pk);                 // (the first call ends in one read-back: a wait on the result's stream)
    if (rc != AASM_OK) { if (rc == AASM_E_OVERFLOW) set_last_error("result too large for the device-side export"); return rc; }
    sz->n_contigs = res->pk.sizes[0]; sz->n_main = res->pk.sizes[1]; sz->n_alt = res->pk.sizes[2];
    sz->n_all_paths = res->pk.sizes[3]; sz->n_all_elems = res->pk.sizes[4];
    return AASM_OK;
}

// a non-empty destination array: device memory of `device`, aligned to `align`
static bool dev_buffer_ok(const void *p, int64_t n, size_t align, int device) {
    if (n <= 0) return true;
    if (!p || ((uintptr_t)p % align) != 0) return false;
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof(at));
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }   // (unregistered host memory)
    return at.type == hipMemoryTypeDevice && at.device == device;
}

int aasm_result_export(aasm_result *res, const aasm_out_sizes *sz, const aasm_dev_out *dst, void *stream) {
    if (!res || !sz || !dst) return AASM_E_INVAL;
    DevCtx &cx = g_ctx[res->device];
    std::lock_guard<std::mutex> lk(cx.mu);
    if (res->generation != cx.generation) { set_last_error("result was invalidated by a later solve on the same device"); return AASM_E_INVAL; }
    const int64_t *k = res->pk.sizes;
    if (!res->pk.sized || sz->n_contigs != k[0] || sz->n_main != k[1] || sz->n_alt != k[2] || sz->n_all_paths != k[3] || sz->n_all_elems != k[4]) {
        set_last_error("sizes are not what aasm_result_sizes returned for this result");
        return AASM_E_INVAL;
    }
    hipSetDevice(res->device);
    const int dv = res->device;
    const int64_t C = k[0];
    if (!dev_buffer_ok(dst->main_off, C + 1, 8, dv) || !dev_buffer_ok(dst->alt_off, C + 1, 8, dv) || !dev_buffer_ok(dst->all_path_off, C + 1, 8, dv) ||
        !dev_buffer_ok(dst->all_elem_off, k[3] + 1, 8, dv) || !dev_buffer_ok(dst->main_elems, k[1], 8, dv) || !dev_buffer_ok(dst->alt_elems, k[2], 8, dv) ||
        !dev_buffer_ok(dst->all_elems, k[4], 8, dv) || !dev_buffer_ok(dst->ctg_status, C, 4, dv)) {
        set_last_error("a destination array is NULL, not device memory of the result's device, or misaligned");
        return AASM_E_INVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    {   // forget the exports that have finished (a caller may export one result many times between two solves)
        size_t j = 0;
        for (hipEvent_t ev : cx.export_events) { if (hipEventQuery(ev) == hipSuccess) (void)hipEventDestroy(ev); else cx.export_events[j++] = ev; }
        cx.export_events.resize(j);
        (void)hipGetLastError();
    }
    // after the solve's work (aasm_result_sizes has waited for it already; the event keeps the order explicit), and the next
    // solve on the device waits for this export before it reuses the arena (drain_exports)
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    hipError_t e = hipEventCreateWithFlags(&ev_in, hipEventDisableTiming);
    if (e == hipSuccess) { cx.export_events.push_back(ev_in); e = hipEventCreateWithFlags(&ev_out, hipEventDisableTiming); }
    if (e == hipSuccess) { cx.export_events.push_back(ev_out); e = hipEventRecord(ev_in, res->stream); }
    if (e == hipSuccess) e = hipStreamWaitEvent(s, ev_in, 0);
    if (e != hipSuccess) { set_last_error(hip_err("export ordering", e)); return AASM_E_HIP; }
    GpuBackend be(cx, s, GpuBackend::Attach{});
    pack_export(be, res->w, res->pk, *dst);
    if (be.failed()) return AASM_E_HIP;
    if ((e = hipEventRecord(ev_out, s)) != hipSuccess) { set_last_error(hip_err("hipEventRecord", e)); return AASM_E_HIP; }
    return AASM_OK;
}

// ---- cut plans of an exported result (aasm_cut.h): one launch on the caller's stream, nothing else ----
namespace {
struct CutGpu {
    hipStream_t stream;
    hipError_t err = hipSuccess;
    void launch_cut(int kc, int64_t nblocks, int nthreads, const CutArgs &a) {
        launch_row(cut_syms, kc, nblocks, nthreads, stream, a);
        err = hipGetLastError();
    }
};
}
// the arrays a cut-plan launch touches (and a rows launch, which reads the plans): device memory of `device`, aligned
static bool cut_arrays_ok(const aasm_batch_in &in, const aasm_dev_out &o, const aasm_dev_cuts &d, const CutArgs &a, int device) {
    const int64_t C = a.C, R = a.R;
    return dev_buffer_ok(in.ctg_rec_off, C + 1, 8, device) && dev_buffer_ok(in.qry_str, R, 8, device) && dev_buffer_ok(in.qry_end, R, 8, device) &&
           dev_buffer_ok(in.aln_fwd, R, 1, device) && dev_buffer_ok(in.rec_cs_off, R + 1, 8, device) &&
           dev_buffer_ok(in.cs_text, R > 0 ? 1 : 0, 1, device) &&     // (the text's length is rec_cs_off[R], on the device: only its base is checked)
           dev_buffer_ok(o.main_off, C + 1, 8, device) && dev_buffer_ok(o.alt_off, C + 1, 8, device) && dev_buffer_ok(o.all_path_off, C + 1, 8, device) &&
           dev_buffer_ok(o.all_elem_off, a.NP + 1, 8, device) && dev_buffer_ok(o.main_elems, a.n[0], 8, device) &&
           dev_buffer_ok(o.alt_elems, a.n[1], 8, device) && dev_buffer_ok(o.all_elems, a.n[2], 8, device) &&
           dev_buffer_ok(d.main, a.n[0], 8, device) && dev_buffer_ok(d.alt, a.n[1], 8, device) && dev_buffer_ok(d.all, a.n[2], 8, device);
}
int aasm_cut_plans_device(const aasm_batch_in *dev_in, const aasm_out_sizes *sz, const aasm_dev_out *dev_out, const aasm_dev_cuts *dst,
                          int device, void *stream) {
    if (!dev_in || !sz || !dev_out || !dst) return AASM_E_INVAL;
    if (!dev_in->cs_text || !dev_in->rec_cs_off) { set_last_error("the device batch carries no cs text (it was uploaded with match ranges)"); return AASM_E_INVAL; }
    CutArgs a;
    if (!cut_args(*dev_in, *sz, *dev_out, *dst, a)) { set_last_error("sizes do not fit the batch"); return AASM_E_INVAL; }
    int rc = ctx_init(device);
    if (rc != AASM_OK) return rc;
    hipSetDevice(device);
    if (!cut_arrays_ok(*dev_in, *dev_out, *dst, a, device)) {
        set_last_error("an array is NULL, not device memory of the device, or misaligned");
        return AASM_E_INVAL;
    }
    CutGpu be{(hipStream_t)stream};
    cut_launch(be, a);
    if (be.err != hipSuccess) { set_last_error(hip_err("kernel launch", be.err)); return AASM_E_HIP; }
    return AASM_OK;
}

void aasm_result_free(aasm_result *res) { delete res; }

void aasm_free_out(aasm_batch_out *out) {
    if (!out) return;
    free(out->main_off); free(out->alt_off); free(out->all_path_off); free(out->all_elem_off);
    free(out->main_elems); free(out->alt_elems); free(out->all_elems); free(out->ctg_status);
    std::memset(out, 0, sizeof(*out));
}

// Test entry (row T1): evaluates the device's PafDistance predicates on n pairs of host tuples.
int aasm_debug_predicates(const int64_t *a, const int64_t *b, int64_t n, uint8_t *out, int device) {
    if (!a || !b || !out || n <= 0) return AASM_E_INVAL;
    int rc = ctx_init(device);
    if (rc != AASM_OK) return rc;
    hipSetDevice(device);
    GraphGpu be{g_ctx[device].stream, "aasm_debug_predicates"};
    DevMem<GraphGpu> m{be};
    const int64_t *da = (const int64_t *)m.up(a, (size_t)n * 40), *db = (const int64_t *)m.up(b, (size_t)n * 40);
    uint8_t *dout = (uint8_t *)m.alloc((size_t)n);
    if (!m.ok) return be.err();
    hipLaunchKernelGGL(aasm_t1_predicates, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, be.stream, da, db, n, dout);
    if (!be.launched() || !be.d2h(out, dout, (size_t)n)) return be.err();
    return AASM_OK;
}

// Test entry (hazard B1): K1's std::sort replay alone, on arbitrary keys.  rec_off[n_contigs + 1] from 0; perm_out[r] per
// record = the input index (relative to its contig) that std::sort leaves at sorted position r.  depth_test as AASM_H2_SORT_DEPTH_MASK.
int aasm_debug_sort_replay(const int64_t *rec_off, int64_t n_contigs, const int64_t *qs, const int64_t *qe, int32_t *perm_out, int depth_test, int device) {
    if (!rec_off || !qs || !qe || !perm_out || n_contigs <= 0 || rec_off[0] != 0) return AASM_E_INVAL;
    for (int64_t c = 0; c < n_contigs; c++) if (rec_off[c + 1] < rec_off[c]) return AASM_E_INVAL;
    const int64_t R = rec_off[n_contigs];
    if (R <= 0 || R > INT32_MAX) return AASM_E_INVAL;
    int rc = ctx_init(device);
    if (rc != AASM_OK) return rc;
    hipSetDevice(device);
    GraphGpu be{g_ctx[device].stream, "aasm_debug_sort_replay"};
    DevMem<GraphGpu> m{be};
    auto filled = [&](size_t bytes, int byte) { void *p = m.alloc(bytes); if (m.ok && !be.fill(p, byte, bytes)) m.ok = false; return p; };
    WS w;
    std::memset(&w, 0, sizeof(w));
    w.C = n_contigs; w.R = R; w.R0 = 0; w.sort_depth_test = depth_test;
    w.rec_off = (const int64_t *)m.up(rec_off, (size_t)(n_contigs + 1) * 8);
    w.in_qs = (const int64_t *)m.up(qs, (size_t)R * 8); w.in_qe = (const int64_t *)m.up(qe, (size_t)R * 8);
    w.s_qs = (int64_t *)filled((size_t)R * 8, 0); w.s_qe = (int64_t *)filled((size_t)R * 8, 0); w.s_orig = (int32_t *)filled((size_t)R * 4, 0);
    w.perm = (int32_t *)filled((size_t)R * 4, 0xff);
    std::vector<int32_t> ones((size_t)n_contigs, 1);
    w.dupflag = (int32_t *)m.up(ones.data(), (size_t)n_contigs * 4);
#if defined(AASM_KPROF)
    w.prof_heap = (int64_t *)filled((size_t)n_contigs * 64, 0);
#endif
    if (!m.ok) return be.err();
    launch_row(pipeline_syms, KN_SORT_FIX, n_contigs, 0, be.stream, w);
    if (!be.launched() || !be.d2h(perm_out, w.perm, (size_t)R * 4)) return be.err();
#if defined(AASM_KPROF)
    {                                                                // diagnostic build: mean cycles per section over the contigs
        std::vector<int64_t> kp((size_t)n_contigs * 8);
        be.d2h(kp.data(), w.prof_heap, kp.size() * 8);
        double mean[8] = {0};
        for (int64_t c = 0; c < n_contigs; c++) for (int i = 0; i < 8; i++) mean[i] += (double)kp[(size_t)c * 8 + i] / (double)n_contigs;
        fprintf(stderr, "sort_fix sections (mean cycles): load %.0f  A %.0f  B %.0f  C %.0f  global partitions %.0f  wave lifetime %.1f us\n", mean[0], mean[1], mean[2], mean[3], mean[4], mean[7] / 100.0);
    }
#endif
    return AASM_OK;
}

// dijkstra (k_shortest_walks.hpp:69-87) over a batch of graphs; host pointers in and out
int aasm_sssp_dijkstra(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5,
                       const int32_t *src, int64_t *d5, int32_t *prev, int device) {
    const char *why = "";
    const int rc = dijkstra_check_args(n_graphs, g_voff, rowptr, col, w5, src, d5, prev, &why);
    return graph_entry("aasm_sssp_dijkstra", rc, why, device, [&](GraphGpu &be) { return dijkstra_run(be, n_graphs, g_voff, rowptr, col, w5, src, d5, prev, &why); });
}

// bellman_ford (k_shortest_walks.hpp:91-129) over a batch of graphs; host pointers in and out
int aasm_sssp_bellman_ford(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5,
                           const int32_t *src, int64_t *d5, int32_t *prev, int32_t *status, int64_t *cycle_off, int32_t *cycle, int device) {
    const char *why = "";
    const int rc = bellman_ford_check_args(n_graphs, g_voff, rowptr, col, w5, src, d5, prev, status, cycle_off, cycle, &why);
    return graph_entry("aasm_sssp_bellman_ford", rc, why, device, [&](GraphGpu &be) {
        return bellman_ford_run(be, n_graphs, g_voff, rowptr, col, w5, src, d5, prev, status, cycle_off, cycle, nullptr, &why);
    });
}

// topology_sort (k_shortest_walks.hpp:132-156) over a batch of graphs; host pointers in and out
int aasm_topology_sort(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, int32_t *order, int32_t *status,
                       int device) {
    const char *why = "";
    const int rc = dag_check_args(n_graphs, g_voff, rowptr, col, nullptr, nullptr, nullptr, nullptr, order, status, true, &why);
    return graph_entry("aasm_topology_sort", rc, why, device, [&](GraphGpu &be) {
        return dag_run(be, n_graphs, g_voff, rowptr, col, nullptr, nullptr, nullptr, nullptr, order, status, &why);
    });
}

// shortest_path_dag (k_shortest_walks.hpp:160-175) over a batch of graphs, with its topology_sort where order is given
int aasm_sssp_dag(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5, const int32_t *src,
                  int64_t *d5, int32_t *prev, int32_t *order, int32_t *status, int device) {
    const char *why = "";
    const int rc = dag_check_args(n_graphs, g_voff, rowptr, col, w5, src, d5, prev, order, status, false, &why);
    return graph_entry("aasm_sssp_dag", rc, why, device, [&](GraphGpu &be) {
        return dag_run(be, n_graphs, g_voff, rowptr, col, w5, src, d5, prev, order, status, &why);
    });
}

// Dial's bucketed BFS (k_weighted_bfs.hpp:16-37) over a batch of graphs; host pointers in and out
int aasm_sssp_dial(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int32_t *cost,
                   const int32_t *src, int lim, int64_t *dist, int64_t *pre, int device) {
    const char *why = "";
    const int rc = dial_check_args(n_graphs, g_voff, rowptr, col, cost, src, lim, dist, pre, &why);
    return graph_entry("aasm_sssp_dial", rc, why, device, [&](GraphGpu &be) { return dial_run(be, n_graphs, g_voff, rowptr, col, cost, src, lim, dist, pre, &why); });
}

// ---- resident graph batches (aasm_graphs.h): the five entries above with device pointers in and out, on the caller's stream ----
extern "C++" {
namespace {
// The backend of one call on a resident batch: the call's stream; memory that outlives it (the handle frees it).
struct GraphsGpu {
    int device;
    hipStream_t stream;
    hipEvent_t ev;                                                   // the handle's event (nullptr while the handle is being made)
    hipStream_t last;                                                // the stream of the handle's latest call
    hipError_t e = hipSuccess;
    bool entered = false;                                            // something was enqueued
    // before the call's first enqueue: a stream other than the latest call's waits for that call's event
    bool ready() {
        if (!entered) { entered = true; if (ev && stream != last && e == hipSuccess) e = hipStreamWaitEvent(stream, ev, 0); }
        return e == hipSuccess;
    }
    void *alloc(size_t n) {
        void *p = nullptr;
        if (e != hipSuccess) return nullptr;
        if ((e = hipMalloc(&p, n ? n : 16)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        return p;
    }
    void free_dev(void *p) { (void)hipFree(p); }
    bool h2d(void *d, const void *h, size_t n) { return ready() && (e = hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, stream)) == hipSuccess; }
    bool fill(void *d, int byte, size_t n) { return ready() && (e = hipMemsetAsync(d, byte, n, stream)) == hipSuccess; }
    bool d2d(void *d, const void *s, size_t n) { return ready() && (n == 0 || (e = hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, stream)) == hipSuccess); }
    bool sync() { return e == hipSuccess && (e = hipStreamSynchronize(stream)) == hipSuccess; }
    bool read(void *h, const void *d, size_t n) {
        if (ready()) e = hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, stream);
        return sync();
    }
    void poison(void *d, size_t n) { if (const int pz = poison_byte()) { if (n) fill(d, pz, n); } }
    void quiesce() { if (ev && e == hipSuccess) e = hipEventSynchronize(ev); }
    bool dev_ok(const void *p, int64_t n, size_t align) { return dev_buffer_ok(p, n, align, device); }
    bool launched() { return e == hipSuccess && (e = hipGetLastError()) == hipSuccess; }
    bool launch_gr(int kid, int64_t nblocks, const GraphsArgs &a) {
        if (!ready()) return false;
        launch_row(graphs_syms, kid, nblocks, 0, stream, a);
        return launched();
    }
    bool launch(int kid, int64_t n_graphs, const SsspArgs &a) {
        if (!ready()) return false;
        launch_row(sssp_syms, kid, n_graphs, 0, stream, a);
        return launched();
    }
    bool launch_ksw(int kid, int64_t n_graphs, const KswArgs &a) {
        if (!ready()) return false;
        launch_row(ksw_syms, kid, n_graphs, 0, stream, (int64_t)0, a);
        return launched();
    }
    int err() {
        if (e == hipSuccess) { e = hipErrorOutOfMemory; }
        return e == hipErrorOutOfMemory ? AASM_E_NOMEM : AASM_E_HIP;
    }
};
}  // namespace

struct aasm_graphs {
    int device;
    GraphsCore *core;
    hipEvent_t ev;                                                   // recorded behind each call
    hipStream_t last;                                                // the stream of the latest call
    std::mutex mu;
};

// rc of a creation or a call as the entry returns it: the checks' message, or the HIP error's
static int graphs_result(const char *entry, int rc, const char *why, const GraphsGpu &be) {
    if (rc == AASM_OK) return rc;
    if (*why) set_last_error(std::string(entry) + ": " + why);
    else set_last_error(be.e == hipSuccess ? std::string(entry) + ": failed" : hip_err(entry, be.e));
    return rc;
}
static int graphs_make(const char *entry, const aasm_graphs_in *in, int device, hipStream_t stream, bool wrap, aasm_graphs **gb) {
    if (!in || !gb) { set_last_error(std::string(entry) + ": NULL argument"); return AASM_E_INVAL; }
    *gb = nullptr;
    const char *why = "";
    GraphsGpu be{device, stream, nullptr, nullptr};
    int rc = wrap ? AASM_OK : graphs_check_host(*in, &why);          // (an upload is checked on the host, before any device is touched)
    if (rc != AASM_OK) return graphs_result(entry, rc, why, be);
    if ((rc = ctx_init(device)) != AASM_OK) return rc;
    hipSetDevice(device);
    if (!wrap) be.stream = g_ctx[device].stream;
    GraphsCore *core = nullptr;
    rc = wrap ? graphs_wrap(be, *in, &core, &why) : graphs_upload(be, *in, &core);
    if (rc != AASM_OK) return graphs_result(entry, rc, why, be);
    aasm_graphs *h = new aasm_graphs;
    h->device = device; h->core = core; h->last = be.stream;
    if ((be.e = hipEventCreateWithFlags(&h->ev, hipEventDisableTiming)) != hipSuccess || (be.e = hipEventRecord(h->ev, be.stream)) != hipSuccess) {
        graphs_destroy(be, core);
        delete h;
        return graphs_result(entry, AASM_E_HIP, why, be);
    }
    *gb = h;
    return AASM_OK;
}
// One call on a handle: under its lock; a stream other than the latest call's waits for that call's event first; run(be, why) is the
// driver; the event is recorded behind whatever was enqueued.
template <class Run> static int graphs_call(const char *entry, aasm_graphs *gb, void *stream, Run run) {
    if (!gb) { set_last_error(std::string(entry) + ": NULL handle"); return AASM_E_INVAL; }
    std::lock_guard<std::mutex> lk(gb->mu);
    hipSetDevice(gb->device);
    GraphsGpu be{gb->device, (hipStream_t)stream, gb->ev, gb->last};
    const char *why = "";
    int rc = run(be, &why);
    if (be.entered) {                                                // (a call refused by its checks has enqueued nothing)
        gb->last = be.stream;
        const hipError_t er = hipEventRecord(gb->ev, be.stream);
        if (rc == AASM_OK && er != hipSuccess) { be.e = er; rc = AASM_E_HIP; }
    }
    return graphs_result(entry, rc, why, be);
}
}  // extern "C++"

int aasm_graphs_upload(const aasm_graphs_in *host, int device, aasm_graphs **gb) { return graphs_make("aasm_graphs_upload", host, device, nullptr, false, gb); }
int aasm_graphs_wrap_device(const aasm_graphs_in *dev, int device, void *stream, aasm_graphs **gb) {
    return graphs_make("aasm_graphs_wrap_device", dev, device, (hipStream_t)stream, true, gb);
}
int aasm_graphs_view(const aasm_graphs *gb, aasm_graphs_in *dev_view) {
    if (!gb || !dev_view) return AASM_E_INVAL;
    *dev_view = gb->core->view;
    return AASM_OK;
}
void aasm_graphs_free(aasm_graphs *gb) {
    if (!gb) return;
    hipSetDevice(gb->device);
    (void)hipEventSynchronize(gb->ev);
    GraphsGpu be{gb->device, nullptr, nullptr, nullptr};
    graphs_destroy(be, gb->core);
    (void)hipEventDestroy(gb->ev);
    delete gb;
}
int aasm_sssp_dijkstra_device(aasm_graphs *gb, const int32_t *src, int64_t *d5, int32_t *prev, void *stream) {
    return graphs_call("aasm_sssp_dijkstra_device", gb, stream, [&](GraphsGpu &be, const char **why) { return graphs_dijkstra(be, *gb->core, src, d5, prev, why); });
}
int aasm_sssp_bellman_ford_device(aasm_graphs *gb, const int32_t *src, int64_t *d5, int32_t *prev, int32_t *status, int64_t *cycle_off, int32_t *cycle,
                                  void *stream) {
    return graphs_call("aasm_sssp_bellman_ford_device", gb, stream, [&](GraphsGpu &be, const char **why) {
        return graphs_bellman_ford(be, *gb->core, src, d5, prev, status, cycle_off, cycle, why);
    });
}
int aasm_topology_sort_device(aasm_graphs *gb, int32_t *order, int32_t *status, void *stream) {
    return graphs_call("aasm_topology_sort_device", gb, stream, [&](GraphsGpu &be, const char **why) {
        return graphs_dag(be, *gb->core, nullptr, nullptr, nullptr, order, status, true, why);
    });
}
int aasm_sssp_dag_device(aasm_graphs *gb, const int32_t *src, int64_t *d5, int32_t *prev, int32_t *order, int32_t *status, void *stream) {
    return graphs_call("aasm_sssp_dag_device", gb, stream, [&](GraphsGpu &be, const char **why) {
        return graphs_dag(be, *gb->core, src, d5, prev, order, status, false, why);
    });
}
int aasm_sssp_dial_device(aasm_graphs *gb, const int32_t *src, int64_t *dist, int64_t *pre, int32_t *status, void *stream) {
    return graphs_call("aasm_sssp_dial_device", gb, stream, [&](GraphsGpu &be, const char **why) { return graphs_dial(be, *gb->core, src, dist, pre, status, why); });
}

// k shortest walks on a resident batch: the solve (returns when the sizes are final), and the export into the caller's device arrays
int aasm_k_shortest_walks_device(aasm_graphs *gb, const int32_t *source, const int32_t *sink, int64_t k, int flags, void *stream, aasm_ksw_sizes *sz) {
    return graphs_call("aasm_k_shortest_walks_device", gb, stream, [&](GraphsGpu &be, const char **why) {
        return graphs_ksw(be, *gb->core, source, sink, k, flags, sz, why);
    });
}
int aasm_ksw_export_device(aasm_graphs *gb, const aasm_ksw_sizes *sz, const aasm_ksw_dev_out *dst, void *stream) {
    return graphs_call("aasm_ksw_export_device", gb, stream, [&](GraphsGpu &be, const char **why) { return graphs_ksw_export(be, *gb->core, sz, dst, why); });
}

// k shortest walks (k_shortest_walks.hpp:177-290, is_dag = true) over a batch of DAGs; host pointers in, library-allocated out
int aasm_k_shortest_walks(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5,
                          const int32_t *source, const int32_t *sink, int64_t k, int flags, int device, aasm_ksw_out *out) {
    const char *why = "";
    const int rc = ksw_check_args(n_graphs, g_voff, rowptr, col, w5, source, sink, k, flags, out, &why);
    return graph_entry("aasm_k_shortest_walks", rc, why, device, [&](GraphGpu &be) {
        return ksw_run(be, n_graphs, g_voff, rowptr, col, w5, source, sink, k, flags, out, (int64_t)4 << 30);
    });
}

void aasm_ksw_free(aasm_ksw_out *out) { ksw_free_out(out); }

int aasm_debug_poison(int byte) {
    if (byte < 0 || byte > 255) return -1;
    return g_poison.exchange(byte, std::memory_order_relaxed);
}

int64_t aasm_debug_counter(const char *name) {
    if (!name) return -1;
    const std::string n(name);
    if (n == "range_splits") return g_n_range_splits.load();
    if (n == "device_mallocs") return g_n_device_mallocs.load();
    if (n == "stream_syncs") return g_n_stream_syncs.load();
    if (n == "read_slow_rows") return g_n_read_slow_rows.load();
    if (n == "read_host_fallbacks") return g_n_read_fallbacks.load();
    if (n == "read_containers") return g_n_read_containers.load();
    if (n == "alt_host_verdicts") return g_n_alt_verdicts.load();
    if (n == "alt_device_merges") return g_n_alt_merges.load();
    return -1;
}

int64_t aasm_debug_fetch(aasm_result *res, const char *name, void *dst, int64_t dst_bytes) {
    if (!res || !name) return AASM_E_INVAL;
    DevCtx &cx = g_ctx[res->device];
    std::lock_guard<std::mutex> lk(cx.mu);
    if (res->generation != cx.generation) return AASM_E_INVAL;
    auto it = res->named.find(name);
    if (it == res->named.end()) return AASM_E_INVAL;
    if (dst) {
        hipSetDevice(res->device);
        size_t n = std::min<size_t>((size_t)dst_bytes, it->second.second);
        hipError_t e = hipMemcpy(dst, it->second.first, n, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { set_last_error(hip_err("debug fetch", e)); return AASM_E_HIP; }
    }
    return (int64_t)it->second.second;
}

// Upload a host batch once (bench / repeated solves): returns a device view.
// The upload lives in plain hipMalloc memory owned by the handle (not in the arena).
struct aasm_upload { int device; std::vector<void *> ptrs; aasm_batch_in view; };

static int upload_range(const aasm_batch_in *in, int64_t c0, int64_t c1, int device, aasm_upload **up_out, aasm_batch_in *dev_view) {
    if (!in || !up_out || !dev_view || c0 < 0 || c1 > in->n_contigs || c0 >= c1) return AASM_E_INVAL;
    int rc = ctx_init(device);
    if (rc != AASM_OK) return rc;
    hipSetDevice(device);
    g_ctx[device].input_arrived.store(1);
    aasm_upload *up = new aasm_upload();
    up->device = device;
    bool ok = true, oom = false;
    std::string why = "the batch carries neither match ranges nor cs tags";
    auto put = [&](const void *src, size_t bytes) -> void * {
        void *p = nullptr;
        if (!ok) return nullptr;
        hipError_t e = hipMalloc(&p, bytes ? bytes : 8);
        if (e != hipSuccess) { ok = false; oom = (e == hipErrorOutOfMemory); (void)hipGetLastError(); why = hip_err("hipMalloc(upload)", e); return nullptr; }
        up->ptrs.push_back(p);
        if (bytes && (e = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice)) != hipSuccess) { ok = false; why = hip_err("hipMemcpy H2D", e); }
        return p;
    };
    // rebase the offsets of the contig range [c0, c1) to start at 0
    const int64_t C = c1 - c0, r0 = in->ctg_rec_off[c0], r1 = in->ctg_rec_off[c1], R = r1 - r0;
    const int64_t g0 = in->rec_rng_off[r0], g1 = in->rec_rng_off[r1], G = g1 - g0;
    std::vector<int64_t> coff(C + 1), roff(R + 1);
    for (int64_t c = 0; c <= C; c++) coff[c] = in->ctg_rec_off[c0 + c] - r0;
    for (int64_t r = 0; r <= R; r++) roff[r] = in->rec_rng_off[r0 + r] - g0;
    aasm_batch_in &v = up->view;
    v.n_contigs = C; v.n_records = R; v.n_ranges = G;
    v.ctg_rec_off = (const int64_t *)put(coff.data(), (C + 1) * 8);
    v.qry_str = (const int64_t *)put(in->qry_str + r0, R * 8);
    v.qry_end = (const int64_t *)put(in->qry_end + r0, R * 8);
    v.ref_str = (const int64_t *)put(in->ref_str + r0, R * 8);
    v.ref_end = (const int64_t *)put(in->ref_end + r0, R * 8);
    v.qry_total = (const int64_t *)put(in->qry_total + r0, R * 8);
    v.ref_chr = (const int32_t *)put(in->ref_chr + r0, R * 4);
    v.aln_fwd = (const uint8_t *)put(in->aln_fwd + r0, R);
    v.map_qul = (const uint8_t *)put(in->map_qul + r0, R);
    v.rec_rng_off = (const int64_t *)put(roff.data(), (R + 1) * 8);
    if (in->rng_qry_l) {
        v.rng_qry_l = (const int64_t *)put(in->rng_qry_l + g0, G * 8);
        v.rng_qry_r = (const int64_t *)put(in->rng_qry_r + g0, G * 8);
        v.rng_ref_l = (const int64_t *)put(in->rng_ref_l + g0, G * 8);
    } else if (in->cs_text && in->rec_cs_off) {                     // the device parses the cs tags (aasm_k0_cs_ranges)
        const int64_t t0 = in->rec_cs_off[r0], t1 = in->rec_cs_off[r1];
        std::vector<int64_t> toff(R + 1);
        for (int64_t r = 0; r <= R; r++) toff[r] = in->rec_cs_off[r0 + r] - t0;
        v.cs_text = (const char *)put(in->cs_text + t0, (size_t)(t1 - t0));
        v.rec_cs_off = (const int64_t *)put(toff.data(), (R + 1) * 8);
    } else ok = false;
    if (!ok) {
        for (void *p : up->ptrs) hipFree(p);
        delete up;
        set_last_error("device upload failed: " + why);
        return oom ? AASM_E_NOMEM : AASM_E_HIP;
    }
    *dev_view = up->view;
    *up_out = up;
    return AASM_OK;
}
int aasm_upload_batch(const aasm_batch_in *in, int device, aasm_upload **up_out, aasm_batch_in *dev_view) {
    if (!in) return AASM_E_INVAL;
    return upload_range(in, 0, in->n_contigs, device, up_out, dev_view);
}
void aasm_upload_free(aasm_upload *up) {
    if (!up) return;
    hipSetDevice(up->device);
    for (void *p : up->ptrs) hipFree(p);
    delete up;
}

// ---- the device reader (aasm_read.h): plain hipMalloc blocks (what it hands out goes into an aasm_upload), the context's stream
// and its single-pass scan.  AASM_READ_TIMING: the stages' wall times (a wait on the stream at every stage's end) on stderr.
namespace {
struct ReadGpu {
    DevCtx &cx;
    GpuBackend scans;                                               // (attached: it allocates nothing and leaves the arena alone)
    hipError_t e = hipSuccess;
    bool oom = false;
    std::vector<void *> blocks;
    const bool timing = std::getenv("AASM_READ_TIMING") != nullptr;
    const char *stage_name = nullptr;
    std::chrono::steady_clock::time_point stage_t0;
    explicit ReadGpu(DevCtx &c) : cx(c), scans(c, c.stream, GpuBackend::Attach{}) {}
    ~ReadGpu() { for (void *p : blocks) hipFree(p); }
    bool ok() const { return e == hipSuccess && !oom && !scans.failed(); }
    int code() const { return oom ? AASM_E_NOMEM : AASM_E_HIP; }
    std::string why() const { return oom ? "out of device memory (device reader)" : e != hipSuccess ? hip_err("device reader", e) : std::string(last_error_text()); }
    void *alloc(size_t n) {
        if (!ok()) return nullptr;
        void *p = nullptr;
        const hipError_t r = hipMalloc(&p, n ? n : 8);
        if (r != hipSuccess) { (void)hipGetLastError(); if (r == hipErrorOutOfMemory) oom = true; else e = r; return nullptr; }
        blocks.push_back(p);
        if (const int pz = poison_byte()) { if ((e = hipMemsetAsync(p, pz, n ? n : 8, cx.stream)) != hipSuccess) return nullptr; }
        return p;
    }
    void release(void *p) {
        auto it = std::find(blocks.begin(), blocks.end(), p);
        if (it == blocks.end()) return;
        blocks.erase(it);
        hipFree(p);
    }
    void keep(void *p) { auto it = std::find(blocks.begin(), blocks.end(), p); if (it != blocks.end()) blocks.erase(it); }
    void h2d(void *d, const void *h, size_t n) {
        if (!ok() || n == 0) return;
        e = hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, cx.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(cx.stream);
    }
    void d2h(void *h, const void *d, size_t n) {
        if (!ok() || n == 0) return;
        e = hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, cx.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(cx.stream);
        scans.scan_stalled();
    }
    void fill32(void *p, int32_t v, int64_t count) { if (ok() && count > 0) e = hipMemsetD32Async((hipDeviceptr_t)p, v, (size_t)count, cx.stream); }
    void scan_i32(const int32_t *in, int64_t n, int64_t *out) { if (ok()) scans.scan_i32(in, n, out); }
    void scan_u8(const uint8_t *in, int64_t n, int64_t *out) { if (ok()) scans.scan_u8(in, n, out); }
    void launch_read(int kr, int64_t nblocks, int nthreads, const ReadArgs &a) {
        if (!ok()) return;
        if (timing) e = hipStreamSynchronize(cx.stream);
        const auto t0 = std::chrono::steady_clock::now();
        launch_row(read_syms, kr, nblocks, nthreads, cx.stream, a);
        if (e == hipSuccess) e = hipGetLastError();
        if (timing && e == hipSuccess) {
            e = hipStreamSynchronize(cx.stream);
            std::fprintf(stderr, "aasm read kernel: %-20s %9.3f ms (%lld blocks)\n", (unsigned)kr < KR_N ? read_syms[kr].name : "", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3, (long long)nblocks);
        }
    }
    void launch_alt(int ka, int64_t nblocks, int nthreads, const AltArgs &a) {
        if (!ok()) return;
        launch_row(alt_syms, ka, nblocks, nthreads, cx.stream, a);
        e = hipGetLastError();
    }
    void stage(const char *name) {
        if (!timing) return;
        if (ok()) e = hipStreamSynchronize(cx.stream);
        const auto now = std::chrono::steady_clock::now();
        if (stage_name) std::fprintf(stderr, "aasm read stage: %-14s %9.3f ms\n", stage_name, std::chrono::duration<double>(now - stage_t0).count() * 1e3);
        stage_name = name; stage_t0 = now;
    }
};
}  // namespace

// the text of a device read that failed, for the host reader's verdict: host text as it is, device text copied back once
static int read_verdict(const char *text, int64_t len, bool on_dev, int device) {
    if (!on_dev || len == 0) return read_host_verdict(on_dev ? "" : text, len);
    std::string host;
    try { host.resize((size_t)len); } catch (...) { set_last_error("out of host memory (device reader)"); return AASM_E_NOMEM; }
    hipSetDevice(device);
    const hipError_t e = hipMemcpy(&host[0], text, (size_t)len, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { (void)hipGetLastError(); set_last_error(hip_err("device reader", e)); return AASM_E_HIP; }
    return read_host_verdict(host.data(), len);
}

// aasm_paf_parse_device (dev_cols = nullptr) and aasm_paf_parse_device_rows
static int parse_device(const char *entry, const char *text, int64_t len, int flags, int device, aasm_paf **paf_out, aasm_upload **up_out, aasm_batch_in *dev_view,
                        aasm_row_cols *dev_cols) {
    if (paf_out) *paf_out = nullptr;
    if (up_out) *up_out = nullptr;
    const bool on_dev = (flags & AASM_READ_TEXT_ON_DEVICE) != 0;
    if ((!text && !(on_dev && len == 0)) || len < 0 || (up_out == nullptr) != (dev_view == nullptr) || (!paf_out && !up_out) || (on_dev && paf_out)) {
        set_last_error(std::string(entry) + ": bad argument");
        return AASM_E_INVAL;
    }
    int rc = ctx_init(device);
    if (rc != AASM_OK) return rc;
    if (on_dev && len > 0) {
        hipSetDevice(device);
        if (!dev_buffer_ok(text, len, 16, device)) { set_last_error(std::string(entry) + ": text is not device memory of the device, or not 16-byte aligned"); return AASM_E_INVAL; }
    }
    DevCtx &cx = g_ctx[device];
    aasm_paf *paf = paf_out ? new aasm_paf() : nullptr;
    ReadOut o;
    std::string why;
    {
        std::lock_guard<std::mutex> lk(cx.mu);                      // (the scans' scratch words are the context's)
        hipSetDevice(device);
        ReadGpu be(cx);
        rc = read_run(be, text, len, flags, paf, up_out != nullptr, o);
        if (rc < 0) {
            why = be.why();
            // a scan that did not run to its end leaves its words behind (solve_on_device does the same)
            (void)hipDeviceSynchronize();
            if (cx.d_scratch) (void)hipMemset(cx.d_scratch, 0, cx.d_scratch_cap * 8);
            cx.pinned[SCAN_STALL_SLOT] = 0;
            (void)hipGetLastError();
        }
        if (rc == AASM_OK && up_out) {
            aasm_upload *up = new aasm_upload();
            up->device = device;
            up->ptrs = {o.ctg_rec_off, o.qry_str, o.qry_end, o.ref_str, o.ref_end, o.qry_total, o.ref_chr, o.aln_fwd, o.map_qul, o.rec_rng_off, o.cs_text, o.rec_cs_off};
            aasm_batch_in &v = up->view;
            std::memset(&v, 0, sizeof v);
            v.n_contigs = o.C; v.n_records = o.R; v.n_ranges = o.n_ranges;
            v.ctg_rec_off = o.ctg_rec_off; v.qry_str = o.qry_str; v.qry_end = o.qry_end; v.ref_str = o.ref_str; v.ref_end = o.ref_end; v.qry_total = o.qry_total;
            v.ref_chr = o.ref_chr; v.aln_fwd = o.aln_fwd; v.map_qul = o.map_qul; v.rec_rng_off = o.rec_rng_off; v.cs_text = o.cs_text; v.rec_cs_off = o.rec_cs_off;
            if (dev_cols) {                                         // (the same handle owns the columns' arrays)
                for (void *p : {(void *)o.ref_total, (void *)o.mat_num, (void *)o.aln_len, (void *)o.row_index, (void *)o.cord_type, (void *)o.names, (void *)o.ctg_name_off, (void *)o.chr_name_off})
                    up->ptrs.push_back(p);
                dev_cols->n_chr = o.n_chr; dev_cols->ref_total = o.ref_total; dev_cols->mat_num = o.mat_num; dev_cols->aln_len = o.aln_len;
                dev_cols->row_index = o.row_index; dev_cols->cord_type = o.cord_type; dev_cols->names = o.names;
                dev_cols->ctg_name_off = o.ctg_name_off; dev_cols->chr_name_off = o.chr_name_off;
            }
            *dev_view = v;
            *up_out = up;
        }
    }
    if (rc == AASM_OK) {
        g_n_read_slow_rows.store(o.slow_rows);
        if (paf_out) { *paf_out = paf; g_n_read_containers++; }
        return AASM_OK;
    }
    delete paf;
    if (rc < 0) { set_last_error(std::string(entry) + ": " + why); return rc; }
    // a text the device does not take: not a hot path, and the host reader's code and message are the contract
    g_n_read_fallbacks++;
    return read_verdict(text, len, on_dev, device);
}

int aasm_paf_parse_device(const char *text, int64_t len, int flags, int device, aasm_paf **paf_out, aasm_upload **up_out, aasm_batch_in *dev_view) {
    return parse_device("aasm_paf_parse_device", text, len, flags & ~(AASM_READ_ROW_COLS | AASM_READ_TEXT_ON_DEVICE), device, paf_out, up_out, dev_view, nullptr);
}

int aasm_paf_parse_device_rows(const char *text, int64_t len, int flags, int device, aasm_paf **paf_out, aasm_upload **up_out, aasm_batch_in *dev_view,
                               aasm_row_cols *dev_cols) {
    if (!up_out || !dev_view || !dev_cols) {
        if (paf_out) *paf_out = nullptr;
        if (up_out) *up_out = nullptr;
        set_last_error("aasm_paf_parse_device_rows: bad argument");
        return AASM_E_INVAL;
    }
    return parse_device("aasm_paf_parse_device_rows", text, len, flags | AASM_READ_ROW_COLS, device, paf_out, up_out, dev_view, dev_cols);
}

// a file's bytes, mapped (or read into memory where it is no regular file), through parse(text, len)
static int with_file_text(const char *path, const std::function<int(const char *, int64_t)> &parse) {
    if (!path) return AASM_E_INVAL;
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) { set_last_error(std::string("cannot open ") + path); return AASM_E_IO; }
    struct stat st;
    if (::fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) {             // pipes etc.: read into memory
        std::string data;
        char buf[1 << 16];
        ssize_t n;
        while ((n = ::read(fd, buf, sizeof buf)) > 0) data.append(buf, (size_t)n);
        ::close(fd);
        return parse(data.data(), (int64_t)data.size());
    }
    if (st.st_size == 0) { ::close(fd); return parse("", 0); }
    void *m = ::mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    ::close(fd);
    if (m == MAP_FAILED) { set_last_error(std::string("cannot map ") + path); return AASM_E_IO; }
    ::madvise(m, (size_t)st.st_size, MADV_WILLNEED);
    const int rc = parse((const char *)m, (int64_t)st.st_size);
    ::munmap(m, (size_t)st.st_size);
    return rc;
}

int aasm_paf_read_device(const char *path, int flags, int device, aasm_paf **paf_out, aasm_upload **up_out, aasm_batch_in *dev_view) {
    return with_file_text(path, [&](const char *text, int64_t len) { return aasm_paf_parse_device(text, len, flags, device, paf_out, up_out, dev_view); });
}

int aasm_paf_read_device_rows(const char *path, int flags, int device, aasm_paf **paf_out, aasm_upload **up_out, aasm_batch_in *dev_view, aasm_row_cols *dev_cols) {
    return with_file_text(path, [&](const char *text, int64_t len) {
        return aasm_paf_parse_device_rows(text, len, flags & ~AASM_READ_TEXT_ON_DEVICE, device, paf_out, up_out, dev_view, dev_cols);
    });
}

// ---- the --alt merge on a resident batch (aasm_alt.h): the reader's backend, the merged arrays in a handle of their own
int aasm_paf_merge_alt_device(const aasm_batch_in *dev_in, const aasm_row_cols *dev_cols, const char *alt_text, int64_t alt_len, double alt_baseline,
                              int flags, int device, aasm_upload **up_out, aasm_batch_in *merged_view, aasm_row_cols *merged_cols) {
    if (up_out) *up_out = nullptr;
    auto inval = [](const char *what) { set_last_error(std::string("aasm_paf_merge_alt_device: ") + what); return AASM_E_INVAL; };
    if (!dev_in || !dev_cols || !up_out || !merged_view || !merged_cols || alt_len < 0 || (!alt_text && alt_len > 0)) return inval("bad argument");
    if (dev_in->rng_qry_l || dev_in->rng_qry_r || dev_in->rng_ref_l || !dev_in->cs_text || !dev_in->rec_cs_off) return inval("the batch is not in its cs form (cs_text / rec_cs_off, no rng_*)");
    const int64_t C = dev_in->n_contigs, R = dev_in->n_records;
    if (C <= 0 || R <= 0 || R > INT32_MAX || dev_cols->n_chr < 0 || dev_cols->n_chr > INT32_MAX / 2) return inval("bad counts");
    int rc = ctx_init(device);
    if (rc != AASM_OK) return rc;
    hipSetDevice(device);
    const aasm_batch_in &in = *dev_in;
    const aasm_row_cols &cl = *dev_cols;
    if (!dev_buffer_ok(in.ctg_rec_off, C + 1, 8, device) || !dev_buffer_ok(in.qry_str, R, 8, device) || !dev_buffer_ok(in.qry_end, R, 8, device) ||
        !dev_buffer_ok(in.ref_str, R, 8, device) || !dev_buffer_ok(in.ref_end, R, 8, device) || !dev_buffer_ok(in.qry_total, R, 8, device) ||
        !dev_buffer_ok(in.ref_chr, R, 4, device) || !dev_buffer_ok(in.aln_fwd, R, 1, device) || !dev_buffer_ok(in.map_qul, R, 1, device) ||
        !dev_buffer_ok(in.rec_rng_off, R + 1, 8, device) || !dev_buffer_ok(in.rec_cs_off, R + 1, 8, device) || !dev_buffer_ok(in.cs_text, 1, 1, device) ||
        !dev_buffer_ok(cl.ref_total, R, 8, device) || !dev_buffer_ok(cl.mat_num, R, 4, device) || !dev_buffer_ok(cl.aln_len, R, 4, device) ||
        !dev_buffer_ok(cl.row_index, R, 4, device) || !dev_buffer_ok(cl.cord_type, R, 1, device) || !dev_buffer_ok(cl.names, 1, 1, device) ||
        !dev_buffer_ok(cl.ctg_name_off, C + 1, 8, device) || !dev_buffer_ok(cl.chr_name_off, cl.n_chr + 1, 8, device))
        return inval("an array of the batch or of its row columns is NULL or not device memory of the device");
    DevCtx &cx = g_ctx[device];
    AltOut o;
    std::string why;
    {
        std::lock_guard<std::mutex> lk(cx.mu);                      // (the scans' scratch words are the context's)
        hipSetDevice(device);
        ReadGpu be(cx);
        rc = alt_merge_run(be, in, cl, alt_text, alt_len, alt_baseline, flags, o);
        if (rc < 0) {
            why = be.why();
            (void)hipDeviceSynchronize();                           // (a scan that did not run to its end leaves its words behind: parse_device)
            if (cx.d_scratch) (void)hipMemset(cx.d_scratch, 0, cx.d_scratch_cap * 8);
            cx.pinned[SCAN_STALL_SLOT] = 0;
            (void)hipGetLastError();
        }
    }
    if (rc < 0) { set_last_error("aasm_paf_merge_alt_device: " + why); return rc; }
    if (rc == AASM_ALT_DECLINED) { g_n_alt_verdicts++; return alt_host_says(alt_text, alt_len, o); }
    aasm_upload *up = new aasm_upload();
    up->device = device;
    up->ptrs = alt_out_arrays(o);
    alt_out_views(o, up->view, *merged_cols);
    *merged_view = up->view;
    *up_out = up;
    g_n_alt_merges++;
    return AASM_OK;
}

// ---- output rows on the device (aasm_rows.h) ----------------------------------------------------------------------------------
// aasm_paf_upload_rows: plain hipMalloc memory owned by the handle, as an uploaded batch's
int aasm_paf_upload_rows(const aasm_paf *paf, int64_t c0, int64_t c1, int device, aasm_upload **up_out, aasm_row_cols *dev_cols) {
    if (!paf || !up_out || !dev_cols) return AASM_E_INVAL;
    RowsHostCols h;
    if (!rows_host_cols(*paf, c0, c1, h)) { set_last_error("aasm_paf_upload_rows: [c0, c1) is no range of the container's contigs"); return AASM_E_INVAL; }
    int rc = ctx_init(device);
    if (rc != AASM_OK) return rc;
    hipSetDevice(device);
    aasm_upload *up = new aasm_upload();
    up->device = device;
    std::memset(&up->view, 0, sizeof up->view);
    hipError_t e = hipSuccess;
    auto put = [&](const void *src, size_t bytes) -> void * {
        void *p = nullptr;
        if (e != hipSuccess) return nullptr;
        if ((e = hipMalloc(&p, bytes ? bytes : 8)) != hipSuccess) return nullptr;
        up->ptrs.push_back(p);
        if (bytes) e = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
        return p;
    };
    aasm_row_cols v;
    const size_t R = h.ref_total.size();
    v.n_chr = (int64_t)h.chr_name_off.size() - 1;
    v.ref_total = (const int64_t *)put(h.ref_total.data(), R * 8);
    v.mat_num = (const int32_t *)put(h.mat_num.data(), R * 4); v.aln_len = (const int32_t *)put(h.aln_len.data(), R * 4);
    v.row_index = (const int32_t *)put(h.row_index.data(), R * 4); v.cord_type = (const uint8_t *)put(h.cord_type.data(), R);
    v.names = (const char *)put(h.names.data(), h.names.size());
    v.ctg_name_off = (const int64_t *)put(h.ctg_name_off.data(), h.ctg_name_off.size() * 8);
    v.chr_name_off = (const int64_t *)put(h.chr_name_off.data(), h.chr_name_off.size() * 8);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        for (void *p : up->ptrs) hipFree(p);
        delete up;
        set_last_error(hip_err("aasm_paf_upload_rows", e));
        return e == hipErrorOutOfMemory ? AASM_E_NOMEM : AASM_E_HIP;
    }
    *dev_cols = v;
    *up_out = up;
    return AASM_OK;
}

namespace {
struct RowsGpu {
    hipStream_t stream;
    hipError_t err = hipSuccess;
    void launch_rows(int kw, int64_t nblocks, int nthreads, const RowsArgs &a) {
        if (err != hipSuccess) return;
        launch_row(rows_syms, kw, nblocks, nthreads, stream, a);
        err = hipGetLastError();
    }
};
// what the sizes calls on a device returned, by their row_off arrays: aasm_rows_format_device cannot read the device.  Under a lock
// of its own, so that the format call never waits for a solve that holds the context's.
struct RowsSized { const int64_t *off[3]; int64_t n[3], bytes[3], n_flagged; };
std::vector<RowsSized> g_rows_sized[16];
std::mutex g_rows_mu;
int64_t *g_rows_words[16];                                           // RowsArgs::words of a device, made once
}  // namespace

// the checked arguments of a rows entry, or AASM_E_INVAL and its message
static int rows_entry_args(const aasm_batch_in *dev_in, const aasm_row_cols *cols, const aasm_out_sizes *sz, const aasm_dev_out *dev_out,
                           const aasm_dev_cuts *cuts, const aasm_dev_rows *ro, int device, RowsArgs &a) {
    if (!dev_in || !cols || !sz || !dev_out || !cuts || !ro) return AASM_E_INVAL;
    if (!dev_in->cs_text || !dev_in->rec_cs_off) { set_last_error("the device batch carries no cs text (it was uploaded with match ranges)"); return AASM_E_INVAL; }
    if (!rows_args(*dev_in, *cols, *sz, *dev_out, *cuts, *ro, a)) { set_last_error("sizes do not fit the batch"); return AASM_E_INVAL; }
    const int rc = ctx_init(device);
    if (rc != AASM_OK) return rc;
    hipSetDevice(device);
    const int64_t C = a.c.C, R = a.c.R;
    if (!cut_arrays_ok(*dev_in, *dev_out, *cuts, a.c, device) || !dev_buffer_ok(dev_in->qry_total, R, 8, device) || !dev_buffer_ok(dev_in->ref_chr, R, 4, device) ||
        !dev_buffer_ok(dev_in->map_qul, R, 1, device) || !dev_buffer_ok(cols->ref_total, R, 8, device) || !dev_buffer_ok(cols->mat_num, R, 4, device) ||
        !dev_buffer_ok(cols->aln_len, R, 4, device) || !dev_buffer_ok(cols->row_index, R, 4, device) || !dev_buffer_ok(cols->cord_type, R, 1, device) ||
        !dev_buffer_ok(cols->names, 1, 1, device) || !dev_buffer_ok(cols->ctg_name_off, C + 1, 8, device) || !dev_buffer_ok(cols->chr_name_off, cols->n_chr + 1, 8, device) ||
        !dev_buffer_ok(ro->main_off, a.c.n[0] + 1, 8, device) || !dev_buffer_ok(ro->alt_off, a.c.n[1] + 1, 8, device) || !dev_buffer_ok(ro->all_off, a.c.n[2] + 1, 8, device)) {
        set_last_error("an array is NULL, not device memory of the device, or misaligned");
        return AASM_E_INVAL;
    }
    return AASM_OK;
}

// under cx.mu: the length pass, the three scans (the context's single-pass scan, in place) and one read-back, on stream s
static int rows_sizes_locked(DevCtx &cx, RowsArgs &a, int flags, int device, hipStream_t s, aasm_rows_info *info) {
    (void)hipStreamSynchronize(cx.stream);                           // (the scans' scratch words are the context's: nothing of a solve may still use them)
    if (!g_rows_words[device]) {
        const hipError_t e = hipMalloc((void **)&g_rows_words[device], RW_WORDS * 8);
        if (e != hipSuccess) { (void)hipGetLastError(); g_rows_words[device] = nullptr; set_last_error(hip_err("hipMalloc(rows)", e)); return e == hipErrorOutOfMemory ? AASM_E_NOMEM : AASM_E_HIP; }
    }
    a.words = g_rows_words[device];
    const int64_t init[RW_WORDS] = {0, AASM_ROWS_NO_KEY};
    hipError_t e = hipMemcpyAsync(a.words, init, sizeof init, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);                // (init is this frame's)
    if (e != hipSuccess) { set_last_error(hip_err("aasm_rows_sizes_device", e)); return AASM_E_HIP; }
    RowsGpu be{s};
    rows_launch_len(be, a, flags);
    if (be.err != hipSuccess) { set_last_error(hip_err("kernel launch", be.err)); return AASM_E_HIP; }
    GpuBackend sc(cx, s, GpuBackend::Attach{});
    for (int l = 0; l < 3; l++) sc.scan_t<int64_t>(a.row_off[l] + 1, a.c.n[l], a.row_off[l]);
    int64_t got[5];
    sc.read_i64s({a.words + RW_FLAGGED, a.words + RW_FIRST, a.row_off[0] + a.c.n[0], a.row_off[1] + a.c.n[1], a.row_off[2] + a.c.n[2]}, got);
    if (sc.failed()) {
        // a scan that did not run to its end leaves its words behind (solve_on_device does the same)
        (void)hipDeviceSynchronize();
        if (cx.d_scratch) (void)hipMemset(cx.d_scratch, 0, cx.d_scratch_cap * 8);
        cx.pinned[SCAN_STALL_SLOT] = 0;
        (void)hipGetLastError();
        return AASM_E_HIP;
    }
    rows_info_of(got, *info);
    for (int l = 0; l < 3; l++) info->bytes[l] = got[2 + l];
    std::lock_guard<std::mutex> rlk(g_rows_mu);
    std::vector<RowsSized> &reg = g_rows_sized[device];
    reg.erase(std::remove_if(reg.begin(), reg.end(), [&](const RowsSized &x) { return x.off[0] == a.row_off[0] && x.off[1] == a.row_off[1] && x.off[2] == a.row_off[2]; }), reg.end());
    if (reg.size() >= 64) reg.erase(reg.begin());
    RowsSized x;
    for (int l = 0; l < 3; l++) { x.off[l] = a.row_off[l]; x.n[l] = a.c.n[l]; x.bytes[l] = info->bytes[l]; }
    x.n_flagged = info->n_flagged;
    reg.push_back(x);
    return AASM_OK;
}

int aasm_rows_sizes_device(const aasm_batch_in *dev_in, const aasm_row_cols *dev_cols, const aasm_out_sizes *sz, const aasm_dev_out *dev_out,
                           const aasm_dev_cuts *cuts, const aasm_dev_rows *row_off, int flags, int device, void *stream, aasm_rows_info *info) {
    if (!info) return AASM_E_INVAL;
    RowsArgs a;
    const int rc = rows_entry_args(dev_in, dev_cols, sz, dev_out, cuts, row_off, device, a);
    if (rc != AASM_OK) return rc;
    DevCtx &cx = g_ctx[device];
    std::lock_guard<std::mutex> lk(cx.mu);
    return rows_sizes_locked(cx, a, flags, device, (hipStream_t)stream, info);
}

// info against what the sizes call on these row_off arrays returned
static bool rows_info_known(int device, const RowsArgs &a, const aasm_rows_info &info) {
    std::lock_guard<std::mutex> rlk(g_rows_mu);
    for (const RowsSized &x : g_rows_sized[device])
        if (x.off[0] == a.row_off[0] && x.off[1] == a.row_off[1] && x.off[2] == a.row_off[2])
            return x.n[0] == a.c.n[0] && x.n[1] == a.c.n[1] && x.n[2] == a.c.n[2] && x.bytes[0] == info.bytes[0] && x.bytes[1] == info.bytes[1] &&
                   x.bytes[2] == info.bytes[2] && x.n_flagged == info.n_flagged;
    return false;
}

int aasm_rows_format_device(const aasm_batch_in *dev_in, const aasm_row_cols *dev_cols, const aasm_out_sizes *sz, const aasm_dev_out *dev_out,
                            const aasm_dev_cuts *cuts, const aasm_dev_rows *row_off, const aasm_rows_info *info, int list, int64_t e0, int64_t e1,
                            char *text, int flags, int device, void *stream) {
    if (!info) return AASM_E_INVAL;
    RowsArgs a;
    const int rc = rows_entry_args(dev_in, dev_cols, sz, dev_out, cuts, row_off, device, a);
    if (rc != AASM_OK) return rc;
    if (const char *why = rows_format_refusal(a, *info, list, e0, e1)) { set_last_error(std::string("aasm_rows_format_device: ") + why); return AASM_E_INVAL; }
    if (!rows_info_known(device, a, *info)) { set_last_error("aasm_rows_format_device: info is not what aasm_rows_sizes_device returned for these row_off arrays"); return AASM_E_INVAL; }
    if (e1 > e0 && !dev_buffer_ok(text, 1, 1, device)) { set_last_error("aasm_rows_format_device: text is NULL or not device memory of the device"); return AASM_E_INVAL; }
    RowsGpu be{(hipStream_t)stream};
    rows_launch_fill(be, a, list, e0, e1, text, flags);
    if (be.err != hipSuccess) { set_last_error(hip_err("kernel launch", be.err)); return AASM_E_HIP; }
    return AASM_OK;
}

// ---- aasm_writer_append_device: the three lists' rows formatted piece by piece, piece k + 1 while piece k comes back and is written ----
namespace {
// rows_cut_pieces' fetch (aasm_rows.h) over a device array: the sampled offsets by one strided copy, a block's own by a plain one
struct RowsOffFetch {
    const int64_t *d_off;
    bool operator()(int64_t first, int64_t stride, int64_t count, int64_t *dst) const {
        if (stride == 1) return hipMemcpy(dst, d_off + first, (size_t)count * 8, hipMemcpyDeviceToHost) == hipSuccess;
        return hipMemcpy2D(dst, 8, d_off + first, (size_t)stride * 8, 8, (size_t)count, hipMemcpyDeviceToHost) == hipSuccess;
    }
};
}  // namespace

int aasm_writer_append_device(aasm_writer *w, const aasm_paf *paf, const aasm_batch_in *dev_in, const aasm_row_cols *dev_cols, const aasm_out_sizes *sz,
                              const aasm_dev_out *dev_out, const aasm_dev_cuts *cuts, int64_t contig0, int64_t piece_bytes, int device) {
    if (!w || !sz || piece_bytes < 0 || (!paf && !dev_in)) return AASM_E_INVAL;
    int rc = writer_device_begin(w, paf, contig0, sz->n_contigs, paf ? paf->has_cs : dev_in->cs_text != nullptr);
    if (rc != AASM_OK) return rc;
    RowsArgs a;
    aasm_dev_rows ro = {nullptr, nullptr, nullptr};
    std::vector<void *> dev_mem;
    char *pinned_own[2] = {nullptr, nullptr};
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool oom = false;
    auto dalloc = [&](size_t bytes) -> void * {
        void *p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes ? bytes : 8);
        if (e != hipSuccess) { (void)hipGetLastError(); oom = true; return nullptr; }
        dev_mem.push_back(p);
        return p;
    };
    auto cleanup = [&]() {
        for (void *p : dev_mem) hipFree(p);
        for (char *p : pinned_own) if (p) hipHostFree(p);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    };
    if ((rc = ctx_init(device)) != AASM_OK) return rc;
    hipSetDevice(device);
    ro.main_off = (int64_t *)dalloc((size_t)(sz->n_main + 1) * 8); ro.alt_off = (int64_t *)dalloc((size_t)(sz->n_alt + 1) * 8); ro.all_off = (int64_t *)dalloc((size_t)(sz->n_all_elems + 1) * 8);
    if (oom) { cleanup(); set_last_error("out of device memory (device writer)"); return AASM_E_NOMEM; }   // (nothing written: the session stays as it was)
    if ((rc = rows_entry_args(dev_in, dev_cols, sz, dev_out, cuts, &ro, device, a)) != AASM_OK) { cleanup(); return rc; }
    DevCtx &cx = g_ctx[device];
    std::lock_guard<std::mutex> lk(cx.mu);
    aasm_rows_info info;
    if ((rc = rows_sizes_locked(cx, a, 0, device, cx.stream, &info)) != AASM_OK) { cleanup(); if (rc == AASM_E_NOMEM) return rc; writer_device_end(w, sz->n_contigs, rc); return rc; }
    const int64_t C = a.c.C;
    if (info.n_flagged != 0 && !paf) {
        // no container, no host codec to ask: the count and the first element's list, index and flags
        static const char *const lists[3] = {"main", "alt", "all"};
        char msg[160];
        std::snprintf(msg, sizeof msg, "%lld output elements cannot be formatted; the first: list %s, element %lld, flags 0x%x", (long long)info.n_flagged,
                      lists[info.bad_list >= 0 && info.bad_list < 3 ? info.bad_list : 0], (long long)info.bad_elem, (unsigned)info.bad_flags);
        cleanup();
        rc = (info.bad_flags & (AASM_ROWS_CUT_ERRORS & ~AASM_CUT_E_RECORD)) ? AASM_E_PARSE : AASM_E_INVAL;
        set_last_error(msg);
        writer_device_end(w, sz->n_contigs, rc);
        return rc;
    }
    if (info.n_flagged != 0) {
        // the first element that cannot be formatted, through the planned writer's own check: its code and message are the contract
        const int l = info.bad_list;
        const int64_t i = info.bad_elem;
        aasm_out_elem el;
        aasm_cut_plan plan;
        std::vector<int64_t> off((size_t)C + 1), eoff;
        hipError_t e = hipMemcpy(&el, a.c.el[l] + i, sizeof el, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(&plan, a.c.dst[l] + i, sizeof plan, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(off.data(), l == 2 ? a.c.path_off : a.c.off[l], (size_t)(C + 1) * 8, hipMemcpyDeviceToHost);
        int64_t owner = i;
        if (e == hipSuccess && l == 2) {
            eoff.resize((size_t)a.c.NP + 1);
            e = hipMemcpy(eoff.data(), a.c.off[2], eoff.size() * 8, hipMemcpyDeviceToHost);
            owner = (std::upper_bound(eoff.begin(), eoff.end(), i) - eoff.begin()) - 1;   // the element's path
        }
        cleanup();
        if (e != hipSuccess) { set_last_error(hip_err("device writer", e)); rc = AASM_E_HIP; }
        else {
            const int64_t c = (std::upper_bound(off.begin(), off.end(), owner) - off.begin()) - 1;
            std::string name = paf->ctg_name[(size_t)(contig0 + c)], err;
            if (l == 2) name += "." + std::to_string((long long)(owner - off[(size_t)c] + 1));
            rc = writer_row_verdict(paf, contig0 + c, name, el, plan, err);
            if (rc == AASM_OK) { rc = AASM_E_INTERNAL; err = "the device refused a row the host writer formats"; }
            set_last_error(err);
        }
        writer_device_end(w, sz->n_contigs, rc);
        return rc;
    }
    // ---- pieces
    const int64_t limit = piece_bytes > 0 ? piece_bytes : (int64_t)AASM_STAGE_BYTES;
    std::vector<RowsPiece> pieces;
    bool ok = true;
    for (int l = 0; l < 3 && ok; l++)
        if (writer_device_has(w, l)) ok = rows_cut_pieces(RowsOffFetch{a.row_off[l]}, a.c.n[l], info.bytes[l], l, limit, pieces);
    if (!ok) { (void)hipGetLastError(); cleanup(); set_last_error("device writer: reading the row offsets failed"); writer_device_end(w, sz->n_contigs, AASM_E_HIP); return AASM_E_HIP; }
    int64_t largest = 0;
    for (const RowsPiece &p : pieces) largest = std::max(largest, p.b1 - p.b0);
    char *dbuf[2] = {nullptr, nullptr}, *hbuf[2] = {nullptr, nullptr};
    if (!pieces.empty()) {
        for (int b = 0; b < 2; b++) dbuf[b] = (char *)dalloc((size_t)largest);
        for (int b = 0; b < 2 && !oom; b++) {
            if (largest <= (int64_t)AASM_STAGE_BYTES) {              // the context's staging chunks (made on first use, kept)
                if (!cx.stage[b] && hipHostMalloc((void **)&cx.stage[b], AASM_STAGE_BYTES) != hipSuccess) { (void)hipGetLastError(); cx.stage[b] = nullptr; oom = true; }
                hbuf[b] = cx.stage[b];
            } else {
                if (hipHostMalloc((void **)&pinned_own[b], (size_t)largest) != hipSuccess) { (void)hipGetLastError(); pinned_own[b] = nullptr; oom = true; }
                hbuf[b] = pinned_own[b];
            }
        }
        for (int b = 0; b < 4 && !oom; b++) if (hipEventCreateWithFlags(&ev[b], hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); ev[b] = nullptr; oom = true; }
        if (oom) { cleanup(); set_last_error("out of memory (device writer)"); return AASM_E_NOMEM; }   // (nothing written yet)
    }
    hipError_t e = hipSuccess;
    auto enqueue = [&](size_t k) {                                   // piece k: formatted on the context's stream, copied back on its side stream
        const RowsPiece &p = pieces[k];
        const int b = (int)(k & 1);
        RowsGpu be{cx.stream};
        rows_launch_fill(be, a, p.list, p.e0, p.e1, dbuf[b], 0);
        e = be.err;
        if (e == hipSuccess) e = hipEventRecord(ev[b], cx.stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(cx.side, ev[b], 0);
        if (e == hipSuccess) e = hipMemcpyAsync(hbuf[b], dbuf[b], (size_t)(p.b1 - p.b0), hipMemcpyDeviceToHost, cx.side);
        if (e == hipSuccess) e = hipEventRecord(ev[2 + b], cx.side);
    };
    rc = AASM_OK;
    if (!pieces.empty()) enqueue(0);
    for (size_t k = 0; k < pieces.size() && e == hipSuccess && rc == AASM_OK; k++) {
        if (k + 1 < pieces.size()) enqueue(k + 1);                   // (its buffers are those of piece k - 1, which is on disk)
        if (e == hipSuccess) e = hipEventSynchronize(ev[2 + (k & 1)]);
        if (e == hipSuccess) rc = writer_device_put(w, pieces[k].list, hbuf[k & 1], pieces[k].b1 - pieces[k].b0);
    }
    (void)hipStreamSynchronize(cx.stream);
    (void)hipStreamSynchronize(cx.side);
    if (e != hipSuccess) { (void)hipGetLastError(); set_last_error(hip_err("device writer", e)); rc = AASM_E_HIP; }
    cleanup();
    writer_device_end(w, sz->n_contigs, rc);
    return rc;
}

// concatenate per-range results (contiguous contig ranges cut[d]..cut[d+1]) in contig order
static void concat_parts(std::vector<aasm_batch_out> &parts, const std::vector<int64_t> &cut, int64_t C, aasm_batch_out *out) {
    const int n_devices = (int)parts.size();
    std::memset(out, 0, sizeof(*out));
    out->n_contigs = C;
    int64_t nm = 0, na = 0, np = 0, ne = 0;
    for (auto &p : parts) { nm += p.main_off[p.n_contigs]; na += p.alt_off[p.n_contigs]; np += p.n_all_paths; ne += p.all_elem_off[p.n_all_paths]; }
    out->main_off = (int64_t *)calloc(C + 1, 8); out->alt_off = (int64_t *)calloc(C + 1, 8); out->all_path_off = (int64_t *)calloc(C + 1, 8);
    out->all_elem_off = (int64_t *)calloc(np + 1, 8); out->ctg_status = (int32_t *)calloc(C + 1, 4);
    out->main_elems = (aasm_out_elem *)calloc(nm + 1, sizeof(aasm_out_elem));
    out->alt_elems = (aasm_out_elem *)calloc(na + 1, sizeof(aasm_out_elem));
    out->all_elems = (aasm_out_elem *)calloc(ne + 1, sizeof(aasm_out_elem));
    out->n_all_paths = np;
    int64_t bm = 0, ba = 0, bp = 0, be_ = 0;
    for (int d = 0; d < n_devices; d++) {
        aasm_batch_out &p = parts[d];
        const int64_t pc = p.n_contigs, c0 = cut[d];
        for (int64_t c = 0; c < pc; c++) {
            out->main_off[c0 + c + 1] = bm + p.main_off[c + 1];
            out->alt_off[c0 + c + 1] = ba + p.alt_off[c + 1];
            out->all_path_off[c0 + c + 1] = bp + p.all_path_off[c + 1];
            out->ctg_status[c0 + c] = p.ctg_status[c];
        }
        for (int64_t q = 0; q < p.n_all_paths; q++) out->all_elem_off[bp + q + 1] = be_ + p.all_elem_off[q + 1];
        std::memcpy(out->main_elems + bm, p.main_elems, sizeof(aasm_out_elem) * (size_t)p.main_off[pc]);
        std::memcpy(out->alt_elems + ba, p.alt_elems, sizeof(aasm_out_elem) * (size_t)p.alt_off[pc]);
        std::memcpy(out->all_elems + be_, p.all_elems, sizeof(aasm_out_elem) * (size_t)p.all_elem_off[p.n_all_paths]);
        bm += p.main_off[pc]; ba += p.alt_off[pc]; bp += p.n_all_paths; be_ += p.all_elem_off[p.n_all_paths];
        aasm_stats &a = out->stats; const aasm_stats &b = p.stats;
        a.n_vertices += b.n_vertices; a.n_pairs += b.n_pairs; a.n_edges += b.n_edges; a.n_heap_nodes += b.n_heap_nodes;
        a.n_paths_found += b.n_paths_found; a.n_paths_converted += b.n_paths_converted; a.n_unconnectable += b.n_unconnectable;
        a.n_internal_errors += b.n_internal_errors; a.n_single += b.n_single; a.range_steps += b.range_steps;
        a.ispr_edges += b.ispr_edges; a.ispr_vertices += b.ispr_vertices; a.path_edges += b.path_edges; a.out_elems += b.out_elems; a.pq_pushes += b.pq_pushes;
        if (b.device_bytes > a.device_bytes) a.device_bytes = b.device_bytes;
        for (int i = 0; i < AASM_N_PHASES; i++) if (b.phase_ms[i] > a.phase_ms[i]) a.phase_ms[i] = b.phase_ms[i];
        if (b.total_ms > a.total_ms) a.total_ms = b.total_ms;
        for (int i = 0; i < 3; i++) if (b.reserved_f[i] > a.reserved_f[i]) a.reserved_f[i] = b.reserved_f[i];
        aasm_free_out(&p);
    }
}

static int validate_batch(const aasm_batch_in *in) {
    if (!in || in->n_contigs <= 0 || !in->ctg_rec_off || in->ctg_rec_off[0] != 0 || in->ctg_rec_off[in->n_contigs] != in->n_records) {
        set_last_error("inconsistent contig offsets");
        return AASM_E_INVAL;
    }
    for (int64_t c = 0; c < in->n_contigs; c++)
        if (in->ctg_rec_off[c + 1] <= in->ctg_rec_off[c]) { set_last_error("empty contig"); return AASM_E_INVAL; }
    if (!in->rec_rng_off || (!in->rng_qry_l && !(in->cs_text && in->rec_cs_off))) {
        set_last_error("the batch carries neither match ranges (rng_*) nor cs tags (cs_text / rec_cs_off)");
        return AASM_E_INVAL;
    }
    // ranges the device's narrowed fields are exact for (aasm_kernels.h AASM_COORD_LIMIT; the device repeats the
    // coordinate check per contig for batches that are handed over already resident)
    for (int64_t c = 0; c < in->n_contigs; c++)
        if (in->ctg_rec_off[c + 1] - in->ctg_rec_off[c] > (int64_t)INT32_MAX - 64) {
            set_last_error("contig " + std::to_string(c) + " has more than 2^31 records");
            return AASM_E_OVERFLOW;
        }
    for (int64_t r = 0; r < in->n_records; r++)
        if (!(host_coord_ok(in->qry_str[r]) && host_coord_ok(in->qry_end[r]) && host_coord_ok(in->ref_str[r]) && host_coord_ok(in->ref_end[r]) && host_coord_ok(in->qry_total[r]))) {
            set_last_error("record " + std::to_string(r) + ": coordinate outside [0, 2^40) (qry_str / qry_end / ref_str / ref_end / qry_total)");
            return AASM_E_OVERFLOW;
        }
    return AASM_OK;
}



// Make the device context and `bytes` of workspace arena ahead of the first solve (a fresh process pays the HIP start-up
// and ~25 ms per GB of hipMalloc otherwise inside its first solve): callers run it on a thread of its own while they still
// read their input.  Not finding the memory is not an error here - the solve allocates what it needs (and reports).
int aasm_reserve_workspace(int device, int64_t bytes) {
    int rc = ctx_init(device);
    if (rc != AASM_OK) return rc;
    DevCtx &cx = g_ctx[device];
    std::lock_guard<std::mutex> lk(cx.mu);
    // the input is on its way (or a solve has run): the free-memory figure below no longer leaves room for it, and a solve
    // that holds the lock first would make this call allocate memory nobody uses after it - the solve allocates for itself
    if (cx.input_arrived.load() != 0) return AASM_OK;
    hipSetDevice(device);
    size_t have = 0;
    for (auto &b : cx.blocks) have += b.cap;
    if (bytes <= 0 || have >= (size_t)bytes) return AASM_OK;
    size_t want = (size_t)bytes - have, free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && want > free_b / 2) want = free_b / 2;   // leave room for the input and the results
    want &= ~(size_t)255;
    if (want < ((size_t)64 << 20)) return AASM_OK;
    char *p = nullptr;
    hipError_t e = hipMalloc((void **)&p, want);
    g_n_device_mallocs++;
    if (e != hipSuccess) { (void)hipGetLastError(); return AASM_E_NOMEM; }
    cx.blocks.push_back(ArenaBlock{p, want, 0});
    return AASM_OK;
}

static void ctx_release_arena(int device) {
    DevCtx &cx = g_ctx[device];
    std::lock_guard<std::mutex> lk(cx.mu);
    hipSetDevice(device);
    hipStreamSynchronize(cx.stream);
    drain_exports(cx);
    for (auto &b : cx.blocks) hipFree(b.p);
    cx.blocks.clear();
    cx.generation++;
}

static int solve_range_once(const aasm_batch_in *in, int64_t c0, int64_t c1, const aasm_opts &o, aasm_batch_out *out) {
    const int64_t limit = decode_hooks(o).range_limit;
    if (limit > 0 && c1 - c0 > limit) {                               // test hook: pretend larger ranges do not fit
        set_last_error("range exceeds the test hook's range limit");
        return AASM_E_NOMEM;
    }
    aasm_upload *up = nullptr;
    aasm_batch_in dv;
    auto t0 = std::chrono::steady_clock::now();
    int rc = upload_range(in, c0, c1, o.device, &up, &dv);
    if (rc != AASM_OK) return rc;
    auto t1 = std::chrono::steady_clock::now();
    aasm_result *res = nullptr;
    rc = aasm_solve_device(&dv, &o, nullptr, &res);
    if (rc == AASM_OK) {
        auto t2 = std::chrono::steady_clock::now();
        rc = aasm_result_fetch(res, out);
        auto t3 = std::chrono::steady_clock::now();
        if (rc == AASM_OK) {
            out->stats.reserved_f[0] = std::chrono::duration<float, std::milli>(t1 - t0).count();   // H2D upload
            out->stats.reserved_f[1] = std::chrono::duration<float, std::milli>(t3 - t2).count();   // D2H + pack
            out->stats.reserved_f[2] = std::chrono::duration<float, std::milli>(t2 - t1).count();   // solve wall
        }
    }
    if (rc == AASM_E_PARSE && g_bad_record >= 0 && in->cs_text && in->rec_cs_off) {   // say what the host codec says about that tag
        const int64_t r = in->ctg_rec_off[c0] + g_bad_record;
        const std::string why = cs_error_message(in->cs_text + in->rec_cs_off[r], in->rec_cs_off[r + 1] - in->rec_cs_off[r], in->aln_fwd[r] != 0,
                                                 in->qry_str[r], in->qry_end[r], in->ref_str[r], in->ref_end[r]);
        set_last_error((why.empty() ? std::string("malformed cs:Z tag") : why) + " (record " + std::to_string(r) + ")");
    }
    aasm_result_free(res);
    aasm_upload_free(up);
    return rc;
}

static void add_stats(aasm_stats &a, const aasm_stats &b, bool sum_time) {
    a.n_vertices += b.n_vertices; a.n_pairs += b.n_pairs; a.n_edges += b.n_edges; a.n_heap_nodes += b.n_heap_nodes;
    a.n_paths_found += b.n_paths_found; a.n_paths_converted += b.n_paths_converted; a.n_unconnectable += b.n_unconnectable;
    a.n_internal_errors += b.n_internal_errors; a.n_single += b.n_single; a.range_steps += b.range_steps;
    a.ispr_edges += b.ispr_edges; a.ispr_vertices += b.ispr_vertices; a.path_edges += b.path_edges; a.out_elems += b.out_elems; a.pq_pushes += b.pq_pushes;
    if (b.device_bytes > a.device_bytes) a.device_bytes = b.device_bytes;
    for (int i = 0; i < AASM_N_PHASES; i++) a.phase_ms[i] = sum_time ? a.phase_ms[i] + b.phase_ms[i] : (b.phase_ms[i] > a.phase_ms[i] ? b.phase_ms[i] : a.phase_ms[i]);
    a.total_ms = sum_time ? a.total_ms + b.total_ms : (b.total_ms > a.total_ms ? b.total_ms : a.total_ms);
    for (int i = 0; i < 3; i++) a.reserved_f[i] = sum_time ? a.reserved_f[i] + b.reserved_f[i] : (b.reserved_f[i] > a.reserved_f[i] ? b.reserved_f[i] : a.reserved_f[i]);
}

// A contig range that does not fit in device memory is split in halves (contigs are
// independent) after the arena of the failed attempt has been given back.
static int solve_range(const aasm_batch_in *in, int64_t c0, int64_t c1, const aasm_opts &o, aasm_batch_out *out) {
    int rc = solve_range_once(in, c0, c1, o, out);
    if (rc != AASM_E_NOMEM || c1 - c0 < 2) return rc;                    // only a true allocation failure is worth splitting for
    g_n_range_splits++;
    ctx_release_arena(o.device);
    const int64_t mid = c0 + (c1 - c0) / 2;
    std::vector<aasm_batch_out> parts(2);
    std::memset(&parts[0], 0, sizeof(aasm_batch_out)); std::memset(&parts[1], 0, sizeof(aasm_batch_out));
    rc = solve_range(in, c0, mid, o, &parts[0]);
    if (rc == AASM_OK) rc = solve_range(in, mid, c1, o, &parts[1]);
    if (rc != AASM_OK) { aasm_free_out(&parts[0]); aasm_free_out(&parts[1]); return rc; }
    std::vector<int64_t> cut{0, mid - c0, c1 - c0};
    aasm_stats st;
    std::memset(&st, 0, sizeof(st));
    add_stats(st, parts[0].stats, true); add_stats(st, parts[1].stats, true);
    concat_parts(parts, cut, c1 - c0, out);
    out->stats = st;
    return AASM_OK;
}

// contigs [c0, c1) of the batch: what a caller that streams a file runs per chunk (out covers c1 - c0 contigs)
int aasm_solve_batch_range(const aasm_batch_in *in, int64_t c0, int64_t c1, const aasm_opts *opts, aasm_batch_out *out) {
    if (!in || !out || c0 < 0 || c1 > in->n_contigs || c0 >= c1) return AASM_E_INVAL;
    aasm_opts o;
    std::memset(&o, 0, sizeof(o));
    if (opts) o = *opts;
    if (c0 == 0) { const int rc = validate_batch(in); if (rc != AASM_OK) return rc; }    // (the whole batch is checked once, with its first range)
    return solve_range(in, c0, c1, o, out);
}

int aasm_solve_batch(const aasm_batch_in *in, const aasm_opts *opts, aasm_batch_out *out) {
    if (!in || !out) return AASM_E_INVAL;
    aasm_opts o;
    std::memset(&o, 0, sizeof(o));
    if (opts) o = *opts;
    int rc = validate_batch(in);
    if (rc != AASM_OK) return rc;
    return solve_range(in, 0, in->n_contigs, o, out);
}

// Contig-sharded solve over n_devices GPUs of one node (devices opts.device .. +n-1):
// static contiguous partition balanced on a per-contig cost estimate (aasm_shard.cpp), one host thread and
// one stream per device, results concatenated in contig order.  No collective anywhere:
// contigs are independent (reference: one TBB task per contig, src/alignasm.cpp:351-359).
int aasm_solve_batch_multi(const aasm_batch_in *in, const aasm_opts *opts, int n_devices, aasm_batch_out *out) {
    if (!in || !out || n_devices < 1) return AASM_E_INVAL;
    aasm_opts o;
    std::memset(&o, 0, sizeof(o));
    if (opts) o = *opts;
    int rc = validate_batch(in);
    if (rc != AASM_OK) return rc;
    const int64_t C = in->n_contigs;
    if (n_devices > C) n_devices = (int)C;
    if (n_devices == 1) return solve_range(in, 0, C, o, out);
    // contiguous blocks balanced on the density-aware per-contig cost (aasm_shard.cpp)
    std::vector<double> cost((size_t)C);
    contig_costs(in, cost.data());
    std::vector<int64_t> cut(n_devices + 1, 0);
    partition_by_cost(cost.data(), C, n_devices, cut.data());
    // test hook (AASM_H2_WRAP_DEVICES, or AASM_TEST_WRAP_DEVICES=1 for the CLI): device ordinals wrap around the devices
    // that exist, so that the one-thread-per-shard path runs on a box with fewer GPUs than shards (the shards of one
    // device take turns on its context)
    const char *wrap_env = getenv("AASM_TEST_WRAP_DEVICES");
    const bool wrap = decode_hooks(o).wrap_devices || (wrap_env && wrap_env[0] == '1');
    const int ndev = std::max(1, aasm_device_count());
    std::vector<aasm_batch_out> parts(n_devices);
    std::vector<int> rcs(n_devices, AASM_OK);
    std::vector<std::string> errs(n_devices);
    {
        std::vector<std::thread> th;
        for (int d = 0; d < n_devices; d++)
            th.emplace_back([&, d] {
                aasm_opts od = o;
                od.device = wrap ? (o.device + d) % ndev : o.device + d;
                std::memset(&parts[d], 0, sizeof(parts[d]));
                static std::mutex turn[16];                              // (a context holds ONE result: a wrapped shard solves and fetches before the next one starts)
                std::unique_lock<std::mutex> lk(turn[od.device & 15], std::defer_lock);
                if (wrap) lk.lock();
                rcs[d] = solve_range(in, cut[d], cut[d + 1], od, &parts[d]);
                if (rcs[d] != AASM_OK) errs[d] = aasm_last_error();
            });
        for (auto &t : th) t.join();
    }
    for (int d = 0; d < n_devices; d++)
        if (rcs[d] != AASM_OK) {
            set_last_error("device " + std::to_string(o.device + d) + ": " + errs[d]);
            for (auto &p : parts) aasm_free_out(&p);
            return rcs[d];
        }
    concat_parts(parts, cut, C, out);
    return AASM_OK;
}

}  // extern "C"
