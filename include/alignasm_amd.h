/*
 * alignasm_amd.h -- C-ABI of the MI355X-native per-contig path-inference solver.
 *
 * Drop-in boundary for ONE hot path of ACCtools/alignasm: the per-contig solver
 *
 *     void solve_ctg_read(std::vector<PafReadData>& in,
 *                         std::vector<PafOutputData>& out,
 *                         std::vector<PafOutputData>& alt_out,
 *                         std::vector<std::vector<PafOutputData>>& max_out)
 *
 * (reference: src/paf_data.hpp:193 declaration, src/paf_data.cpp:223 definition,
 *  call sites src/alignasm.cpp:357,373,391).  The reference has no FFI layer; this
 * header is the FFI a maintainer would bind (INTEGRATION.md shows the glue).
 * The GPU wants many contigs per launch, so the unit is a BATCH of contigs in flat
 * SoA arrays with per-contig offsets instead of one std::vector per call.
 *
 * Conventions (all taken from the reference):
 *  - every interval is CLOSED [str, end], 0-based        (src/alignasm.cpp:141-151)
 *  - for '-' strand records ref_str > ref_end: ref_str is the reference position of
 *    qry_str                                              (src/alignasm.cpp:155-159)
 *  - records of one contig are given in INPUT order; position inside the contig is
 *    the reference's PafReadData::ctg_index               (src/alignasm.cpp:138)
 *  - match ranges are what get_overlap_range() produces   (src/paf_data.cpp:90-123):
 *    one (qry_l, qry_r, ref_l) triple per ':' op of the cs tag, query-oriented;
 *    the reference-side right end is ref_l + (qry_r-qry_l)*step and is not passed.
 *
 * No exceptions cross this ABI; every entry point returns 0 or a negative AASM_E_*.
 * All arithmetic on the path is int64 / int32 integer work (no floating point).
 */
#ifndef ALIGNASM_AMD_H
#define ALIGNASM_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AASM_ABI_VERSION 3

/* error codes */
#define AASM_OK              0
#define AASM_E_INVAL        -1   /* bad argument / inconsistent offsets            */
#define AASM_E_NODEVICE     -2   /* no HIP device / HIP runtime error at init      */
#define AASM_E_HIP          -3   /* HIP runtime error during a solve               */
#define AASM_E_NOMEM        -4   /* device or host allocation failed               */
#define AASM_E_OVERFLOW     -5   /* input outside the supported range (coordinates >= 2^40, a contig of >= 2^31
                                    records / vertices / heap nodes) or an internal pool overflow        */
#define AASM_E_INTERNAL     -6   /* "must not happen" state of the reference hit   */
#define AASM_E_PARSE        -7   /* PAF / cs tag parse error (host codec)          */
#define AASM_E_IO           -8

/* ---- input: a batch of contigs -------------------------------------------------
 * Mirrors the solver-relevant fields of PafReadData (src/paf_data.hpp:51-67).
 * All pointers are HOST pointers for aasm_solve_batch() and DEVICE pointers for
 * aasm_solve_device().                                                           */
typedef struct aasm_batch_in {
    int64_t n_contigs;
    int64_t n_records;            /* == ctg_rec_off[n_contigs]                     */
    int64_t n_ranges;             /* == rec_rng_off[n_records]                     */
    const int64_t *ctg_rec_off;   /* [n_contigs+1] record offsets, non-decreasing  */
    const int64_t *qry_str;       /* [n_records]  PafReadData::qry_str             */
    const int64_t *qry_end;       /* [n_records]  PafReadData::qry_end (closed)    */
    const int64_t *ref_str;       /* [n_records]  ref position of qry_str          */
    const int64_t *ref_end;       /* [n_records]  ref position of qry_end          */
    const int64_t *qry_total;     /* [n_records]  PafReadData::qry_total_length    */
    const int32_t *ref_chr;       /* [n_records]  dense reference-name id          */
    const uint8_t *aln_fwd;       /* [n_records]  1 = '+', 0 = '-'                 */
    const uint8_t *map_qul;       /* [n_records]  mapping quality                  */
    const int64_t *rec_rng_off;   /* [n_records+1] match-range offsets             */
    const int64_t *rng_qry_l;     /* [n_ranges]   qry_overlap_range[k].first       */
    const int64_t *rng_qry_r;     /* [n_ranges]   qry_overlap_range[k].second      */
    const int64_t *rng_ref_l;     /* [n_ranges]   ref_overlap_range[k].first       */
    /* Alternative to the three rng_* arrays (ABI 2): when rng_qry_l is NULL and cs_text is
     * not, the device derives the match ranges itself from the records' short-form cs tags
     * (get_overlap_range, paf_data.cpp:90-123, kernel aasm_k0_cs_ranges).  rec_rng_off and
     * n_ranges must still be given: a record's range count is its number of ':' operations. */
    const char    *cs_text;       /* cs tags back to back, each starting "cs:Z:"    */
    const int64_t *rec_cs_off;    /* [n_records+1] offsets into cs_text            */
} aasm_batch_in;

/* ---- options --------------------------------------------------------------------*/
typedef struct aasm_opts {
    int32_t max_paths;         /* MAX_PATH_COUNT, src/paf_data.cpp:729; 0 -> 10000   */
    int32_t non_skip_linkable; /* global NON_SKIP_LINKABLE, src/paf_data.hpp:12      */
    int32_t device;            /* HIP device ordinal                                  */
    int32_t collect_timing;    /* 1: bracket every kernel with HIP events            */
    int32_t keep_debug;        /* 1: keep device intermediates for aasm_debug_fetch   */
    int32_t reserved[3];       /* test hooks, 0 in production: see AASM_H0_* below  */
} aasm_opts;

/* Test hooks in aasm_opts.reserved: each forces one launch form (tests cross-check it against the default) or one fault path.
 * A multi-bit field is (word & MASK) >> SHIFT.  Word 1 > 0: contig ranges longer than this "do not fit" (aasm_solve_batch's range split). */
#define AASM_H0_SEQ_SELECT       0x1      /* K9 by the sequential selection kernel (default: plan-based)                     */
#define AASM_H0_HEAP_MW_ALL      0x2      /* K7: every contig's heaps by the several-waves-per-contig kernel                 */
#define AASM_H0_HEAP_MW_NONE     0x4      /* K7: none of them (default: by graph density)                                    */
#define AASM_H0_ENUM_HEAP        0x8      /* K8 on the d-ary heap queue (default: sorted front + sorted runs)                */
#define AASM_H0_ENUM_SMALL       0x10     /* K8 with the 40-entry front (default: for 14 * 256 < contigs <= 20 * 256, K > 21) */
#define AASM_H0_GRID_ORDER       0x20     /* workgroups take their work items in grid order (default: XCD by XCD)            */
#define AASM_H0_CHAIN_MASK       0xC0     /* the chain class (aasm_k67_chain; default: small batches, the long tail of big ones): */
#define AASM_H0_CHAIN_ALL        0x40     /*   every sparse contig                                                           */
#define AASM_H0_CHAIN_NONE       0x80     /*   none                                                                          */
#define AASM_H0_CHAIN_HALF       0xC0     /*   the contigs of at least the batch's mean size                                 */
#define AASM_H0_MW_MASK          0xFF00   /* K7's several-waves kernel (default: ranked, largest node bound first; waves per contig by
                                             how many contigs share the chip): 4 / 8 / 16 waves per contig, or ...          */
#define AASM_H0_MW_INPUT_ORDER   1        /*   input order, a block per contig of the batch                                  */
#define AASM_H0_MW_SHIFT         8
#define AASM_H0_GRAPH_LAUNCHES   0x10000  /* rows, reversed CSR and sweep headers by the separate launches (default: aasm_k46_graph
                                             for the contigs small enough)                                                   */
#define AASM_H2_LAUNCH_FAILURE   0x1      /* inject one failing kernel launch (must surface as AASM_E_HIP)                   */
#define AASM_H2_WRAP_DEVICES     0x2      /* aasm_solve_batch_multi wraps device ordinals around the devices that exist      */
#define AASM_H2_DIRTY_SCAN       0x4      /* the next scan's ticket counter as an aborted launch leaves it (AASM_E_HIP after 10 s) */
#define AASM_H2_CHAIN_HDR_LOST   0x8      /* the chain class's pre-pass wave of contig 0 never publishes the root's header   */
#define AASM_H2_CHAIN_DONE_LOST  0x10     /* ... nor that it is done (AASM_E_INTERNAL for the contig, nothing may hang)      */
#define AASM_H2_CHAIN_OWN_QUEUE  0x20     /* the chain class's heap wave keeps its own BFS queue (default: the order from a wave of
                                             its own while the class has at most AASM_CHAIN_ORD_MAX = 1 024 contigs)         */
#define AASM_H2_SMALL_ROOT_RING  0x40     /* that heap wave's ring of parents' roots has 4 entries, not 512                  */
#define AASM_H2_SORT_DEPTH_MASK  0xFF00   /* d + 1: the sort replay takes its heap sort fallback after d partition levels    */
#define AASM_H2_SORT_DEPTH_SHIFT 8

/* ---- output ---------------------------------------------------------------------
 * One element == one PafOutputData (src/paf_data.hpp:90-105).                      */
typedef struct aasm_out_elem {
    int64_t edited_qry_str, edited_qry_end;
    int64_t edited_ref_str, edited_ref_end;
    int32_t ctg_index;         /* index of the record inside its contig (input order) */
    int32_t is_alt_path;       /* tp:A:S if 1 (src/alignasm.cpp:438)                   */
} aasm_out_elem;

#define AASM_N_PHASES 16
typedef struct aasm_stats {
    int64_t n_vertices;        /* sum over contigs of V = N + P + 2                   */
    int64_t n_pairs;           /* sum of P (overlap vertices)                          */
    int64_t n_edges;           /* sum of E = get_edge_count(graph)                     */
    int64_t n_heap_nodes;      /* persistent leftist-heap nodes allocated              */
    int64_t n_paths_found;     /* sum of distances.size()                              */
    int64_t n_paths_converted; /* calls of edge_path_to_paf_path                       */
    int64_t n_unconnectable;   /* overlap pairs with no cut (paf_data.cpp:373-375)     */
    int64_t n_internal_errors; /* contigs that hit a must-not-happen state             */
    int64_t n_single;          /* contigs with one record (paf_data.cpp:235-239)       */
    int64_t range_steps;       /* match-range entries visited by the merges            */
    int64_t device_bytes;      /* peak device workspace                                */
    int64_t ispr_edges;        /* K9: edges relaxed by internal_shortest_path_recover  */
    int64_t ispr_vertices;     /* K9: window vertices expanded                         */
    int64_t path_edges;        /* K9: edges of recovered + upgraded paths              */
    int64_t out_elems;         /* K9: PafOutputData elements produced by conversions   */
    int64_t pq_pushes;         /* K8: priority-queue pushes                            */
    float   phase_ms[AASM_N_PHASES];  /* per-phase kernel time (HIP events), ms       */
    float   total_ms;                 /* whole device pipeline, ms                    */
    float   reserved_f[3];
} aasm_stats;

/* phase ids for aasm_stats::phase_ms */
enum {
    AASM_PH_SORT = 0,     /* K1 sort + parts (3 kernels)                  */
    AASM_PH_PAIRS,        /* K2 overlap slots + cut merge + vertex ids    */
    AASM_PH_EDGES,        /* K3/K4 CSR build + scores                     */
    AASM_PH_REVCSR,       /* reversed CSR                                 */
    AASM_PH_SPTREE,       /* K6 aasm_k6_rev_sweep alone                   */
    AASM_PH_FWD,          /* K5/K6 aasm_k5_fwd_sweep alone                */
    AASM_PH_HEAP,         /* K7 aasm_k7_heap alone                        */
    AASM_PH_ENUM,         /* K8 aasm_k8_enum alone                        */
    AASM_PH_SELECT,       /* K9 aasm_k9_select alone                      */
    AASM_PH_GATHER,       /* output compaction                            */
    AASM_PH_HEAP_PREP,    /* SP-tree children CSR + arena sizing          */
    AASM_PH_TOPO,         /* topologically ordered CSR copy for K9        */
    AASM_PH_MISC,
    AASM_PH_CS,           /* K0 aasm_k0_cs_ranges alone (only with cs_text input) */
    AASM_PH_FINAL,        /* K9 per-contig final pick (aasm_k9_sel_final)          */
    AASM_PH_CHAIN         /* aasm_k67_chain: K6 sweep + K7 pre-pass + K7 heaps of the chain class, beside each other */
};

/* Ragged result of a batch: three lists per contig, exactly the three output
 * vectors of solve_ctg_read.  `all` is a list of paths per contig.
 * Arrays are malloc'ed by the library, released by aasm_free_out().              */
typedef struct aasm_batch_out {
    int64_t n_contigs;
    int64_t *main_off;      /* [n_contigs+1] into main_elems                       */
    int64_t *alt_off;       /* [n_contigs+1] into alt_elems                        */
    int64_t *all_path_off;  /* [n_contigs+1] into all_elem_off (paths per contig)  */
    int64_t *all_elem_off;  /* [n_all_paths+1] into all_elems                      */
    aasm_out_elem *main_elems;
    aasm_out_elem *alt_elems;
    aasm_out_elem *all_elems;
    int64_t n_all_paths;
    int32_t *ctg_status;    /* [n_contigs] 0 ok, <0 AASM_E_* for that contig       */
    aasm_stats stats;
} aasm_batch_out;

/* ---- entry points -----------------------------------------------------------------*/

/* library / device probe.  Returns AASM_OK when a gfx950-class HIP device is usable. */
int  aasm_abi_version(void);
int  aasm_device_count(void);
int  aasm_init(int device);
const char *aasm_last_error(void);

/* solve_ctg_read over a batch (replaces the dispatch loop src/alignasm.cpp:346-397).
 * Host pointers in, host arrays out (malloc'ed into *out).                           */
int  aasm_solve_batch(const aasm_batch_in *in, const aasm_opts *opts, aasm_batch_out *out);
/* The same for contigs [c0, c1) of the batch (out then covers c1 - c0 contigs): a caller that streams a file solves one
 * range while it writes the rows of the range before (aasm_writer_*).  The batch is validated with the range c0 = 0.   */
int  aasm_solve_batch_range(const aasm_batch_in *in, int64_t c0, int64_t c1, const aasm_opts *opts, aasm_batch_out *out);

/* Contig-sharded solve across n_devices GPUs of one node (devices opts->device .. +n-1):
 * static per-contig partition, one host thread + stream per device, outputs concatenated
 * in contig order; no collective (contigs are independent, src/alignasm.cpp:351-359).    */
int  aasm_solve_batch_multi(const aasm_batch_in *in, const aasm_opts *opts, int n_devices, aasm_batch_out *out);

/* The partition aasm_solve_batch_multi uses, for callers that run one process per GPU (bench.py, MPI-style
 * launchers): cost[c] = estimated GPU cost of contig c (records + a graph-density term from the part sizes);
 * cuts[0..n_shards] = cut points of the contiguous partition whose fullest block is as light as a contiguous partition
 * allows (cuts[0] = 0, cuts[n] = n_contigs).  aasm_partition_costs: the same cut for caller-supplied costs.
 * Host pointers; only ctg_rec_off, qry_str and qry_end are read.                                       */
int  aasm_contig_costs(const aasm_batch_in *in, double *cost);
int  aasm_partition_contigs(const aasm_batch_in *in, int n_shards, int64_t *cuts);
int  aasm_partition_costs(const double *cost, int64_t n_contigs, int n_shards, int64_t *cuts);

/* The solver's generic single-source shortest paths, dijkstra() (src/k_shortest_walks.hpp:69-87), over a batch of
 * graphs that may contain cycles: graph g owns vertices [g_voff[g], g_voff[g+1]) (local ids 0..), rowptr is one CSR
 * row-pointer array over all vertices, col holds LOCAL head ids, w5 five int64 per edge {qry_score, ref_score, anom,
 * qul_nonzero, qul_total}, src the local source per graph.  d5 (5 int64 per vertex; unreachable = PafDistance::max()
 * = {-1,-1,-1,-1,0}) and prev (-1 = none) are exactly the reference's return values.  The reference's CLI never
 * calls dijkstra (is_dag = true, paf_data.cpp:728); this entry exists because the solver class offers it.  */
int  aasm_sssp_dijkstra(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5,
                        const int32_t *src, int64_t *d5, int32_t *prev, int device);

/* The solver's single-source shortest paths for graphs with negative weights, bellman_ford() (src/k_shortest_walks.hpp:91-129: a
 * round-counted SPFA), over a batch of graphs in aasm_sssp_dijkstra's layout.  The weight domain is dijkstra's without the clause
 * on the score sum's sign: |scores| < 2^39, anom 0..2, qul counts 0..1 (AASM_E_OVERFLOW outside).  Per graph g:
 *   status[g] = 0   d5 / prev are exactly the reference's two vectors (prev depends on the order of the relaxations, which is kept)
 *   status[g] = 1   a negative cycle - a relaxation in round n, n the graph's vertex count; this includes a cycle whose score sum
 *                   is not negative but round which the qul ratio keeps improving.  The reference returns no distance vector: the
 *                   graph's d5 is PafDistance::max() everywhere, its prev -1, and cycle[cycle_off[g] .. cycle_off[g + 1]) holds
 *                   detect_cycle()'s list (:94-107): closed, first entry == last entry, in edge direction, local vertex ids
 *   status[g] < 0   AASM_E_INVAL: the prev chain from the relaxed vertex met -1 before it repeated a vertex (the reference indexes
 *                   out of bounds there), no cycle is reported; AASM_E_INTERNAL: the queue's proven room ran out (must not happen)
 * A graph's status never fails the call, and the rest of the batch is solved.  cycle_off has n_graphs + 1 entries; cycle needs room
 * for g_voff[n_graphs] + n_graphs entries (a graph's closed cycle holds at most its vertex count + 1). */
int  aasm_sssp_bellman_ford(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5,
                            const int32_t *src, int64_t *d5, int32_t *prev, int32_t *status, int64_t *cycle_off, int32_t *cycle, int device);

/* The solver's topology_sort() (src/k_shortest_walks.hpp:132-156) and shortest_path_dag() (:160-175) - the two its command line
 * reaches, with is_dag = true - over a batch of graphs in aasm_sssp_dijkstra's layout.  Per graph g:
 *   status[g] = 0   the graph is acyclic.  order[g_voff[g] ..] is topology_sort()'s vector as local ids: Kahn's algorithm with a FIFO
 *                   queue - the vertices of in-degree 0 in ascending id, then a vertex when its last in-edge is processed, "last" in
 *                   (position of the tail in the queue, position in the tail's list); parallel edges count once each.  d5 / prev are
 *                   shortest_path_dag(g, src)'s two vectors: d[src] = IDENTITY, the vertices taken in that order, one whose distance
 *                   == PafDistance::max() skipped, each list walked in list order under the strict test d[to] > d[v] + w (CALC_SUM
 *                   mode).  So among candidates the order cannot tell apart the FIRST in (Kahn position of the tail, list position)
 *                   stays, with its own five numbers, and prev is its tail; and the sort covers the whole graph, not only what src
 *                   reaches.
 *   status[g] = 1   the graph holds a cycle (a self-loop included), anywhere in it.  The reference asserts; built with NDEBUG it
 *                   returns an empty order and relaxes nothing: order is -1 everywhere, d5 is PafDistance::max() everywhere except
 *                   IDENTITY at src, prev is -1 everywhere.
 * A graph's status never fails the call, and the rest of the batch is solved.  The weight domain of aasm_sssp_dag is
 * aasm_sssp_bellman_ford's (the DAG relaxation assumes no sign); it accepts at most 2^20 vertices and fewer than 2^31 edges per
 * graph (AASM_E_OVERFLOW before a device is touched), aasm_topology_sort fewer than 2^31 of either.  order may be NULL in
 * aasm_sssp_dag.  Layout and pointer errors are AASM_E_INVAL, as for the other graph entries. */
int  aasm_topology_sort(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col,
                        int32_t *order, int32_t *status, int device);
int  aasm_sssp_dag(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5,
                   const int32_t *src, int64_t *d5, int32_t *prev, int32_t *order /* may be NULL */, int32_t *status, int device);

/* Dial's bucketed BFS, k_weighted_bfs() (src/k_weighted_bfs.hpp:16-37; the solver runs it with lim = 2 on the anomaly weights,
 * src/paf_data.cpp:704-713), over a batch of digraphs that may contain cycles and parallel edges: same graph layout as
 * aasm_sssp_dijkstra, cost one int32 per edge in 0 .. lim (lim <= 7), src the local source per graph.  dist (-1 = unreachable)
 * and pre (-1 = none; LOCAL vertex ids) are exactly the vectors the reference fills - pre depends on the LIFO order inside a
 * bucket, which the kernel keeps (buckets staged in LDS, pushes compacted per bucket by ballot + prefix count). */
int  aasm_sssp_dial(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int32_t *cost,
                    const int32_t *src, int lim, int64_t *dist, int64_t *pre, int device);

/* ---- Resident graph batches: the five entries above over a checked batch that lives on one device, results left on the device ----
 * A batch is checked and made resident ONCE (aasm_graphs_upload from host arrays, which are copied and owned by the handle;
 * aasm_graphs_wrap_device over DEVICE arrays, which are borrowed: never written, never freed, and kept alive and unchanged by the
 * caller while the handle lives).  The *_device entries then take `src` and every output as DEVICE arrays the caller owns, in the
 * host entries' shapes (d5 [n_vertices * 5], prev / order / dist / pre [n_vertices], status [n_graphs], cycle_off [n_graphs + 1],
 * cycle room for n_vertices + n_graphs), enqueue everything on `stream` (a hipStream_t of the device, NULL = the null stream) and
 * touch no output outside its stated length.  When the stream gets there every output holds, word for word, what the host entry of
 * the same name returns for the same graphs and sources, with two differences: aasm_sssp_dial_device reports Dial's must-not-happen
 * bucket overflow as status[g] = AASM_E_INTERNAL instead of failing the call, and cycle_off / cycle are packed on the device.
 *
 * Pointers (as aasm_result_export): an array that is not empty must be memory of the batch's device, aligned to 8 bytes (4 for
 * int32 arrays) - else AASM_E_INVAL and nothing is enqueued; col must be non-NULL even with n_edges == 0.
 * An array's SIZE is not checked: the lengths are the caller's word, and an overstated one makes the kernels read past the array.
 * Creation checks: the host entries' (layout; the w5 domain of aasm_sssp_bellman_ford; with cost, lim 0..7 and the cost range), with
 * the host entries' codes and message texts, plus "graph offsets do not end at n_vertices" and "row pointers do not end at n_edges"
 * (AASM_E_INVAL).  aasm_graphs_wrap_device runs them as kernels in three stages (graph offsets, row pointers, edges), the host
 * reading one verdict word between stages: nothing is read through an offset before the stage that validated it has passed.  The
 * handle remembers the first edge whose score sum is negative: aasm_sssp_dijkstra_device on such a batch returns aasm_sssp_dijkstra's
 * AASM_E_OVERFLOW and message for it; bellman_ford and dag accept it.
 * Per call: the entry's size limits (2^20 vertices for _dag_device, fewer than 2^31 vertices or edges per graph) from counts the
 * handle keeps on the host; the sources by a small kernel whose one-word verdict is read back ("graph g: source outside it",
 * AASM_E_INVAL, nothing more enqueued); an entry whose array the batch lacks (w5, cost) is AASM_E_INVAL.
 * Waiting: topology_sort, dag, bellman_ford and dial return without waiting for the solve (their only host wait is the source
 * verdict; topology_sort has none).  dijkstra waits to the end: its heap room grows 1x, 4x, 16x, 64x for as long as any graph ran out
 * of it (one word per round, reduced on the device), and at 64x it returns aasm_sssp_dijkstra's AASM_E_OVERFLOW and message.
 * Working memory belongs to the handle, grows on demand and is kept between calls (aasm_debug_poison fills it before each call).  The
 * handle records an event behind each call, and a call on another stream makes that stream wait for it first: two streams may share
 * a handle.  aasm_graphs_free waits for the handle's work in flight; NULL is accepted. */
typedef struct aasm_graphs aasm_graphs;           /* a checked graph batch resident on one device */
typedef struct aasm_graphs_in {
    int64_t n_graphs, n_vertices, n_edges;        /* the arrays' lengths, stated by the caller */
    const int64_t *g_voff;   /* [n_graphs+1]   */
    const int64_t *rowptr;   /* [n_vertices+1] */
    const int32_t *col;      /* [n_edges]      */
    const int64_t *w5;       /* [n_edges*5] or NULL: no dijkstra / bellman_ford / dag on this batch */
    const int32_t *cost;     /* [n_edges]   or NULL: no dial */
    int32_t lim, reserved;   /* dial's lim (0..7), read only with cost */
} aasm_graphs_in;
int  aasm_graphs_upload(const aasm_graphs_in *host, int device, aasm_graphs **gb);              /* copies; the handle owns them */
int  aasm_graphs_wrap_device(const aasm_graphs_in *dev, int device, void *stream, aasm_graphs **gb); /* borrows; checked ON the device */
int  aasm_graphs_view(const aasm_graphs *gb, aasm_graphs_in *dev_view);
void aasm_graphs_free(aasm_graphs *gb);           /* waits for the handle's work in flight */

int  aasm_sssp_dijkstra_device    (aasm_graphs *gb, const int32_t *src, int64_t *d5, int32_t *prev, void *stream);
int  aasm_sssp_bellman_ford_device(aasm_graphs *gb, const int32_t *src, int64_t *d5, int32_t *prev, int32_t *status,
                                   int64_t *cycle_off, int32_t *cycle, void *stream);
int  aasm_topology_sort_device    (aasm_graphs *gb, int32_t *order, int32_t *status, void *stream);
int  aasm_sssp_dag_device         (aasm_graphs *gb, const int32_t *src, int64_t *d5, int32_t *prev, int32_t *order /* may be NULL */,
                                   int32_t *status, void *stream);
int  aasm_sssp_dial_device        (aasm_graphs *gb, const int32_t *src, int64_t *dist, int64_t *pre, int32_t *status, void *stream);

/* The solver's k shortest walks, k_shortest_walks(source, sink, k) with is_dag = true and kth_shortest_walk_recover()
 * (src/k_shortest_walks.hpp:177-290), over a batch of DAGs in aasm_sssp_dijkstra's layout and weight domain (score sum >= 0,
 * |scores| < 2^39, anom 0..2, qul counts 0..1), at most 2^20 vertices per graph, 1 <= k <= 2^24.  Results are the
 * reference's with the monotonic allocator's queue ties (node arena index, then insertion index).  A walk is reported as
 * caller CSR positions (global edge ids), source -> sink: a tree edge is the edge whose relaxation set best[], a sidetrack
 * the edge its heap node was inserted for, so parallel edges stay apart.  A graph with a cycle gets status AASM_E_INVAL and
 * no walks; the other graphs of the batch are solved.  Every array is allocated by the library: release with aasm_ksw_free.
 *
 * With AASM_KSW_CYCLES every graph of the call is solved as the reference does with is_dag = false, negative_edge = false
 * (its default, :65,185): the shortest-path tree is the one dijkstra() from the sink over the reversed graph leaves (:69-87),
 * also on a graph that happens to be acyclic, where it can differ from the DAG relaxation's tree among tied distances.  Walks
 * may repeat vertices and run through cycles and through the sink.  Three limits hold there, each per graph, the rest of the
 * batch being solved:
 *  - dijkstra makes at most 64 * (E + 2) pushes.  A cycle can improve a distance for ever (a larger qul_nonzero / qul_total
 *    ratio orders first and is not monotone under addition; the reference does not return): status AASM_E_OVERFLOW, no walks.
 *    A graph whose best[] is no tree into the sink (the sink's own distance improved round a cycle; the reference does not
 *    return either) gets AASM_E_INVAL and no walks, with d5 / best as dijkstra left them.
 *  - a walk has any number of edges: when a queued distance leaves |qry_score|, |ref_score| < 2^62 or anom, qul_nonzero,
 *    qul_total < 2^30 the enumeration ends with AASM_E_OVERFLOW; n_found, dist5 and the walks hold what was found before.
 *  - a graph whose walks hold more than 2^28 edges together keeps n_found and dist5, gets empty walk ranges and AASM_E_OVERFLOW.
 *
 * With AASM_KSW_NEGATIVE the weight domain is aasm_sssp_bellman_ford's: edges whose score sum is negative are accepted (without
 * it they are AASM_E_OVERFLOW, as ever).  Alone, the flag changes nothing else: the reference's is_dag = true ignores negative_edge,
 * and its DAG relaxation assumes no sign.  Beside AASM_KSW_CYCLES the solver runs as with negative_edge = true: the tree is the one
 * bellman_ford() from the sink over the reversed graph leaves (:186), which always ends, so the bound on pushes does not apply; a
 * graph with a negative cycle (aasm_sssp_bellman_ford's status 1) gets AASM_E_INVAL, no walks and d5 / best as max / -1 - the
 * reference has no distance vector to index there.  The tree guard and the other two limits hold unchanged. */
#define AASM_KSW_WALKS      0x1     /* fill walk_off / walk_edges                                                     */
#define AASM_KSW_TREE       0x2     /* fill d5 / best                                                                 */
#define AASM_KSW_CYCLES     0x4     /* graphs may hold cycles: the reference's is_dag = false                         */
#define AASM_KSW_NEGATIVE   0x8     /* edges may have a negative score sum: the reference's negative_edge = true      */
#define AASM_KSW_HOOK_ARENA 0x100   /* test hook, 0 in production: fill hook_arena / hook_hroot                       */
typedef struct aasm_ksw_out {
    int64_t  n_graphs, k;
    int64_t *n_found;          /* [n_graphs] distances.size() of the reference (0 .. k)                              */
    int64_t *dist5;            /* [n_graphs * k * 5] {qry, ref, anom, qnz, qtot} per walk (0 beyond n_found)         */
    int64_t *walk_off;         /* [n_graphs * k + 1] into walk_edges (empty beyond n_found); AASM_KSW_WALKS          */
    int64_t *walk_edges;       /* caller CSR positions, source -> sink; AASM_KSW_WALKS                               */
    int64_t *d5;               /* [VT * 5] distance to the sink (PafDistance::max() where there is none); AASM_KSW_TREE */
    int32_t *best;             /* [VT] next vertex towards the sink, local id (-1 = none); AASM_KSW_TREE              */
    int64_t *heap_nodes;       /* [n_graphs] heap nodes the reference allocates                                     */
    int32_t *status;           /* [n_graphs] 0, AASM_E_INVAL (cycle), AASM_E_OVERFLOW (a capacity or limit above) */
    int64_t *hook_arena;       /* AASM_KSW_HOOK_ARENA: {rank, key[5], u, v, left, right} per node, graph after graph */
    int32_t *hook_hroot;       /* AASM_KSW_HOOK_ARENA: [VT] heap root as the graph's arena index (-1 = nullptr)      */
} aasm_ksw_out;
int  aasm_k_shortest_walks(int64_t n_graphs, const int64_t *g_voff, const int64_t *rowptr, const int32_t *col, const int64_t *w5,
                           const int32_t *source, const int32_t *sink, int64_t k, int flags, int device, aasm_ksw_out *out);
void aasm_ksw_free(aasm_ksw_out *out);

/* k shortest walks on a resident graph batch (a handle that carries w5), results left on the device: a solve that returns sizes,
 * then an export into DEVICE arrays the caller allocates from them - the pattern of aasm_result_sizes / aasm_result_export.
 * `source` and `sink` are device arrays [n_graphs]; k and flags mean what they mean in aasm_k_shortest_walks, with every per-graph
 * status and limit of it (AASM_KSW_HOOK_ARENA is refused as an unknown flag).
 *
 * The result is PACKED by n_found instead of padded to k, and nothing in either entry allocates or touches n_graphs * k words:
 * found_off is the prefix sum of n_found, walk i of graph g is walk found_off[g] + i.  For the same graphs, sources, sinks, k and
 * flags, n_found, heap_nodes, status, d5 and best are word for word aasm_k_shortest_walks'; dist5[(found_off[g] + i) * 5 ..] is its
 * dist5[(g * k + i) * 5 ..] and walk found_off[g] + i holds the edge ids of its walk g * k + i, for i < n_found[g]; a graph it
 * reports with empty walk ranges has empty ranges here.
 *
 * aasm_k_shortest_walks_device.  Checks before anything is enqueued: the pointers (as the other *_device entries), the batch's
 * w5, 2^20 vertices and fewer than 2^31 edges per graph, k, the flags, and - without AASM_KSW_NEGATIVE - the batch's first edge
 * with a negative score sum (aasm_k_shortest_walks' AASM_E_OVERFLOW and message).  Sources and sinks are checked by a kernel with a
 * one-word verdict: "graph g: source outside it" / "graph g: sink outside it" (AASM_E_INVAL), the lowest g, its source first.
 * The solve is NOT asynchronous: it returns when *sz is final.  Its host waits do not grow with the batch: the host reads the
 * source / sink verdict, three totals after the tree stage (the arena, queue and result room: the per-graph bounds and the scans
 * that place them are made by a kernel), two totals after the enumeration, and under AASM_KSW_CYCLES without AASM_KSW_NEGATIVE one
 * word per round of heap room (1x, 4x, 16x: which graphs run again is decided on the device).  The whole batch is solved in one
 * piece out of the handle's working memory (aasm_debug_poison covers it); its size, every array rounded up to 256 bytes:
 *     80 B per vertex + 8 B per edge + 124 B per graph (+ 2 words)
 *   + the larger of the tree stage's heap room  (48 B x: nothing in DAG mode; 2 * (E + 2) entries per graph with AASM_KSW_NEGATIVE;
 *                with AASM_KSW_CYCLES alone E + 2 per graph, then 4, 16, 64 x (E + 2) for the graphs that run again)
 *     and the enumeration's                     (48 B x sum of arena nodes + 56 B x sum of queue entries + 44 B x sum of walks[g]),
 * where per graph with a walk arena nodes = ins * (floor(log2(ins + 1)) + 2) (ins: the sidetrack edges reachable from the sink's
 * tree, <= E), queue entries = 3 * walks - 2, walks = min(k, number of walks) - so at most about 200 B x k per graph beside the
 * arena.  While the block grows between the stages the old and the new one exist together.  If it cannot be had the call returns
 * AASM_E_NOMEM; the handle stays usable and the caller splits the batch.
 *
 * aasm_ksw_export_device is asynchronous on `stream`: no host wait, no read-back, no allocation, no cell touched outside the
 * stated lengths.  It may be called more than once for one solve.  AASM_E_INVAL with nothing enqueued: sz is not what the latest
 * k-walk solve on this handle returned; a later call on the handle (any *_device entry, another k-walk solve) has reused the
 * working memory the result lives in; an array that is not empty is NULL, not memory of the batch's device, or misaligned
 * (walk_off / walk_edges are asked for only with AASM_KSW_WALKS, d5 / best only with AASM_KSW_TREE).  The handle's event ordering
 * covers both entries: two streams may share a handle, and aasm_graphs_free waits for exports in flight. */
typedef struct aasm_ksw_sizes {      /* filled by the solve, handed back unchanged to the export */
    int64_t n_graphs, n_vertices, k;
    int64_t n_walks;                 /* sum of n_found                                  */
    int64_t n_walk_edges;            /* 0 without AASM_KSW_WALKS                        */
    int32_t flags, reserved;
    int64_t serial;                  /* which solve of this handle                      */
} aasm_ksw_sizes;
typedef struct aasm_ksw_dev_out {    /* DEVICE arrays, caller-owned */
    int64_t *n_found;      /* [n_graphs]                                                */
    int64_t *found_off;    /* [n_graphs + 1] prefix sums of n_found                     */
    int64_t *dist5;        /* [n_walks * 5]  walk i of graph g at found_off[g] + i      */
    int64_t *walk_off;     /* [n_walks + 1] into walk_edges; AASM_KSW_WALKS             */
    int64_t *walk_edges;   /* [n_walk_edges] caller CSR positions, source -> sink       */
    int64_t *d5;           /* [n_vertices * 5]; AASM_KSW_TREE                           */
    int32_t *best;         /* [n_vertices];     AASM_KSW_TREE                           */
    int64_t *heap_nodes;   /* [n_graphs]                                                */
    int32_t *status;       /* [n_graphs]                                                */
} aasm_ksw_dev_out;
int  aasm_k_shortest_walks_device(aasm_graphs *gb, const int32_t *source, const int32_t *sink, int64_t k, int flags, void *stream,
                                  aasm_ksw_sizes *sz);
int  aasm_ksw_export_device(aasm_graphs *gb, const aasm_ksw_sizes *sz, const aasm_ksw_dev_out *dst, void *stream);

/* Same, with the batch already resident in device memory (in->pointers are device
 * pointers; in->ctg_rec_off / rec_rng_off too).  `stream` is a hipStream_t (or NULL).
 * The device result stays resident in an opaque handle until fetched/freed.          */
typedef struct aasm_result aasm_result;
int  aasm_solve_device(const aasm_batch_in *dev_in, const aasm_opts *opts, void *stream,
                       aasm_result **res);
int  aasm_result_stats(const aasm_result *res, aasm_stats *stats);
int  aasm_result_fetch(aasm_result *res, aasm_batch_out *out);   /* D2H + ragged pack */
void aasm_result_free(aasm_result *res);
void aasm_free_out(aasm_batch_out *out);

/* ---- results on the device: the output path matching aasm_upload_batch -> aasm_solve_device ------------------------------
 * The arrays of aasm_result_fetch, built on the device (ragged pack kernels) into buffers the CALLER owns, so that a batch goes
 * from HBM to HBM and its answer outlives the next solve on the device (a result itself lives in the workspace arena, which the
 * next solve reuses).  Use: aasm_result_sizes -> allocate on the result's device -> aasm_result_export.                       */
typedef struct aasm_out_sizes {
    int64_t n_contigs;
    int64_t n_main;            /* main_elems entries (== main_off[n_contigs])          */
    int64_t n_alt;             /* alt_elems entries                                    */
    int64_t n_all_paths;       /* all_elem_off has n_all_paths + 1 entries            */
    int64_t n_all_elems;       /* all_elems entries                                    */
} aasm_out_sizes;
/* DEVICE pointers owned by the caller; same fields and meaning as aasm_batch_out's arrays */
typedef struct aasm_dev_out {
    int64_t *main_off;         /* [n_contigs+1]   */
    int64_t *alt_off;          /* [n_contigs+1]   */
    int64_t *all_path_off;     /* [n_contigs+1]   */
    int64_t *all_elem_off;     /* [n_all_paths+1] */
    aasm_out_elem *main_elems; /* [n_main]        */
    aasm_out_elem *alt_elems;  /* [n_alt]         */
    aasm_out_elem *all_elems;  /* [n_all_elems]   */
    int32_t *ctg_status;       /* [n_contigs]     */
} aasm_dev_out;
/* Counts and places the .all paths on the device and returns the five sizes.  NOT asynchronous: one small device->host copy
 * and a wait on the result's stream.  The device-side offsets it computes are kept in the result for the export.          */
int  aasm_result_sizes(aasm_result *res, aasm_out_sizes *sz);
/* Asynchronous on `stream` (a hipStream_t on the result's device; NULL = the null stream), no host wait: once the stream gets
 * there, dst holds exactly what aasm_result_fetch returns.  AASM_E_INVAL (nothing enqueued) when sz is not what
 * aasm_result_sizes returned for this result, when a later solve invalidated the result, or when an array that is not
 * empty is NULL, host memory, memory of another device or not 8-byte (ctg_status: 4-byte) aligned.  The next solve on the
 * device waits for the exports in flight before it reuses the workspace; the caller's buffers are never touched again.  */
int  aasm_result_export(aasm_result *res, const aasm_out_sizes *sz, const aasm_dev_out *dst, void *stream);

/* ---- cut plans: what a PAF row needs beyond an element's coordinates (get_edited_paf_data, src/paf_data.cpp:125-220) ------------
 * A re-cut record's cs tag is three pieces: [":" head_keep] + ONE stretch of the record's own tag + [":" tail_keep] (only the
 * first and the last kept ':' run can lose bases; every other operation stays or goes whole).  A plan holds the stretch as byte
 * offsets, so a row costs its writer one copy and no walk over the tag.                                                       */
typedef struct aasm_cut_plan {          /* 48 bytes, 8-byte aligned */
    int64_t keep_lo, keep_hi;           /* byte offsets inside the record's own tag (from its 'c' of "cs:Z:") of the operations kept whole: one stretch [keep_lo, keep_hi); equal = none */
    int64_t head_keep, tail_keep;       /* bases left of a shortened first / last ':' run in TEXT order; 0 = none */
    int32_t mat_num, aln_len;           /* PafEditData's, with the reference's int32 arithmetic */
    int32_t flags;                      /* AASM_CUT_* */
    int32_t reserved;                   /* 0 */
} aasm_cut_plan;
#define AASM_CUT_IS_CUT      0x1   /* 0: the element spans the whole record, take the record's own tag and columns 10 / 11; every other field is 0 */
#define AASM_CUT_IRREGULAR   0x2   /* a kept ':' run is not written as std::to_string writes it (":007"): mat_num / aln_len hold, the text must be rendered run by run */
#define AASM_CUT_E_TAG       0x10  /* malformed tag met during the walk */
#define AASM_CUT_E_INS_CLIP  0x20  /* "Alignment was clipped inside a cs insert" (paf_data.cpp:153-164) */
#define AASM_CUT_E_EDIT      0x40  /* "Edited cs tag does not match ..." (:209-218) */
#define AASM_CUT_E_RECORD    0x80  /* ctg_index outside the element's contig */
/* A plan with an error flag holds that flag (and AASM_CUT_IS_CUT for the three walk errors) and zeros.  Precedence is the host
 * codec's: tag, insert clip, edit check; the walk stops once its cursor has left the edited interval, so a malformed operation
 * behind that point is not reported (the solve that produced the elements has already rejected such a tag, AASM_E_PARSE).      */
typedef struct aasm_dev_cuts { aasm_cut_plan *main, *alt, *all; } aasm_dev_cuts;   /* DEVICE, caller-owned: [n_main], [n_alt], [n_all_elems] */

/* The plans of every element of an exported result, on the device: a pure function over device arrays (no aasm_result, no
 * workspace).  dev_in: the view aasm_upload_batch returned, with cs_text / rec_cs_off (a batch uploaded with rng_* arrays has no
 * tags on the device); sz, dev_out: what aasm_result_export filled.  An element's record is ctg_rec_off[c] + ctg_index, c from
 * main_off / alt_off, for .all from all_elem_off -> path -> all_path_off.  Asynchronous on `stream` (a hipStream_t of `device`;
 * NULL = the null stream): no host wait, no read-back, no allocation; behind an export on the same stream nothing is needed in
 * between.  AASM_E_INVAL (nothing enqueued) when dev_in has no cs text, when sz does not fit dev_in, or when an array that is
 * not empty is NULL, host memory, memory of another device or not 8-byte aligned.  Errors of one element go into its flags.   */
int  aasm_cut_plans_device(const aasm_batch_in *dev_in, const aasm_out_sizes *sz, const aasm_dev_out *dev_out,
                           const aasm_dev_cuts *dst, int device, void *stream);

/* Upload a host batch once and solve it repeatedly (benchmark path: inputs resident in
 * HBM before the timed region).  dev_view receives device pointers for aasm_solve_device. */
typedef struct aasm_upload aasm_upload;
int  aasm_upload_batch(const aasm_batch_in *host_in, int device, aasm_upload **up, aasm_batch_in *dev_view);
void aasm_upload_free(aasm_upload *up);

/* Start-up helper for a fresh process (no counterpart in the reference: its state is the CPU heap): creates the device
 * context and grows the workspace arena to `bytes` (capped at half of the free device memory) so that the first solve
 * does not pay HIP's start-up and the arena's hipMalloc calls.  Meant to run on a thread of its own while the caller
 * still reads its input (the CLI does: ~3.7 bytes of arena per byte of PAF text).  AASM_E_NOMEM is harmless here. */
int  aasm_reserve_workspace(int device, int64_t bytes);

/* Debug/parity hook: copy a named device intermediate of a result solved with
 * opts.keep_debug=1 (names listed in DESIGN.md; e.g. "perm", "csr_col", "sp_d").
 * Call with dst==NULL to get the byte size.                                           */
int64_t aasm_debug_fetch(aasm_result *res, const char *name, void *dst, int64_t dst_bytes);
/* Process-wide diagnostic counters (tests / tuning): "range_splits" (contig ranges halved after an
 * out-of-memory), "device_mallocs" (hipMalloc calls of the arenas), "stream_syncs" (host waits on a
 * pipeline stream), "read_slow_rows" / "read_host_fallbacks" (aasm_paf_parse_device), "read_containers" (containers built by
 * device reads).  Unknown name: -1.                                                                                    */
int64_t aasm_debug_counter(const char *name);
/* Process-wide debug switch (tests): 0 = off (production); 1..255 = the byte every allocator of device working memory fills
 * fresh memory with: the whole workspace arena at the start of each aasm_solve_device (and a block created during it), each
 * block of the generic graph entries (aasm_sssp_*, aasm_k_shortest_walks, the debug entries) and of the device reader.  A
 * kernel that reads a cell nobody wrote then meets the byte, not what the last tenant left.  Not filled: the scans' ticket /
 * tile words, pinned buffers, the rows' persistent words, aasm_upload memory.  Returns the previous value; -1 (nothing
 * changed) for a value outside 0..255.  Needs no device.                                                               */
int aasm_debug_poison(int byte);
/* Test entry for row T1: the device's PafDistance predicates (paf_data.hpp:142-168) on n pairs of
 * {qry, ref, anom, qul_nonzero, qul_total} tuples.  out[i] bit 0: a < b in CALC_SUM mode, bit 1: a < b in
 * QRY_SCORE mode, bit 2: a == b, bit 3: K7's node-key test, bit 4: K8's queue order (equal node / index), bit 5: the
 * same order as K8's default queue keeps it ({qry + ref, key2, node:index} words, aasm_enum.h qe_less / qe_key2). */
int  aasm_debug_predicates(const int64_t *a, const int64_t *b, int64_t n, uint8_t *out, int device);
/* Test entry for hazard B1: K1's replay of libstdc++'s std::sort (paf_data.cpp:241-246 sorts with an unstable sort, so the
 * order of records with equal (qry_str, qry_end) is whatever that algorithm leaves) alone, on arbitrary keys.
 * rec_off[n_contigs + 1] starts at 0; perm_out[rec_off[c] + r] = the input index, relative to contig c, that ends at
 * sorted position r.  depth_test: 0, or d + 1 for a depth limit of d partition levels (as AASM_H2_SORT_DEPTH_MASK). */
int  aasm_debug_sort_replay(const int64_t *rec_off, int64_t n_contigs, const int64_t *qs, const int64_t *qe, int32_t *perm_out,
                            int depth_test, int device);

/* ---- host-side codec + file contract (reference: src/paf_data.cpp:19-220,
 *      src/alignasm.cpp:76-183,398-490).  Implemented in host C++.                  */
typedef struct aasm_paf aasm_paf;    /* parsed PAF file: names, records, cs strings   */

int  aasm_paf_read(const char *path, aasm_paf **paf);              /* alignasm.cpp:76-183 */
/* Host threads of the PAF reader and the output writers (row-parallel; results do not depend
 * on it).  The reference's -t/--thread (alignasm.cpp:45-49,346-352) sizes the TBB arena that
 * runs solve_ctg_read; here that work is on the GPU and -t sizes the host codec instead.
 * 0 = the CPUs this process may use - hardware threads cut to the affinity mask and the cgroup CPU
 * quota, at most 64 (default).  Returns the previous setting. */
int  aasm_set_host_threads(int n);
int  aasm_paf_parse_mem(const char *text, int64_t len, aasm_paf **paf);
/* Reader flags.  AASM_READ_DEVICE_RANGES: do not build the match ranges on the host; rows are
 * only indexed and their ':' operations counted, aasm_paf_batch() then hands out cs_text /
 * rec_cs_off with NULL rng_* pointers and the solver parses the cs tags on the GPU (a malformed
 * tag is then reported by the solve call, AASM_E_PARSE, instead of by the reader).           */
#define AASM_READ_DEVICE_RANGES 1
int  aasm_paf_read_opts(const char *path, int flags, aasm_paf **paf);
int  aasm_paf_parse_mem_opts(const char *text, int64_t len, int flags, aasm_paf **paf);
/* The device reader: host text in, a resident batch in the cs form out (cs_text / rec_cs_off, rng_* NULL: ready for
 * aasm_solve_device and aasm_cut_plans_device) and the container the writers need.  The device frames the rows and parses the
 * twelve columns itself; the host copies the tags into the container from its own text, at offsets the device computed.
 *   text      HOST memory, the bytes of a PAF file (aasm_paf_read_device: the file is mapped).
 *   *paf      equal, field for field, to aasm_paf_parse_mem_opts(text, len, AASM_READ_DEVICE_RANGES, ...).  paf may be NULL: no
 *             container is built.
 *   *up       owns every device array; release with aasm_upload_free.  *dev_view: what aasm_upload_batch(aasm_paf_batch(paf)) gives.
 *             up and dev_view may both be NULL: only the container is built.
 * Errors: AASM_E_INVAL (NULL text, negative len, one of up / dev_view alone, nothing asked for), AASM_E_NODEVICE, AASM_E_NOMEM /
 * AASM_E_HIP (a failed HIP call is not retried).  A text the device finds fault with (fewer than 12 columns, no cs:Z: tag, a number
 * strtoll does not take whole, a row too long, no rows) is read again by the host reader, whose code and message are returned:
 * the first bad row in file order, a malformed tag in an earlier row included.  A malformed tag in an otherwise well-formed
 * file is reported by the solve, as with AASM_READ_DEVICE_RANGES.  Numbers off the fast path ([-] and 1 - 18 digits) are
 * resolved by the host, row by row.  aasm_debug_counter: "read_slow_rows" (such rows in the last device read),
 * "read_host_fallbacks" (device reads that reran the host reader).                                                        */
#define AASM_READ_H_WEAK_HASH 0x100   /* test hook, 0 in production: the reference-name hash is (length & 3) */
#define AASM_READ_H_FEW_BLOCKS 0x200  /* test hook, 0 in production: every reader grid is capped at 3 blocks (grid-stride loops) */
int  aasm_paf_parse_device(const char *text, int64_t len, int flags, int device, aasm_paf **paf, aasm_upload **up, aasm_batch_in *dev_view);
int  aasm_paf_read_device(const char *path, int flags, int device, aasm_paf **paf, aasm_upload **up, aasm_batch_in *dev_view);
/* The device reader that also leaves the row columns resident: *dev_cols is, array for array and byte for byte, what
 * aasm_paf_upload_rows(P, 0, n_contigs, ...) gives for the host reader's container P of the same text (names: the contig names back
 * to back, then the reference names in first-appearance order; row_index[r] = r, cord_type[r] = 0).  The numeric columns are the
 * ones the device parsed, the names are copied out of the text on the device.  up, dev_view and dev_cols are required; *up owns
 * the batch's arrays and the columns' arrays, one aasm_upload_free releases both.  paf may be NULL: then no container is built -
 * no tag pool, no column fetch, no host pass over the text - and solve, cut plans, rows and aasm_writer_append_device (paf = NULL)
 * run from the resident arrays alone.  Errors, host fallback, slow rows and counters as aasm_paf_parse_device; aasm_debug_counter
 * "read_containers": containers built by device reads in this process.
 *   AASM_READ_ROW_COLS        what these entries add to a device read (they imply it; aasm_paf_parse_device ignores it).
 *   AASM_READ_TEXT_ON_DEVICE  text is device memory of `device`, 16-byte aligned, complete before the call; the library does not
 *                             copy it and never frees or writes it.  Only with paf = NULL (AASM_E_INVAL otherwise, as for a
 *                             misaligned pointer, host memory or memory of another device; nothing is enqueued).  The host steps
 *                             fetch what they need: a slow row's bytes, and the whole text once when the read has failed and
 *                             the host reader says why.  The call is synchronous.                                          */
#define AASM_READ_ROW_COLS 2
#define AASM_READ_TEXT_ON_DEVICE 4
struct aasm_row_cols;
int  aasm_paf_parse_device_rows(const char *text, int64_t len, int flags, int device, aasm_paf **paf, aasm_upload **up,
                                aasm_batch_in *dev_view, struct aasm_row_cols *dev_cols);
int  aasm_paf_read_device_rows(const char *path, int flags, int device, aasm_paf **paf, aasm_upload **up, aasm_batch_in *dev_view,
                               struct aasm_row_cols *dev_cols);
/* --alt merge of a second PAF of sub-contig re-alignments (alignasm.cpp:186-332) */
int  aasm_paf_merge_alt(aasm_paf *paf, const char *alt_path, double alt_baseline);
int  aasm_paf_merge_alt_mem(aasm_paf *paf, const char *text, int64_t len, double alt_baseline);
void aasm_paf_free(aasm_paf *paf);
int  aasm_paf_batch(const aasm_paf *paf, aasm_batch_in *view);      /* borrowed pointers  */
int64_t aasm_paf_n_contigs(const aasm_paf *paf);
/* write <stem>.aln.paf / .aln.alt.paf / .aln.all.paf (alignasm.cpp:407-490)          */
int  aasm_paf_write_outputs(const aasm_paf *paf, const aasm_batch_out *out,
                            const char *main_path, const char *alt_path, const char *all_path);
/* The same in pieces: the three files are opened once (under temporary names), receive the rows of consecutive contig
 * ranges in order (out = the result of contigs [contig0, contig0 + out->n_contigs)), and take their final names at
 * aasm_writer_close(w, 1); close(w, 0), or any failed append, removes them.                                        */
typedef struct aasm_writer aasm_writer;
int  aasm_writer_open(const char *main_path, const char *alt_path, const char *all_path, aasm_writer **w);
int  aasm_writer_append(aasm_writer *w, const aasm_paf *paf, const aasm_batch_out *out, int64_t contig0);
int  aasm_writer_close(aasm_writer *w, int commit);
/* aasm_writer_append with the rows' mat_num, aln_len and tag pieces taken from cut plans (aasm_cut_plans_device, fetched to the
 * host) instead of a walk over every re-cut record's tag; the files are byte for byte those of aasm_writer_append.  A plan with
 * AASM_CUT_IRREGULAR is rendered by the walk as before; one with an error flag fails the append with the host codec's code and
 * message for that error; counts that are not out's, a plan that disagrees with its element about being cut, or a stretch outside
 * the record's tag give AASM_E_INVAL.                                                                                          */
typedef struct aasm_cuts { int64_t n_main, n_alt, n_all; aasm_cut_plan *main, *alt, *all; } aasm_cuts;   /* HOST arrays, parallel to aasm_batch_out's element lists */
int  aasm_writer_append_cuts(aasm_writer *w, const aasm_paf *paf, const aasm_batch_out *out, const aasm_cuts *cuts, int64_t contig0);
/* ---- output rows on the device: from an exported result and its cut plans to the bytes of the three files --------------------------
 * A row is what emit_line (aasm_paf.cpp) writes, byte for byte: for element o of contig c, record r = ctg_rec_off[c] + o.ctg_index,
 *   name \t qry_total[r] \t o.qs \t o.qe+1 \t (+|-) \t chr_name[ref_chr[r]] \t ref_total[r] \t A \t B+1 \t mat \t aln \t map_qul[r]
 *   \t tp:A:(S|P) \t xi:Z:(P_|A_)row_index[r] \t TAG \n
 * (A, B) = (o.rs, o.re) on '+', (o.re, o.rs) on '-'; name = ctg_name[c], in .all ctg_name[c] "." (path's number in c, from 1);
 * an element that spans its record (plan flags 0) takes the record's whole tag and its mat_num / aln_len, a cut one takes
 * "cs:Z:" [":" head_keep] tag[keep_lo, keep_hi) [":" tail_keep] and the plan's counts; a plan with AASM_CUT_IRREGULAR is rendered
 * on the device by the walk (every surviving ':' run as ":" + its kept bases, every other surviving operation as it stands).
 * Use: aasm_paf_upload_rows (once per container) -> aasm_rows_sizes_device -> aasm_rows_format_device per list and range.        */
/* DEVICE arrays: what an output row prints beyond aasm_batch_in.  names: contig names, then reference names, back to back. */
typedef struct aasm_row_cols {
    int64_t n_chr;
    const int64_t *ref_total;                       /* [n_records] */
    const int32_t *mat_num, *aln_len, *row_index;   /* [n_records] */
    const uint8_t *cord_type;                       /* [n_records] 0 = P_, 1 = A_ */
    const char    *names;
    const int64_t *ctg_name_off;                    /* [n_contigs+1] into names */
    const int64_t *chr_name_off;                    /* [n_chr+1]     into names */
} aasm_row_cols;
/* the row columns of contigs [c0, c1) of a container (after a --alt merge too), uploaded once; release with aasm_upload_free */
int  aasm_paf_upload_rows(const aasm_paf *paf, int64_t c0, int64_t c1, int device, aasm_upload **up, aasm_row_cols *dev_cols);

/* The --alt merge on the device: the second PAF joins a batch that is resident in its cs form (cs_text / rec_cs_off, rng_* NULL)
 * with its row columns - what aasm_paf_parse_device_rows gives, or aasm_upload_batch plus aasm_paf_upload_rows.  The merged batch
 * equals, array for array and byte for byte, aasm_paf_parse_mem_opts(main, AASM_READ_DEVICE_RANGES) -> aasm_paf_merge_alt_mem(alt,
 * baseline) -> aasm_paf_batch / aasm_paf_upload_rows(0, C): every contig is its main records followed by the kept alt rows in
 * alt-file order, rec_rng_off holds the ':' counts, row_index is the alt row's number among the non-empty lines (cord_type 1), new
 * reference names are numbered behind the main file's in first-appearance order over all alt rows and appended to `names`.
 *   dev_in, dev_cols  DEVICE arrays, read only, never freed; the input batch stays usable whatever the call returns.
 *   alt_text          HOST memory, the bytes of the alt PAF.  A text without rows gives a merged batch equal to the input.
 *   flags             0; AASM_READ_H_WEAK_HASH, AASM_READ_H_FEW_BLOCKS: the reader's test hooks, for every table and grid of the merge.
 *   *up               a new handle that owns every array of *merged_view and *merged_cols (one aasm_upload_free); NULL on failure.
 * Declined texts (AASM_E_PARSE, nothing built, counter "alt_host_verdicts"): a row with fewer than 12 columns, without a cs:Z: tag
 * or with a number that is none; a piece name that is not <name>:<1 - 18 digits>[-...]; a group of rows without a positive
 * aln_len / qry_total ratio (its zeroed stand-in is the host's to rebuild); more than INT32_MAX records.  The host's own scan of
 * the alt rows then speaks: if it finds the text bad, the message is its text for the first bad row in file order, else
 * "aasm_paf_merge_alt_device: the device does not merge this alt text (<reason>, alt row <n>); merge on the host".
 * A malformed cs tag in an otherwise well-formed alt row is NOT found here (the host merge finds it): as with
 * AASM_READ_DEVICE_RANGES it is reported by the solve of the merged batch, AASM_E_PARSE.  Numbers off the fast path are resolved by
 * the host, row by row.  Other errors: AASM_E_INVAL (a NULL or host pointer where device memory is required, a batch with rng_* or
 * without cs_text, a negative alt_len; nothing enqueued), AASM_E_NODEVICE, AASM_E_NOMEM, AASM_E_HIP (never retried).
 * aasm_debug_counter "alt_device_merges": merges the device completed.                                                        */
int  aasm_paf_merge_alt_device(const aasm_batch_in *dev_in, const aasm_row_cols *dev_cols, const char *alt_text, int64_t alt_len, double alt_baseline,
                               int flags, int device, aasm_upload **up, aasm_batch_in *merged_view, aasm_row_cols *merged_cols);

typedef struct aasm_dev_rows { int64_t *main_off, *alt_off, *all_off; } aasm_dev_rows;  /* DEVICE, caller-owned: [n_main+1], [n_alt+1], [n_all_elems+1] */
typedef struct aasm_rows_info {
    int64_t bytes[3];          /* text bytes of main / alt / all */
    int64_t n_flagged;         /* elements that cannot be formatted */
    int64_t bad_elem; int32_t bad_list, bad_flags;   /* the first of them in file order; -1 / 0 / 0 when none */
} aasm_rows_info;
/* bad_flags: the plan's AASM_CUT_E_* flags (AASM_CUT_E_RECORD also for a ctg_index outside the element's contig), or one of */
#define AASM_ROWS_E_PLAN     0x100  /* the plan disagrees with its element about being cut ("cut plan does not belong to its output element") */
#define AASM_ROWS_E_STRETCH  0x200  /* the stretch lies outside the record's tag, or a negative head / tail ("cut plan reaches outside the record's cs tag") */
#define AASM_ROWS_H_FEW_BLOCKS 0x200  /* flags, test hook, 0 in production: every rows grid is capped at 3 blocks (grid-stride loops) */
/* The byte length of every row and their prefix sums: row_off[l][i] = file offset of row i of list l, row_off[l][n] = bytes[l].
 * As aasm_result_sizes NOT asynchronous: ordered behind what is already enqueued on `stream`, one small read-back and a wait.
 * An element whose plan carries an AASM_CUT_E_* flag, whose plan disagrees with it about being cut, or whose stretch is outside
 * its record's tag has length 0 and is counted in n_flagged; the first one in file order (main, alt, all; lowest index) is named.
 * AASM_E_INVAL as aasm_cut_plans_device.                                                                                       */
int  aasm_rows_sizes_device(const aasm_batch_in *dev_in, const aasm_row_cols *dev_cols, const aasm_out_sizes *sz,
                            const aasm_dev_out *dev_out, const aasm_dev_cuts *cuts, const aasm_dev_rows *row_off,
                            int flags, int device, void *stream, aasm_rows_info *info);
/* The rows [e0, e1) of list `list` (0 main, 1 alt, 2 all) into text, whose byte 0 is file offset row_off[list][e0]; it must hold
 * row_off[list][e1] - row_off[list][e0] bytes, and no byte outside them is touched: ranges concatenate to the file.  As
 * aasm_cut_plans_device asynchronous on `stream`: no host wait, no read-back, no allocation.  AASM_E_INVAL (nothing enqueued)
 * when info->n_flagged != 0, when e0 > e1 or e1 > the list's elements, when info is not what aasm_rows_sizes_device returned for
 * these row_off arrays, or when an array that is not empty is NULL, host memory, memory of another device or misaligned.
 * The library remembers the 64 most recent sizes calls per device, by their three row_off arrays: a later sizes call on the same
 * three arrays replaces the earlier one (whose info is refused from then on), and the info of a call that 64 calls on other
 * arrays have followed is refused too ("info is not what aasm_rows_sizes_device returned for these row_off arrays"); calling
 * aasm_rows_sizes_device again makes it valid.  A caller that keeps more than 64 sized results per device re-sizes before it
 * formats.                                                                                                                     */
int  aasm_rows_format_device(const aasm_batch_in *dev_in, const aasm_row_cols *dev_cols, const aasm_out_sizes *sz,
                             const aasm_dev_out *dev_out, const aasm_dev_cuts *cuts, const aasm_dev_rows *row_off,
                             const aasm_rows_info *info, int list, int64_t e0, int64_t e1, char *text,
                             int flags, int device, void *stream);

/* aasm_writer_append with the rows formatted on the device: the three lists' text is made in pieces of at most piece_bytes
 * (0 = default; a row longer than a piece gets a piece of its own), brought back through pinned staging and written in order,
 * piece k + 1 being formatted while piece k is copied back and written.  dev_in .. cuts: the resident batch, the row columns of the
 * same contigs, the exported result and its plans, all on `device`; the files are byte for byte those of aasm_writer_append for
 * the same result, and the session rules are its own.  A result with an element that cannot be formatted writes nothing and fails
 * the append with the code and message of aasm_writer_append_cuts on the same inputs.
 * paf may be NULL (a batch read by aasm_paf_parse_device_rows without a container): the session's checks then take the contig
 * count from sz and the presence of tags from dev_in->cs_text, the bytes written are the same, and a result with an element that
 * cannot be formatted writes nothing and fails with AASM_E_PARSE (a tag, insert-clip or edit flag) or AASM_E_INVAL (a record or
 * plan fault) and the message "<count> output elements cannot be formatted; the first: list <main|alt|all>, element <index>,
 * flags 0x<flags>".                                                                                                         */
int  aasm_writer_append_device(aasm_writer *w, const aasm_paf *paf, const aasm_batch_in *dev_in, const aasm_row_cols *dev_cols,
                               const aasm_out_sizes *sz, const aasm_dev_out *dev_out, const aasm_dev_cuts *cuts,
                               int64_t contig0, int64_t piece_bytes, int device);
/* get_overlap_range (paf_data.cpp:90): returns #ranges or <0; arrays may be NULL      */
int64_t aasm_cs_match_ranges(const char *cs, int64_t cs_len, int aln_fwd,
                             int64_t qry_str, int64_t qry_end, int64_t ref_str, int64_t ref_end,
                             int64_t *qry_l, int64_t *qry_r, int64_t *ref_l, int64_t cap);
/* get_edited_paf_data (paf_data.cpp:125): re-cut a cs tag; returns length written     */
int64_t aasm_cs_edit(const char *cs, int64_t cs_len, int aln_fwd,
                     int64_t qry_str, int64_t qry_end,
                     int64_t e_qry_str, int64_t e_qry_end, int64_t e_ref_str, int64_t e_ref_end,
                     char *out_cs, int64_t cap, int32_t *mat_num, int32_t *aln_len, int32_t *is_cut);

/* ---- synthetic PAF generator (SURVEY.md Appendix C spec; own code) -----------------*/
typedef struct aasm_synth_cfg {
    int64_t n_contigs;
    int64_t recs_per_contig;   /* fixed size, or the mean when heavy_tail=1            */
    uint64_t seed;
    int32_t dense;             /* 0 sparse, 1 dense/high-multiplicity                  */
    int32_t heavy_tail;        /* log-normal contig sizes                              */
    int32_t dup_every;         /* >0: duplicate every n-th record on another chr (ties)*/
    int32_t reserved;          /* bit 0: shuffle records inside a contig; bit 1: no cs tags; bit 2: records only (no match
                                  ranges, no cs: the form the contig cost model reads)                            */
} aasm_synth_cfg;
int  aasm_synth_paf(const aasm_synth_cfg *cfg, aasm_paf **paf);     /* full PAF w/ cs  */
/* contigs [first, first + count) of that file: a contig has its own PRNG stream, so the range equals the same contigs of the
   whole (BASELINE configs[3] / [4]: a rank of a contig-sharded run generates only its own block of the one file)            */
int  aasm_synth_paf_range(const aasm_synth_cfg *cfg, int64_t first, int64_t count, aasm_paf **paf);
int  aasm_paf_to_text(const aasm_paf *paf, char **text, int64_t *len); /* free()       */
int  aasm_paf_save(const aasm_paf *paf, const char *path);          /* the same text written to a file (no 2 GiB limit on the caller's side) */

#ifdef __cplusplus
}
#endif
#endif /* ALIGNASM_AMD_H */
