// aasm_paf.hpp -- host-side PAF container shared by the codec, the generator and the CLI.
// Mirrors what the reference keeps per record in PafReadData (src/paf_data.hpp:51-67)
// plus the per-file tables of src/alignasm.cpp:87-98 (contig names, reference names).
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/alignasm_amd.h"

namespace aasm {
// resize() without the zero fill: the big arrays (match ranges, cs text: GBs at whole-genome
// scale) are sized once and then written, and first touched, by all reader threads at once
template <class T> struct default_init_alloc : std::allocator<T> {
    template <class U> struct rebind { using other = default_init_alloc<U>; };
    template <class U, class... A> void construct(U *p, A &&...a) {
        if constexpr (sizeof...(A) == 0) ::new ((void *)p) U; else ::new ((void *)p) U(std::forward<A>(a)...);
    }
};
using big_i64 = std::vector<int64_t, default_init_alloc<int64_t>>;
using big_char = std::vector<char, default_init_alloc<char>>;
}  // namespace aasm

// X(type, name) for every per-record column (one value per record, input order): the arrays below and the codec's
// record type (aasm_paf.cpp) derive from this one list
#define AASM_PAF_RECORD_COLUMNS(X)                                                                                      \
    X(int64_t, qry_str) X(int64_t, qry_end) X(int64_t, ref_str) X(int64_t, ref_end) X(int64_t, qry_total)              \
    X(int64_t, ref_total) X(int32_t, ref_chr) X(int32_t, mat_num) X(int32_t, aln_len) X(int32_t, row_index)            \
    X(uint8_t, aln_fwd) X(uint8_t, map_qul) X(uint8_t, cord_type) /* cord_type: TYPE_MAIN=0 / TYPE_ALT=1 */

struct aasm_paf {
    // per contig (consecutive rows with the same query name, alignasm.cpp:125-133)
    std::vector<std::string> ctg_name;
    std::vector<int64_t> ctg_rec_off;          // [C+1]
    // per record, input order
#define AASM_X(T, name) std::vector<T> name;
    AASM_PAF_RECORD_COLUMNS(AASM_X)
#undef AASM_X
    std::vector<int64_t> cs_off;               // [R+1] into cs_pool (each entry "cs:Z:...")
    aasm::big_char cs_pool;
    bool has_cs = true;                        // generator may skip cs strings (bench)
    bool device_ranges = false;                // AASM_READ_DEVICE_RANGES: rng_* stay empty, rec_rng_off holds the counts
    // reference names (chr_map / chr_rev_map, alignasm.cpp:90-93)
    std::vector<std::string> chr_name;
    // match ranges (get_overlap_range, paf_data.cpp:90-123)
    std::vector<int64_t> rec_rng_off;          // [R+1]
    aasm::big_i64 rng_qry_l, rng_qry_r, rng_ref_l;
    std::string error;

    int64_t n_contigs() const { return (int64_t)ctg_name.size(); }
    int64_t n_records() const { return (int64_t)qry_str.size(); }
};

namespace aasm {
// cs codec (own implementation of the behaviour of paf_data.cpp:19-220)
void set_last_error(const std::string &msg);
const char *last_error_text();
// message of the tokenizer / get_overlap_range for one record (used when the device reports a bad cs tag)
std::string cs_error_message(const char *cs, int64_t cs_len, bool aln_fwd, int64_t qry_str, int64_t qry_end, int64_t ref_str, int64_t ref_end);
int host_threads();                          // aasm_set_host_threads (0 = all hardware threads), resolved
// the device reader's slow path (aasm_read.h): one line without its line end through the host's parse_row + record_of; false: no row
struct ReadRowCols { int64_t qry_str, qry_end, ref_str, ref_end, qry_total, ref_total; int32_t mat_num, aln_len; uint8_t aln_fwd, map_qul; int64_t aln_len64; };   // aln_len64: column 11 in full
bool read_slow_row(const char *s, const char *e, ReadRowCols &out);
// the --alt merge on the device (aasm_alt.h) declined a text: scan_alt_rows' code and message for it (AASM_OK: the host takes it)
int alt_host_verdict(const char *text, int64_t len, std::string &err);
// The device writer's (aasm_writer_append_device, aasm_gpu.hip) way into a writer session, whose struct stays aasm_paf.cpp's:
// begin: aasm_writer_append's argument and session checks for contigs [contig0, contig0 + n_contigs), nothing changed;
// has: file i of the session is open;  put: append these bytes to file i of the session;  end: the range is done with rc (a
// failure marks the session failed);  row_verdict: emit_line's code and message for one element and its plan (0: it formats).
int writer_device_begin(aasm_writer *w, const aasm_paf *paf /* or nullptr: no container */, int64_t contig0, int64_t n_contigs, bool has_cs);
bool writer_device_has(const aasm_writer *w, int file);
int writer_device_put(aasm_writer *w, int file, const char *bytes, int64_t n);
void writer_device_end(aasm_writer *w, int64_t n_contigs, int rc);
int writer_row_verdict(const aasm_paf *paf, int64_t contig, const std::string &name, const aasm_out_elem &o, const aasm_cut_plan &plan, std::string &err);
// aasm_shard.cpp: per-contig cost estimate and the contiguous cost-balanced partition built on it
void contig_costs(const aasm_batch_in *in, double *cost);
void partition_by_cost(const double *cost, int64_t C, int n_shards, int64_t *cuts);
}  // namespace aasm
