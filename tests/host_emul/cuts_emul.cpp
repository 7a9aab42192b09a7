// tests/host_emul/cuts_emul.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The cut-plan kernel (alignasm_amd/csrc/aasm_cut.h: kb_cut_plan, launched by cut_launch) compiled for the HOST with one lane
// per block, so the CPU tier can check it against the recorded reference vectors and the host codec.
//  * libaasm_emul_cuts.so: emc_cut_plans(), the entry's argument order with host arrays.
//  * cuts_emul_san: the same body in a program built with the host address sanitizer, which plans every record from a private
//    copy of its tag, so that a read outside [rec_cs_off[r], rec_cs_off[r + 1]) ends the program.
#define AASM_HOST_EMUL 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../alignasm_amd/csrc/aasm_cut.h"
#include "emul_launch.h"

using namespace aasm;

namespace {
AASM_EMUL_ROWS(cut_rows, AASM_CUT_KERNELS);
struct EmuCut {
    int64_t max_blocks;                                              // (fewer blocks than chunks: the grid-stride loop)
    void launch_cut(int kc, int64_t nblocks, int nthreads, const CutArgs &a) {
        emul_launch(cut_rows, kc, nthreads, 0, nblocks, max_blocks, [&](const KCtx &k) { run_cut_body(kc, k, a); });
    }
};
int run(const aasm_batch_in *in, const aasm_out_sizes *sz, const aasm_dev_out *out, const aasm_dev_cuts *dst, int64_t max_blocks) {
    if (!in || !sz || !out || !dst || !in->cs_text || !in->rec_cs_off) return AASM_E_INVAL;
    CutArgs a;
    if (!cut_args(*in, *sz, *out, *dst, a)) return AASM_E_INVAL;
    EmuCut be{max_blocks};
    cut_launch(be, a);
    return AASM_OK;
}
}  // namespace

extern "C" {
// aasm_cut_plans_device on host arrays; max_blocks > 0 caps the grid
int emc_cut_plans(const aasm_batch_in *in, const aasm_out_sizes *sz, const aasm_dev_out *out, const aasm_dev_cuts *dst, int64_t max_blocks) {
    return run(in, sz, out, dst, max_blocks);
}
int64_t emc_chunk(void) { return AASM_CUT_CHUNK; }
}

#if defined(AASM_EMUL_SAN_MAIN)
#include "emul_san.h"
// cuts_emul_san IN OUT, for a batch of one-record contigs with main elements only.  IN = int64 {R, NM, text bytes}, then qs[R],
// qe[R], cs_off[R + 1], main_off[R + 1], the NM elements (40 bytes each), fwd[R] and the cs text; OUT = the NM plans.
// Every record is planned on its own, from a private copy of its tag that ENDS where its heap block ends and starts at the
// tag's own alignment inside an 8-byte word: the sanitizer ends the program at the first byte read behind a tag.
int main(int argc, char **argv) {
    std::vector<int64_t> raw;
    if (argc != 3 || !emul_san::read_words(argv[1], raw) || raw.size() < 3) return 2;
    const int64_t R = raw[0], NM = raw[1], TB = raw[2];
    const int64_t *qs = raw.data() + 3, *qe = qs + R, *cs_off = qe + R, *main_off = cs_off + R + 1;
    const aasm_out_elem *el = (const aasm_out_elem *)(main_off + R + 1);
    const uint8_t *fwd = (const uint8_t *)(el + NM);
    const char *text = (const char *)fwd + R;
    if ((const char *)(raw.data() + raw.size()) < text + TB) return 2;
    std::vector<aasm_cut_plan> plans((size_t)NM + 1);
    for (int64_t r = 0; r < R; r++) {
        const int64_t len = cs_off[r + 1] - cs_off[r], mis = cs_off[r] & 7, n = main_off[r + 1] - main_off[r];
        if (n == 0) continue;
        char *block = emul_san::block<char>(mis + len);
        std::memcpy(block + mis, text + cs_off[r], (size_t)len);
        const int64_t rec_off[2] = {0, 1}, off[2] = {0, n}, zero[2] = {0, 0}, one_cs[2] = {mis, mis + len};
        aasm_batch_in in;
        std::memset(&in, 0, sizeof in);
        in.n_contigs = 1; in.n_records = 1; in.ctg_rec_off = rec_off; in.qry_str = qs + r; in.qry_end = qe + r; in.aln_fwd = fwd + r;
        in.cs_text = block; in.rec_cs_off = one_cs;
        aasm_dev_out o;
        std::memset(&o, 0, sizeof o);
        o.main_off = (int64_t *)off; o.alt_off = (int64_t *)zero; o.all_path_off = (int64_t *)zero; o.all_elem_off = (int64_t *)zero;
        o.main_elems = (aasm_out_elem *)el + main_off[r];
        const aasm_out_sizes sz{1, n, 0, 0, 0};
        const aasm_dev_cuts d{plans.data() + main_off[r], nullptr, nullptr};
        if (run(&in, &sz, &o, &d, 0) != AASM_OK) return 3;
        std::free(block);
    }
    return emul_san::write_bytes(argv[2], plans.data(), sizeof(aasm_cut_plan) * (size_t)NM) ? 0 : 2;
}
#endif
