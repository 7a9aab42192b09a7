// tests/host_emul/emul_launch.h -- TEST INFRASTRUCTURE ONLY: a launch of a row of any kernel table (aasm_dev.h) on the host.
#pragma once
#include <cstring>
#include <vector>

#include "../../alignasm_amd/csrc/aasm_dev.h"

namespace aasm {

// what a launch needs of a row; AASM_EMUL_ROWS(name, TABLE): the rows of a table, by id
struct EmulRow { int lanes; size_t lds; };
#define AASM_EMUL_ROW(id, sym, block, lanes, ...) {lanes, 0},
#define AASM_EMUL_ROWL(id, sym, block, lanes, lds, ...) {lanes, lds},
#define AASM_EMUL_ROWS(name, TABLE) constexpr EmulRow name[] = {TABLE(AASM_EMUL_ROW, AASM_EMUL_ROWL)}

// Row `id` for the work items [g0, g0 + n), a block each: the blocks one after the other, in each the row's lanes (of a block of
// nthreads threads) one after the other.  max_blocks > 0 caps the grid (fewer blocks than items: the bodies' grid-stride loops).
// Every block starts from LDS of the row's size poisoned with 0xA5, which catches reads of never-written cells.
// body(k): the row's body for thread k, through the table's dispatcher.
template <size_t N, class Body>
void emul_launch(const EmulRow (&rows)[N], int id, int nthreads, int64_t g0, int64_t n, int64_t max_blocks, Body body) {
    const int lanes = emul_lanes(nthreads, rows[id].lanes);
    if (max_blocks > 0 && n > max_blocks) n = max_blocks;
    std::vector<char> lds(rows[id].lds);                            // (heap memory: aligned for any type)
    for (int64_t b = g0; b < g0 + n; b++) {
        if (!lds.empty()) memset(lds.data(), 0xA5, lds.size());
        for (int t = 0; t < lanes; t++) body(KCtx{t, lanes, b, n, 0, lds.empty() ? nullptr : lds.data()});
    }
}

}  // namespace aasm
