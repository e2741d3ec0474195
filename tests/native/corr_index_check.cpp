// corr_index_check.cpp - the host build of pyrecode_amd/csrc/rc_corr.h as a stand-alone program (tests/test_corr_cpu.py builds it, also
// under AddressSanitizer / UBSan, and compares its answers with the arithmetic restated in Python integers, tests/corr_model.py).
// Reads cases from standard input, one per line, and answers each with one line:
//   s R                                   -> side, cells, accumulators a lane keeps
//   g nx ny R row col cell                -> cells of the padded reference, the window's base, the cell's offset
//   w nb8 n R                             -> blocks a workgroup walks, workgroups per frame, bytes of the partial rows
//   b nx ny level d bound n bytes_0 ..    -> 1 if the batch keeps to the no-wrap rule, else 0
// Prints "ok" at the end; the exit status is 1 for a line it cannot read.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../pyrecode_amd/csrc/rc_corr.h"

int main()
{
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 's') {
            uint32_t R;
            if (scanf("%" SCNu32, &R) != 1 || R > rc::CORR_MAX_RADIUS) return 1;
            printf("%" PRIu32 " %" PRIu32 " %" PRIu32 "\n", rc::corr_side(R), rc::corr_cells(R), rc::corr_lane_cells(R));
        } else if (kind == 'g') {
            uint32_t nx, ny, R, row, col, cell;
            if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &nx, &ny, &R, &row, &col, &cell) != 6) return 1;
            printf("%" PRIu64 " %" PRIu64 " %" PRIu32 "\n", rc::corr_padded_cells(nx, ny, R), rc::corr_window_base(row, col, nx, R), rc::corr_cell_offset(cell, nx, R));
        } else if (kind == 'w') {
            uint64_t nb8;
            uint32_t n, R;
            if (scanf("%" SCNu64 " %" SCNu32 " %" SCNu32, &nb8, &n, &R) != 3 || n == 0) return 1;
            const uint32_t nblk = (uint32_t)((nb8 + 255) / 256);
            printf("%" PRIu32 " %" PRIu32 " %" PRIu64 "\n", rc::corr_blocks_per_chunk(nblk, n), rc::corr_chunks(nblk, n), rc::corr_workspace_bytes(nb8, n, R));
        } else if (kind == 'b') {
            uint32_t nx, ny, level, d, bound, n;
            if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &nx, &ny, &level, &d, &bound, &n) != 6) return 1;
            std::vector<uint32_t> sizes(3 * (size_t)n, 0u);
            for (uint32_t f = 0; f < n; ++f)
                if (scanf("%" SCNu32, &sizes[3 * (size_t)f + 2]) != 1) return 1;
            printf("%d\n", rc::corr_batch_fits(nx, ny, level, d, bound, sizes.data(), n) ? 1 : 0);
        } else
            return 1;
    }
    printf("ok\n");
    return 0;
}
