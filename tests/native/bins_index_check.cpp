// bins_index_check.cpp - the host build of pyrecode_amd/csrc/rc_bins.h as a stand-alone program (tests/test_bins_cpu.py builds it, also
// under AddressSanitizer / UBSan, and compares its answers with the arithmetic restated in Python integers, tests/bins_model.py).
// Reads cases from standard input, one per line, and answers each with one line:
//   t B level                             -> the histogram's tier, its LDS bytes, the workgroups a launch aims for
//   w nb8 n B                             -> blocks a workgroup walks, workgroups per frame, bytes of the partial rows
// Prints "ok" at the end; the exit status is 1 for a line it cannot read.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../pyrecode_amd/csrc/rc_bins.h"

int main()
{
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 't') {
            uint32_t B, level;
            if (scanf("%" SCNu32 " %" SCNu32, &B, &level) != 2 || B == 0 || B > rc::BINS_MAX) return 1;
            printf("%" PRIu32 " %" PRIu32 " %" PRIu32 "\n", rc::bins_tier(B), rc::bins_lds_bytes(B, level), rc::bins_target_wgs(B));
        } else if (kind == 'w') {
            uint64_t nb8;
            uint32_t n, B;
            if (scanf("%" SCNu64 " %" SCNu32 " %" SCNu32, &nb8, &n, &B) != 3 || n == 0 || B == 0 || B > rc::BINS_MAX) return 1;
            const uint32_t nblk = (uint32_t)((nb8 + 255) / 256);
            printf("%" PRIu32 " %" PRIu32 " %" PRIu64 "\n", rc::bins_blocks_per_chunk(nblk, n, B), rc::bins_chunks(nblk, n, B), rc::bins_workspace_bytes(nb8, n, B));
        } else
            return 1;
    }
    printf("ok\n");
    return 0;
}
