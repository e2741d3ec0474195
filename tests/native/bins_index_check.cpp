// bins_index_check.cpp - the host build of pyrecode_amd/csrc/rc_bins.h as a stand-alone program (tests/test_bins_cpu.py builds it, also
// under AddressSanitizer / UBSan, and compares its answers with the arithmetic restated in Python integers, tests/bins_model.py), and the
// row of rc_read_plan.h that the bins kind adds.
// Reads cases from standard input, one per line, and answers each with one line:
//   t B level                             -> the histogram's tier, its LDS bytes, the workgroups a launch aims for
//   w nb8 n B                             -> blocks a workgroup walks, workgroups per frame, bytes of the partial rows
//   k                                     -> RK_BINS' row: esz coo stats counts sums cells held | its synchronous route | late(plain) late(inflate)
//                                            | segments, offset and bytes of a 1000-byte output's copy-back at totals 0 and 7 | the message
//                                            names rc_bins_frames_submit | RK_BINS - RK_CORR, RK_ALL - RK_BINS, RK_KINDS - RK_TRACE
// Prints "ok" at the end; the exit status is 1 for a line it cannot read.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../pyrecode_amd/csrc/rc_bins.h"
#include "../../pyrecode_amd/csrc/rc_read_plan.h"

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
        } else if (kind == 'k') {
            const rc::ReadKindInfo i = rc::read_kind_info(rc::RK_BINS);
            const rc::CopyPlan p0 = rc::read_copy_plan(rc::RK_BINS, 7, 0, 1000), p7 = rc::read_copy_plan(rc::RK_BINS, 7, 7, 1000);
            printf("%u %u %d %d %d %d %d | %u | %d %d | %u %" PRIu64 " %" PRIu64 " %u %" PRIu64 " %" PRIu64 " | %d | %d %d %d\n", i.esz, i.coo, i.stats, i.counts,
                   i.sums, i.cells, i.held, (unsigned)rc::verdict_route_sync(i), rc::read_copy_is_late(rc::RK_BINS, false), rc::read_copy_is_late(rc::RK_BINS, true),
                   p0.nseg, p0.seg[0].off, p0.seg[0].bytes, p7.nseg, p7.seg[0].off, p7.seg[0].bytes, i.pageable && strstr(i.pageable, "rc_bins_frames_submit") ? 1 : 0,
                   (int)rc::RK_BINS - (int)rc::RK_CORR, (int)rc::RK_ALL - (int)rc::RK_BINS, (int)rc::RK_KINDS - (int)rc::RK_TRACE);
        } else
            return 1;
    }
    printf("ok\n");
    return 0;
}
