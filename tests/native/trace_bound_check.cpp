// trace_bound_check.cpp - the host build of pyrecode_amd/csrc/rc_trace.h as a stand-alone program (tests/test_trace_cpu.py builds it, also
// under AddressSanitizer / UBSan, and compares its answers with the rule restated in Python integers, tests/trace_model.py).
// Reads cases from standard input, one per line, and answers each with one line:
//   f nx ny level d k n  bound_0 .. bound_{k-1}  bytes_0 .. bytes_{n-1}     -> 1 if the batch keeps to the no-wrap rule, else 0
//   c a vmax pixels                                                          -> 1 if a * vmax * pixels <= 2^63 - 1, else 0
//   p nx ny level d bytes                                                    -> the set pixels the frame can hold
//   a w                                                                      -> |w| of the int32 w as uint32
// Prints "ok" at the end; the exit status is 1 for a line it cannot read.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../pyrecode_amd/csrc/rc_trace.h"

int main()
{
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'f') {
            uint32_t nx, ny, level, d, k, n;
            if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &nx, &ny, &level, &d, &k, &n) != 6 || k > rc::TRACE_MAX_PLANES) return 1;
            std::vector<uint32_t> bound(k), sizes(3 * (size_t)n, 0u);
            for (uint32_t m = 0; m < k; ++m)
                if (scanf("%" SCNu32, &bound[m]) != 1) return 1;
            for (uint32_t f = 0; f < n; ++f)
                if (scanf("%" SCNu32, &sizes[3 * (size_t)f + 2]) != 1) return 1;
            printf("%d\n", rc::trace_batch_fits(nx, ny, level, d, k, bound.data(), sizes.data(), n) ? 1 : 0);
        } else if (kind == 'c') {
            uint64_t a, vmax, pixels;
            if (scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &a, &vmax, &pixels) != 3) return 1;
            printf("%d\n", rc::trace_column_fits(a, vmax, pixels) ? 1 : 0);
        } else if (kind == 'p') {
            uint32_t nx, ny, level, d, bytes;
            if (scanf("%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &nx, &ny, &level, &d, &bytes) != 5) return 1;
            printf("%" PRIu64 "\n", rc::trace_frame_pixels(nx, ny, level, d, bytes));
        } else if (kind == 'a') {
            int32_t w;
            if (scanf("%" SCNd32, &w) != 1) return 1;
            printf("%" PRIu32 "\n", rc::trace_abs(w));
        } else
            return 1;
    }
    printf("ok\n");
    return 0;
}
