// calib_select_check.cpp - the host build of pyrecode_amd/csrc/rc_calib.h as a stand-alone program (tests/test_calibration_cpu.py builds it
// with -fsanitize=address,undefined): every record of the input file is one column and one question; the answers go to stdout, one line
// per record, for the test to compare with numpy.  The program also checks every answer against std::sort itself and fails on a mismatch.
//   record: u32 n | u32 r (ascending rank of the pair) | u32 k (ranks from the top) | n x u16
//   line:   lo hi median2 std_bits top_defined top_bits
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../pyrecode_amd/csrc/rc_calib.h"

struct VecCol {
    const std::vector<uint16_t> *v;
    uint32_t operator()(uint32_t i) const { return v->at(i); }   // (bounds-checked: a rank loop that leaves the column ends the program)
};

static uint32_t bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t hdr[3], records = 0;
    while (fread(hdr, 4, 3, f) == 3) {
        const uint32_t n = hdr[0], r = hdr[1], k = hdr[2];
        std::vector<uint16_t> col(n);
        if (n == 0 || r >= n || fread(col.data(), 2, n, f) != n) { fprintf(stderr, "bad record %u\n", records); return 2; }
        const VecCol c{&col};
        uint32_t lo = 0, hi = 0;
        rc::calib_select_pair(c, n, r, lo, hi);
        const uint32_t m2 = rc::calib_median2(c, n);
        const float sd = rc::calib_std(c, n);
        float top = 65535.0f;
        const float med = 0.5f * (float)m2;
        const bool ok = rc::calib_top_pair(c, n, med, k, top);
        // the same answers from a sorted copy
        std::vector<uint16_t> s(col);
        std::sort(s.begin(), s.end());
        const uint32_t want_hi = s[std::min(r + 1, n - 1)];
        const uint32_t want_m2 = (n & 1u) ? 2u * s[n / 2] : (uint32_t)s[n / 2 - 1] + s[n / 2];
        uint32_t above = 0;
        for (uint16_t v : col) above += (float)v > med ? 1u : 0u;
        const bool want_ok = k >= 1 && above >= k + 1;
        if (lo != s[r] || hi != want_hi || m2 != want_m2 || ok != want_ok || (ok && top != ((float)s[n - k - 1] + (float)s[n - k]) / 2.0f)) {
            fprintf(stderr, "record %u (n %u r %u k %u): got %u %u %u %d\n", records, n, r, k, lo, hi, m2, (int)ok);
            return 1;
        }
        printf("%u %u %u %u %d %u\n", lo, hi, m2, bits(sd), (int)ok, bits(top));
        ++records;
    }
    fclose(f);
    printf("records %u ok\n", records);
    return 0;
}
