// rc_deflate_model.h - HOST side of the device DEFLATE encoder's residual stream at compression_level >= 2: one Huffman table per ctx,
// fitted to a byte histogram of a sample, in the form the kernel uses (bit-reversed codes) and the form a dynamic block carries (its
// header bit string).  Serial statement of the whole stream: tests/deflate_values_model.py; kernels: rc_pix_deflate.hip.
//
// The reference runs zlib.compress(packed_residuals, level) (recode_writer.py:507-511 -> recode_compressors.py:84-85).  The packed stream
// has no repeats worth finding, so a literals-only dynamic-Huffman block (RFC 1951 BTYPE 10) per 32 KiB chunk is the whole gain:
//   - 257 symbols (256 literals + end-of-block), every one with a code of at most 12 bits, so that frames unlike the sample still encode
//     and a `code | len << 12` entry fits 16 bits;
//   - the distance alphabet is the single zero-length code RFC 1951 3.2.7 allows for literal-only data (stock zlib accepts it:
//     tests/test_deflate_values_cpu.py);
//   - the 258 code lengths are written with the code-length symbols 0..15 and 16 (repeat the previous length 3..6 times); no literal has
//     length zero, so 17 / 18 never apply.  The code-length code is fitted with the same routine (19 symbols, 7 bits) and HCLEN is always 15.
// Plain C++ (no HIP): built into librecode_hip.so for the ctx and into tests/native/deflate_model_check.cpp.
#pragma once
#include <stdint.h>
#include <string.h>

#include "rc_zstd_model.h"

namespace rc {

constexpr int DM_SYMS = 257, DM_EOB = 256, DM_MAXBITS = 12, DM_CL_MAXBITS = 7;
constexpr int DM_HDR_WORDS = 96;   // 17 + 57 + at most 258 * 9 bits of lengths = 2396 bits

struct DeflateModel {
    uint16_t code[DM_SYMS + 3];    // bit-reversed code | len << 12 (the kernel ORs LSB-first); [256] = end of block
    uint32_t usable;               // 0: the fitted code would not shrink the sample, the ctx keeps stored blocks
    uint32_t hdr_bits;             // bits of a coded block in front of its first literal
    uint32_t hdr[DM_HDR_WORDS];    // ... LSB-first, BFINAL clear
};

// RFC 1951 3.2.2: canonical code values (as read MSB-first) from lengths; zero lengths get no code
inline void dm_canonical(const uint8_t *len, int nsym, int maxbits, uint16_t *code)
{
    uint32_t count[17] = {0}, next[17] = {0};
    for (int s = 0; s < nsym; ++s) if (len[s]) count[len[s]]++;
    uint32_t c = 0;
    for (int b = 1; b <= maxbits; ++b) { c = (c + count[b - 1]) << 1; next[b] = c; }
    for (int s = 0; s < nsym; ++s) code[s] = len[s] ? (uint16_t)next[len[s]]++ : (uint16_t)0;
}
inline uint32_t dm_reverse(uint32_t v, int nbits)
{
    uint32_t r = 0;
    for (int i = 0; i < nbits; ++i) r |= ((v >> i) & 1u) << (nbits - 1 - i);
    return r;
}

// hist: the sample's 256 byte counts (the end-of-block count is derived: one per 32 KiB).  Fills lengths (optional), codes, header, usable.
inline void dm_build_model(const uint32_t *hist256, DeflateModel *M, uint8_t *len_out = nullptr)
{
    memset(M, 0, sizeof *M);
    uint32_t hist[DM_SYMS];
    uint64_t total = 0;
    for (int v = 0; v < 256; ++v) { hist[v] = hist256[v]; total += hist256[v]; }
    hist[DM_EOB] = (uint32_t)((total >> 15) ? (total >> 15) : 1);
    uint8_t len[DM_SYMS];
    zm_huf_lengths_n(hist, len, DM_SYMS, DM_MAXBITS);
    if (len_out) memcpy(len_out, len, DM_SYMS);
    uint16_t code[DM_SYMS];
    dm_canonical(len, DM_SYMS, DM_MAXBITS, code);
    for (int s = 0; s < DM_SYMS; ++s) M->code[s] = (uint16_t)(dm_reverse(code[s], len[s]) | ((uint32_t)len[s] << 12));
    M->usable = zm_code_pays(hist256, M->code) ? 1u : 0u;
    // the lengths as code-length symbols
    struct Sym { uint8_t s, extra; };
    Sym syms[DM_SYMS + 1];
    int ns = 0;
    uint8_t seq[DM_SYMS + 1];
    memcpy(seq, len, DM_SYMS);
    seq[DM_SYMS] = 0;   // the one distance code, of length zero
    for (int i = 0; i < DM_SYMS + 1;) {
        const uint8_t v = seq[i++];
        syms[ns++] = {v, 0};
        int run = 0;
        while (i + run < DM_SYMS + 1 && seq[i + run] == v) ++run;
        while (run >= 3) {
            const int r = run < 6 ? run : 6;
            syms[ns++] = {16, (uint8_t)(r - 3)};
            run -= r; i += r;
        }
    }
    uint32_t clhist[19] = {0};
    for (int i = 0; i < ns; ++i) clhist[syms[i].s]++;
    uint8_t cl_len[19];
    uint16_t cl_code[19];
    zm_huf_lengths_n(clhist, cl_len, 19, DM_CL_MAXBITS);
    dm_canonical(cl_len, 19, DM_CL_MAXBITS, cl_code);
    ZmBits w(reinterpret_cast<uint8_t *>(M->hdr), sizeof M->hdr);
    w.add(0, 1); w.add(2, 2);                 // BFINAL (set by the kernel), BTYPE 10
    w.add(0, 5); w.add(0, 5); w.add(15, 4);   // HLIT 257, HDIST 1, HCLEN 19
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int i = 0; i < 19; ++i) w.add(cl_len[order[i]], 3);
    for (int i = 0; i < ns; ++i) {
        w.add(dm_reverse(cl_code[syms[i].s], cl_len[syms[i].s]), cl_len[syms[i].s]);
        if (syms[i].s == 16) w.add(syms[i].extra, 2);
    }
    M->hdr_bits = w.n;
    if (!w.ok) M->usable = 0;   // (cannot happen: DM_HDR_WORDS holds the longest header)
}

}  // namespace rc
