// The decoding core of the batched device inflate (pyrecode_amd/csrc/rc_inflate.h) on the CPU, put together the way rc_inflate.hip puts
// it together on the device: candidates -> every candidate sized on its own -> chain -> the units decoded again to their place.
//   as a shared library (tests/test_inflate_chain_cpu.py): inflate_chain_check() on the catalogue of tests/inflate_chain_model.py;
//   as a program (-DINFLATE_CHECK_MAIN, meant for -fsanitize=address,undefined): reads records [kind][csize][size][bytes] from a file,
//   checks each against the size it names, then feeds the core damaged copies of every record and random bytes - the contract of
//   rc_inflate.h is that ARBITRARY bytes neither read outside the stream's dwords nor write outside the unit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../pyrecode_amd/csrc/rc_inflate.h"

using namespace rc;

namespace {
struct VecOut {
    std::vector<uint8_t> &v;
    size_t base;
    void put(uint32_t i, uint32_t byte) { v.at(base + i) = (uint8_t)byte; }
    uint32_t get(uint32_t i) { return v.at(base + i); }
};
struct NoOut {
    void put(uint32_t, uint32_t) {}
    uint32_t get(uint32_t) { return 0; }
};

// one candidate of a value stream; out: nullptr = size it only
bool val_unit(InfBits<InfGlobalLoad> &b, uint32_t &pos, uint32_t lim, uint32_t nmax, std::vector<uint8_t> *out, size_t base, uint32_t &regen, uint32_t &bfinal)
{
    static InfDyn D;
    const uint32_t btype = (b.peek(pos) >> 1) & 3u;
    if (btype == 0u) {
        if (!inf_stored_header(b, pos, lim, INF_VAL_UNIT, regen, bfinal)) return false;
        if (out && regen <= nmax)
            for (uint32_t i = 0; i < regen; ++i) out->at(base + i) = (uint8_t)b.peek(pos + 8u * i);
        pos += 8u * regen;
        return true;
    }
    if (btype != 2u) return false;
    if (!inf_dyn_header(b, pos, lim < pos + INF_DYN_HEADER_BITS ? lim : pos + INF_DYN_HEADER_BITS, D, bfinal)) return false;
    uint32_t n = 0;
    const int r = inf_literals(b, pos, 0xFFFFFFFFu, lim, D, n, nmax + 1u, nmax, [&](uint32_t at, uint32_t byte) { if (out) out->at(base + at) = (uint8_t)byte; });
    regen = n;
    return r == INF_DONE && inf_close(b, pos, lim, bfinal);
}
}  // namespace

// 0: out holds the stream's `size` bytes; -2: refused.  misalign (0..3): where the stream starts relative to a dword.
extern "C" int inflate_chain_check(const uint8_t *stream, uint32_t csize, uint32_t size, uint32_t kind, uint32_t misalign, uint8_t *out,
                                   uint32_t *units_out, uint32_t *ncand_out)
{
    if (csize < 8 || stream[0] != 0x78 || stream[1] != 0x01 || ((stream[2] & 6u) != 0u && (stream[2] & 6u) != (kind ? 4u : 2u))) return -2;
    const uint32_t U = kind ? INF_VAL_UNIT : INF_MAP_UNIT, units = inf_units(size, U), off = misalign & 3u;
    // exactly the dwords that overlap the stream: a read outside them is a heap overflow
    const uint32_t nwords = (csize + off + 3u) >> 2;
    std::vector<uint32_t> buf(nwords, 0xA5A5A5A5u);
    memcpy(reinterpret_cast<uint8_t *>(buf.data()) + off, stream, csize);
    const InfGlobalLoad gl{buf.data(), nwords};
    const uint32_t lim = 8u * (csize - 4u + off);
    std::vector<uint32_t> cand;
    for (uint32_t p = 0; p < csize; ++p)
        if (inf_is_candidate([&](uint32_t q) { if (q >= csize) abort(); return (uint32_t)stream[q]; }, p, csize, U)) cand.push_back(p);
    if (ncand_out) *ncand_out = (uint32_t)cand.size();
    if (cand.size() > 2u * units + INF_CAND_EXTRA) return -2;
    std::vector<uint32_t> link(cand.size(), INF_NONE);
    for (size_t c = 0; c < cand.size(); ++c) {
        InfBits<InfGlobalLoad> bits(gl);
        uint32_t pos = 8u * (cand[c] + off), regen = 0, bfinal = 0;
        NoOut none;
        const bool ok = kind ? val_unit(bits, pos, lim, U, nullptr, 0, regen, bfinal) : inf_map_unit<false>(bits, pos, lim, none, regen, bfinal);
        if (!ok) continue;
        const uint32_t end = (pos >> 3) - off;
        if (end == csize - 4u) { link[c] = INF_TERM; continue; }
        for (size_t j = c + 1; j < cand.size(); ++j)
            if (cand[j] == end) link[c] = (uint32_t)j;
    }
    std::vector<uint32_t> unit_cand;
    for (uint32_t c = 0;;) {
        if (cand.empty() || unit_cand.size() >= units) return -2;
        unit_cand.push_back(c);
        if (link[c] == INF_TERM) break;
        if (link[c] == INF_NONE || link[c] <= c) return -2;
        c = link[c];
    }
    if (unit_cand.size() != units) return -2;
    std::vector<uint8_t> dst((size_t)units * U, 0);
    for (uint32_t k = 0; k < units; ++k) {
        const uint32_t want = size > k * U ? (size - k * U < U ? size - k * U : U) : 0u;
        InfBits<InfGlobalLoad> bits(gl);
        uint32_t pos = 8u * (cand[unit_cand[k]] + off), regen = 0, bfinal = 0;
        VecOut vo{dst, (size_t)k * U};
        const bool ok = kind ? val_unit(bits, pos, lim, want, &dst, (size_t)k * U, regen, bfinal) : inf_map_unit<true>(bits, pos, lim, vo, regen, bfinal);
        if (!ok || regen != want || bfinal != (k + 1 == units ? 1u : 0u)) return -2;
    }
    if (out && size) memcpy(out, dst.data(), size);
    if (units_out) *units_out = units;
    return 0;
}

#ifdef INFLATE_CHECK_MAIN
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t hdr[3], seed = 12345u, nrec = 0, ndamaged = 0, naccepted = 0;
    auto rnd = [&] { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    std::vector<uint8_t> s, out;
    while (fread(hdr, 4, 3, f) == 3) {
        s.resize(hdr[1]);
        if (fread(s.data(), 1, s.size(), f) != s.size()) return 2;
        out.assign((size_t)hdr[2] + 1, 0);
        for (uint32_t mis = 0; mis < 4; ++mis)
            if (inflate_chain_check(s.data(), hdr[1], hdr[2], hdr[0], mis, out.data(), nullptr, nullptr) != 0) { fprintf(stderr, "record %u refused\n", nrec); return 1; }
        ++nrec;
        for (uint32_t t = 0; t < 48; ++t) {        // damaged copies: flipped bits, bytes overwritten by markers and stored headers, cut short
            std::vector<uint8_t> d(s);
            const uint32_t what = t % 4;
            for (uint32_t j = 0; j <= t % 3; ++j) {
                const uint32_t at = rnd() % (uint32_t)d.size();
                if (what == 0) d[at] ^= (uint8_t)(1u << (rnd() & 7u));
                else if (what == 1 && at + 4 <= d.size()) memcpy(&d[at], "\x00\x00\xff\xff", 4);
                else if (what == 2 && at + 5 <= d.size()) { const uint32_t n = rnd() & 0xFFFFu; d[at] = 0; d[at + 1] = n & 255; d[at + 2] = n >> 8; d[at + 3] = ~n & 255; d[at + 4] = (~n >> 8) & 255; }
            }
            if (what == 3) d.resize(8 + rnd() % (uint32_t)(d.size() - 7));
            ++ndamaged;
            naccepted += inflate_chain_check(d.data(), (uint32_t)d.size(), hdr[2], hdr[0], t & 3u, out.data(), nullptr, nullptr) == 0;
        }
    }
    fclose(f);
    for (uint32_t t = 0; t < 400; ++t) {           // random bytes under a good header, sprinkled with markers
        std::vector<uint8_t> d(16 + rnd() % 3000u);
        for (auto &b : d) b = (uint8_t)rnd();
        d[0] = 0x78; d[1] = 0x01; d[2] = (uint8_t)((d[2] & ~6u) | ((t & 1u) ? ((t & 2u) ? 4u : 2u) : 0u));
        for (uint32_t j = 0; j < 6; ++j) { const uint32_t at = 3 + rnd() % (uint32_t)(d.size() - 8); memcpy(&d[at], "\x00\x00\xff\xff", 4); if (j & 1) d[at + 4] = (uint8_t)((t & 2u) ? 4u : 2u); }
        out.assign(70000, 0);
        ++ndamaged;
        naccepted += inflate_chain_check(d.data(), (uint32_t)d.size(), 1 + rnd() % 60000u, (t >> 1) & 1u, t & 3u, out.data(), nullptr, nullptr) == 0;
    }
    printf("records %u ok, damaged / random inputs %u (accepted %u)\n", nrec, ndamaged, naccepted);
    return 0;
}
#endif
