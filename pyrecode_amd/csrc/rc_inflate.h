// rc_inflate.h - the decoding core of the batched device inflate (rc_inflate.hip): what ONE lane does with one candidate block start of
// a zlib stream this library's device DEFLATE encoder wrote (rc_deflate_block.h: the binary map, rc_pix_deflate.hip: the residual stream).
// Plain C++ as well as HIP: the same functions are built into tests/native/inflate_chain_check.cpp and judged there, on the CPU, against
// stdlib zlib and the serial Python statement of the scheme (tests/inflate_chain_model.py).
//
// The streams' units (a 512-byte tile of the map, a 32 KiB chunk of the residual stream) all start on a byte, but where is known only by
// decoding the unit in front.  Every start, though, is offset 2, or follows the empty stored block 00 00 FF FF that closes a coded unit,
// or follows a full stored unit: those positions are CANDIDATES, every candidate is decoded on its own, and the real units are the
// candidates on the chain end -> candidate that starts at offset 2 (DESIGN.md "device inflate").  False candidates feed these
// functions arbitrary bytes by design, so:
//   - bits come through InfBits, whose loader answers 0 for any dword that does not overlap the stream;
//   - every step checks the bit position against `lim` (the stream's Adler-32 trailer) - each loop iteration consumes at least one bit;
//   - output positions are checked against the unit's size before they are used;
//   - the fixed code is decoded arithmetically; the tables of a dynamic block are indexed by masked bits and checked counters only.
// A candidate that fails any check is simply not a unit (false is not an error).  The Adler-32 is not checked.
#pragma once
#include <stdint.h>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define INF_HD __host__ __device__ __forceinline__
#else
#define INF_HD inline
#endif

namespace rc {

constexpr uint32_t INF_MAP_UNIT = 512u, INF_VAL_UNIT = 1u << 15;
constexpr uint32_t INF_NONE = 0xFFFFFFFFu;   // InfStream chain link: the candidate is no unit, or no candidate sits at its end
constexpr uint32_t INF_TERM = 0xFFFFFFFEu;   // ... its end is the stream's trailer
constexpr uint32_t INF_MAXBITS = 12;         // longest literal code of the subset (rc_deflate_model.h)
constexpr uint32_t INF_CAND_EXTRA = 64;      // a stream has room for 2 * units + INF_CAND_EXTRA candidates

// One zlib stream of a batch (host -> device).  Positions inside a stream are byte offsets from `src`.
struct InfStream {
    uint64_t src;            // its first byte in the batch's stored bytes
    uint64_t dst;            // where its first unit goes in the decoded-streams buffer (dword aligned)
    uint32_t csize, size;    // stored bytes, bytes it regenerates
    uint32_t unit;           // INF_MAP_UNIT or INF_VAL_UNIT
    uint32_t units;          // max(ceil(size / unit), 1)
    uint32_t cand0, cap;     // its rows of the candidate tables
    uint32_t unit0;          // its row of the unit table
    uint32_t pad;
};
inline uint32_t inf_units(uint64_t size, uint32_t unit) { return size ? (uint32_t)((size + unit - 1) / unit) : 1u; }

INF_HD uint32_t inf_rev(uint32_t v, uint32_t len)   // the low `len` (<= 16) bits of v, reversed
{
    v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
    v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
    v = ((v & 0x0F0Fu) << 4) | ((v >> 4) & 0x0F0Fu);
    v = ((v & 0x00FFu) << 8) | ((v >> 8) & 0x00FFu);
    return v >> (16u - len);
}

// p is a candidate block start of a stream of csize bytes with units of U bytes; at(q): the stream's byte q (asked for 0 <= q < csize only)
template <class At>
INF_HD bool inf_is_candidate(At at, uint32_t p, uint32_t csize, uint32_t U)
{
    if (p < 2 || csize < 6 || p >= csize - 4) return false;
    if (p == 2) return true;
    if (p >= 6 && at(p - 1) == 0xFF && at(p - 2) == 0xFF && at(p - 3) == 0 && at(p - 4) == 0) return true;
    const uint32_t H = 5 + U;
    return p >= 2 + H && at(p - H) == 0 && at(p - H + 1) == (U & 255) && at(p - H + 2) == (U >> 8) && at(p - H + 3) == (~U & 255) && at(p - H + 4) == ((~U >> 8) & 255);
}

// The stream as dwords from the aligned address at or below its first byte: ld(w) = dword w, 0 when it does not overlap the stream
// (a dword that does may hold up to 3 bytes from either side of it: inside the batch in front, inside the 15 bytes the reader guarantees behind).
struct InfGlobalLoad {
    const uint32_t *base;
    uint32_t nwords;
    INF_HD uint32_t operator()(uint32_t w) const { return w < nwords ? base[w] : 0u; }
};
// 32 bits at any bit position (positions count from the loader's dword 0); the two dwords under the last position are kept
template <class Load>
struct InfBits {
    Load ld;
    uint32_t w, lo, hi;
    INF_HD explicit InfBits(Load l) : ld(l), w(0x80000000u), lo(0), hi(0) {}
    INF_HD uint32_t peek(uint32_t pos)
    {
        const uint32_t ww = pos >> 5;
        if (ww != w) {
            lo = ww == w + 1 ? hi : ld(ww);
            hi = ld(ww + 1);
            w = ww;
        }
        return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (pos & 31u));
    }
};

// behind a coded unit's end-of-block code: the last unit is padded to the byte, any other is followed by the empty stored block
template <class Bits>
INF_HD bool inf_close(Bits &b, uint32_t &pos, uint32_t lim, uint32_t bfinal)
{
    if (!bfinal) {
        if (b.peek(pos) & 7u) return false;
        pos = (pos + 3u + 7u) & ~7u;
        if (pos + 32u > lim || b.peek(pos) != 0xFFFF0000u) return false;
        pos += 32u;
    } else
        pos = (pos + 7u) & ~7u;
    return pos <= lim;
}

// a stored block at pos (a byte boundary): its data bits start at the returned pos
template <class Bits>
INF_HD bool inf_stored_header(Bits &b, uint32_t &pos, uint32_t lim, uint32_t U, uint32_t &len, uint32_t &bfinal)
{
    const uint32_t h = b.peek(pos) & 0xFFu;
    if (h > 1u || pos + 40u > lim) return false;     // (the encoder's padding bits are zero)
    bfinal = h;
    const uint32_t v = b.peek(pos + 8u);
    len = v & 0xFFFFu;
    if ((len ^ (v >> 16)) != 0xFFFFu || len > U) return false;
    pos += 40u;
    return pos + 8u * len <= lim;
}

// One unit of a binary-map stream at pos: a stored block, or a fixed-Huffman block whose matches stay inside the unit, and what closes
// it.  STORE: the bytes go to out.put(i, byte) in order, matches read out.get(i) back; otherwise they are only counted.  On success pos
// is the next unit's start.
template <bool STORE, class Bits, class Out>
INF_HD bool inf_map_unit(Bits &b, uint32_t &pos, uint32_t lim, Out &out, uint32_t &regen, uint32_t &bfinal)
{
    uint32_t v = b.peek(pos), n = 0;
    const uint32_t btype = (v >> 1) & 3u;
    if (btype == 0u) {
        if (!inf_stored_header(b, pos, lim, INF_MAP_UNIT, regen, bfinal)) return false;
        if (STORE)
            for (uint32_t i = 0; i < regen; ++i) out.put(i, b.peek(pos + 8u * i) & 0xFFu);
        pos += 8u * regen;
        return true;
    }
    if (btype != 1u) return false;
    bfinal = v & 1u;
    pos += 3u;
    for (;;) {
        if (pos > lim) return false;
        v = b.peek(pos);
        uint32_t sym, l = 8u;
        const uint32_t r8 = inf_rev(v & 255u, 8);
        if (r8 < 0x30u) { sym = 256u + (r8 >> 1); l = 7u; }
        else if (r8 < 0xC0u) sym = r8 - 0x30u;
        else if (r8 < 0xC8u) sym = 280u + r8 - 0xC0u;
        else { sym = 144u + ((r8 << 1) | ((v >> 8) & 1u)) - 0x190u; l = 9u; }
        pos += l;
        if (sym < 256u) {
            if (n >= INF_MAP_UNIT) return false;
            if (STORE) out.put(n, sym);
            ++n;
            continue;
        }
        if (sym == 256u) break;
        if (sym > 285u) return false;
        v = b.peek(pos);                    // <= 5 + 5 + 13 bits follow
        uint32_t len, e = 0;
        if (sym < 265u) len = sym - 254u;
        else if (sym == 285u) len = 258u;
        else {
            e = (sym - 261u) >> 2;
            len = 3u + ((4u + ((sym - 261u) & 3u)) << e) + (v & ((1u << e) - 1u));
        }
        v >>= e;
        const uint32_t ds = inf_rev(v & 31u, 5);
        v >>= 5;
        if (ds > 29u) return false;
        uint32_t dist = ds + 1u, de = 0;
        if (ds >= 4u) {
            de = (ds >> 1) - 1u;
            dist = 1u + ((2u + (ds & 1u)) << de) + (v & ((1u << de) - 1u));
        }
        pos += e + 5u + de;
        if (dist > n || n + len > INF_MAP_UNIT) return false;
        if (STORE)
            for (uint32_t i = 0; i < len; ++i) out.put(n + i, out.get(n + i - dist));
        n += len;
    }
    regen = n;
    return pos <= lim && inf_close(b, pos, lim, bfinal);
}

// ---- a literals-only dynamic-Huffman block (the residual stream's coded chunk) -----------------------------------------------------
// What one decoder needs besides the bits (LDS on the device)
struct InfDyn {
    uint16_t tab[1u << INF_MAXBITS];   // the next 12 bits -> symbol | length << 9; 0: no code
    uint8_t lens[264];                 // the 258 code lengths of the header
    uint8_t cl_sym[20];                // the code-length code's symbols sorted by (length, symbol)
    uint16_t cl_cnt[8];                // ... and how many there are of every length
    uint16_t cnt[16], nxt[16];
};
constexpr uint32_t INF_DYN_HEADER_BITS = 17u + 19u * 3u + 258u * 14u;   // no header is longer

// the header of a dynamic block at pos (BTYPE checked by the caller) -> D.tab; pos: the first literal.  The subset: HLIT 0, HDIST 0 (257
// literal / end-of-block codes, one distance code), a complete code-length code, literal codes of <= 12 bits that are not over-subscribed.
template <class Bits>
INF_HD bool inf_dyn_header(Bits &b, uint32_t &pos, uint32_t lim, InfDyn &D, uint32_t &bfinal)
{
    uint32_t v = b.peek(pos);
    bfinal = v & 1u;
    if (((v >> 3) & 0x3FFu) != 0u) return false;
    const uint32_t hclen = ((v >> 13) & 15u) + 4u;
    pos += 17u;
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint64_t cl = 0;                      // 19 lengths of 3 bits, by symbol
    for (uint32_t i = 0; i < 8; ++i) D.cl_cnt[i] = 0;
    for (uint32_t i = 0; i < hclen; ++i) {
        const uint32_t l = b.peek(pos) & 7u;
        pos += 3u;
        cl |= (uint64_t)l << (3u * order[i]);
        ++D.cl_cnt[l];
    }
    if (pos > lim) return false;
    int32_t left = 1;
    for (uint32_t l = 1; l < 8; ++l) {
        left = 2 * left - (int32_t)D.cl_cnt[l];
        if (left < 0) return false;
    }
    if (left != 0) return false;
    uint32_t k = 0;
    for (uint32_t l = 1; l < 8; ++l)
        for (uint32_t s = 0; s < 19; ++s)
            if (((cl >> (3u * s)) & 7u) == l) D.cl_sym[k++] = (uint8_t)s;     // (k <= 19)
    uint32_t i = 0;
    while (i < 258u) {
        if (pos > lim) return false;
        v = b.peek(pos);
        uint32_t code = 0, first = 0, index = 0, sym = 19u, l = 1;
        for (; l < 8u; ++l) {
            code |= (v >> (l - 1u)) & 1u;
            const uint32_t c = D.cl_cnt[l];
            if (code - first < c) { sym = D.cl_sym[index + code - first]; break; }   // (index + code - first < index + c <= 19)
            index += c;
            first = (first + c) << 1;
            code <<= 1;
        }
        if (sym > 18u) return false;
        pos += l;
        v >>= l;
        if (sym < 16u) { D.lens[i++] = (uint8_t)sym; continue; }
        uint32_t rep, val = 0;
        if (sym == 16u) {
            if (i == 0) return false;
            val = D.lens[i - 1];
            rep = 3u + (v & 3u); pos += 2u;
        } else if (sym == 17u) { rep = 3u + (v & 7u); pos += 3u; }
        else { rep = 11u + (v & 127u); pos += 7u; }
        if (i + rep > 258u) return false;
        for (uint32_t j = 0; j < rep; ++j) D.lens[i++] = (uint8_t)val;
    }
    if (pos > lim) return false;
    for (uint32_t l = 0; l < 16; ++l) D.cnt[l] = 0;
    for (uint32_t s = 0; s < 257u; ++s) {
        if (D.lens[s] > INF_MAXBITS) return false;
        ++D.cnt[D.lens[s]];
    }
    if (D.lens[256] == 0) return false;
    uint32_t kraft = 0, c = 0;
    D.cnt[0] = 0;
    for (uint32_t l = 1; l <= INF_MAXBITS; ++l) {
        kraft += (uint32_t)D.cnt[l] << (INF_MAXBITS - l);
        c = (c + D.cnt[l - 1]) << 1;
        D.nxt[l] = (uint16_t)c;
    }
    if (kraft > (1u << INF_MAXBITS)) return false;
    for (uint32_t t = 0; t < (1u << INF_MAXBITS); ++t) D.tab[t] = 0;
    for (uint32_t s = 0; s < 257u; ++s) {
        const uint32_t l = D.lens[s];
        if (!l) continue;
        const uint32_t r = inf_rev(D.nxt[l]++, l);     // (not over-subscribed: the code is below 2^l)
        for (uint32_t t = r; t < (1u << INF_MAXBITS); t += 1u << l) D.tab[t] = (uint16_t)(s | (l << 9));
    }
    return true;
}

enum { INF_FAIL = 0, INF_DONE = 1, INF_MORE = 2 };
// literals from pos on, while pos < stop (the bits the caller has staged) and n < n_stop (the room of its output stage); the block holds at
// most nmax of them.  put(n, byte) takes literal n.  INF_DONE: the end-of-block code was read.
template <class Bits, class Put>
INF_HD int inf_literals(Bits &b, uint32_t &pos, uint32_t stop, uint32_t lim, const InfDyn &D, uint32_t &n, uint32_t n_stop, uint32_t nmax, Put put)
{
    while (pos < stop && n < n_stop) {
        const uint32_t e = D.tab[b.peek(pos) & ((1u << INF_MAXBITS) - 1u)];
        if (!e) return INF_FAIL;
        pos += e >> 9;
        if (pos > lim) return INF_FAIL;
        const uint32_t s = e & 511u;
        if (s == 256u) return INF_DONE;
        if (n >= nmax) return INF_FAIL;
        put(n, s);
        ++n;
    }
    return INF_MORE;
}

}  // namespace rc
