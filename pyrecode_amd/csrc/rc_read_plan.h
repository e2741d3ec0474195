// rc_read_plan.h - the parts of the batched reader (rc_reader.hip) that hold no HIP call: what a result kind means for the expand kernels,
// the verdict a finished batch gets from its error word, and how a staged output goes back to the caller.  Plain C++:
// tests/native/read_plan_check.cpp walks all of it against tables written out by hand (tests/test_read_plan_cpu.py).
// A new result kind fills in: a row of read_kind_info, its synchronous route (verdict_route_sync), its segments (read_copy_plan) - and a
// hand-written row in each of read_plan_check.cpp's tables, which walk every kind up to RK_KINDS.
#pragma once
#include <stdint.h>
#include "../../include/recode_hip.h"

namespace rc {
// triplets, COO with uint16 / uint32 values, level-2 rows / columns + statistics, events (rc_count_frames), the adds into an rc_sum handle
// (frames' values; one count per event), cells of a region (dense), 4 + k sums per frame (trace), a correlation surface per frame (corr), counts and sums per frame and
// bin of a label map (bins).
enum ReadKind : uint32_t { RK_TRIPLETS, RK_COO16, RK_COO32, RK_L2, RK_EVENTS, RK_SUM, RK_COUNTED_SUM, RK_DENSE, RK_TRACE, RK_CORR, RK_BINS, RK_KINDS };
struct ReadKindInfo {
    uint32_t esz;         // bytes per entry of the output, counted against the caller's capacity (0: the kind has no entries)
    uint32_t coo;         // what the emit kernel is told: 0 = triplets, else COO with values of that many bytes (RK_L2: 2, and no value array)
    bool stats;           // level-2 statistics are decoded as values (klevel 2)
    bool counts;          // the kernels of rc_count.hip run behind the count
    bool sums;            // adds into an rc_sum handle
    bool cells;           // writes cells of a size the arguments give (dense, trace, corr, bins), not entries
    bool held;            // host memory is staged in BOTH forms and filled only behind the verdict: a refused batch writes nothing
    const char *pageable; // what a submit says to an output in pageable host memory
};
inline ReadKindInfo read_kind_info(ReadKind k)
{
    static const char *const entries = "rc_expand_frames_submit: triplets must be device or page-locked host memory";
    static const ReadKindInfo table[RK_KINDS] = {
        /* RK_TRIPLETS    */ {24, 0, false, false, false, false, false, entries},
        /* RK_COO16       */ {10, 2, false, false, false, false, false, entries},
        /* RK_COO32       */ {12, 4, false, false, false, false, false, entries},
        /* RK_L2          */ {8, 2, true, false, false, false, false, entries},
        /* RK_EVENTS      */ {20, 0, false, true, false, false, true, "rc_count_frames_submit: events must be device or page-locked host memory"},
        /* RK_SUM         */ {0, 0, false, false, true, false, false, nullptr},
        /* RK_COUNTED_SUM */ {0, 0, false, true, true, false, false, nullptr},
        /* RK_DENSE       */ {0, 0, false, false, false, true, true, "rc_expand_frames_dense_submit: out must be device or page-locked host memory"},
        /* RK_TRACE       */ {0, 0, false, false, false, true, true, "rc_trace_frames_submit: out must be device or page-locked host memory"},
        /* RK_CORR        */ {0, 0, false, false, false, true, true, "rc_corr_frames_submit: out must be device or page-locked host memory"},
        /* RK_BINS        */ {0, 0, false, false, false, true, true, "rc_bins_frames_submit: out must be device or page-locked host memory"},
    };
    return table[k];
}
// the frames' value stream is decoded (level 1: residuals; level 2: statistics, for RK_L2 alone - otherwise stepped over)
inline bool read_kind_values(ReadKind k, uint32_t level) { return level == 1 || read_kind_info(k).stats; }
// what the expand kernels see: 2 = value 1, COO without the value array
inline uint32_t read_kind_klevel(ReadKind k, uint32_t level) { return level == 1 ? 1u : read_kind_info(k).stats ? 2u : 3u; }

// ---- the verdict: the error word the kernels leave has 1 = a block did not decode to its size, 2 = more entries than the capacity, 4 = a
// value stream shorter than its frame's set pixels need, 8 = not the device DEFLATE encoder's stream.  A route tests them in ITS order, the
// first step that fires is the verdict; the orders differ, and are the ones each route had when it was a chain of ifs of its own.
enum VerdictStep : uint8_t {
    VS_END,               // nothing fired: RC_OK
    VS_FOREIGN,           // bit 8
    VS_BLOCK,             // bit 1
    VS_VALUES,            // bit 4
    VS_VALUES_HOST,       // in place of bit 4: the host's per-frame check of the prefix against the value streams' bytes (values_short)
    VS_STATS_SHORT,       // rc_expand_frames_l2: stats holds fewer entries than the frames have statistics
    VS_NO_OUTPUT,         // the caller named no output array and gets the prefix alone: RC_OK here
    VS_CAPACITY,          // total > capacity, or bit 2
};
// rc_expand_frames_wait (every kind) | synchronous triplets / COO / level-2 | synchronous rc_count_frames and rc_sum_add_counted (no output
// array: it ends at VS_NO_OUTPUT) | synchronous sum, dense, trace, corr, bins: never RC_ERR_OUT_TOO_SMALL
enum VerdictRoute : uint32_t { VR_WAIT, VR_SYNC_ENTRIES, VR_SYNC_EVENTS, VR_SYNC_QUIET, VR_ROUTES };
inline VerdictRoute verdict_route_sync(ReadKindInfo i) { return i.counts ? VR_SYNC_EVENTS : i.sums || i.cells ? VR_SYNC_QUIET : VR_SYNC_ENTRIES; }
struct VerdictFacts {
    uint32_t err;                     // the error word
    uint64_t total, cap;              // entries the batch has, entries the caller's output holds (a kind without entries is never too small)
    bool has_output;                  // the caller named an output array
    bool stats_short, values_short;   // what the synchronous entries route found on the host (false elsewhere)
};
struct Verdict {
    int status; const char *msg; VerdictStep step;      // msg: rc_last_error's text; step: the one that fired
    bool decoded() const { return step != VS_FOREIGN && step != VS_BLOCK; }      // the streams decoded, whatever became of the entries
};
inline Verdict read_verdict(VerdictRoute route, ReadKind kind, const VerdictFacts &f)
{
    static const VerdictStep order[VR_ROUTES][7] = {
        /* VR_WAIT         */ {VS_FOREIGN, VS_BLOCK, VS_CAPACITY, VS_VALUES, VS_END},
        /* VR_SYNC_ENTRIES */ {VS_FOREIGN, VS_BLOCK, VS_STATS_SHORT, VS_NO_OUTPUT, VS_CAPACITY, VS_VALUES_HOST, VS_END},
        /* VR_SYNC_EVENTS  */ {VS_FOREIGN, VS_BLOCK, VS_VALUES, VS_NO_OUTPUT, VS_CAPACITY, VS_END},
        /* VR_SYNC_QUIET   */ {VS_FOREIGN, VS_BLOCK, VS_VALUES, VS_END},
    };
    const uint64_t cap = read_kind_info(kind).esz ? f.cap : ~0ull;
    for (const VerdictStep *s = order[route]; *s != VS_END; ++s) {
        const char *msg = nullptr;
        int status = RC_ERR_CORRUPT;
        if (*s == VS_FOREIGN && (f.err & 8)) { status = RC_ERR_UNSUPPORTED; msg = "rc_expand_frames: not the device DEFLATE encoder's stream (use the stock decoder)"; }
        if (*s == VS_BLOCK && (f.err & 1)) msg = "rc_expand_frames: a block does not decode to its expected size";
        if ((*s == VS_VALUES && (f.err & 4)) || (*s == VS_VALUES_HOST && f.values_short))
            msg = "rc_expand_frames: value stream shorter than popcount(bitmap) * bit_depth bits";
        if (*s == VS_STATS_SHORT && f.stats_short) { status = RC_ERR_OUT_TOO_SMALL; msg = "rc_expand_frames_l2: stats holds fewer entries than the frames have statistics"; }
        if (*s == VS_CAPACITY && (f.total > cap || (f.err & 2))) {
            status = RC_ERR_OUT_TOO_SMALL;
            msg = route == VR_SYNC_EVENTS ? "rc_count_frames: events holds fewer entries than the frames have events"
                                          : "rc_expand_frames: triplets holds fewer entries than the frames have set pixels";
        }
        if (msg) return {status, msg, *s};
        if (*s == VS_NO_OUTPUT && !f.has_output) return {RC_OK, nullptr, *s};
    }
    return {RC_OK, nullptr, VS_END};
}

// ---- the copy-back: an output staged in device memory keeps the caller's layout (the arrays of a COO or event output `cap` entries apart),
// so it goes back as up to four (offset, bytes) segments, the same offsets on both sides
struct CopyPlan { uint32_t nseg; struct { uint64_t off, bytes; } seg[4]; };
// behind the verdict: the `total` entries the batch has (none: nothing to copy), or all `cell_bytes` of a dense / trace / corr / bins output
inline CopyPlan read_copy_plan(ReadKind k, uint64_t cap, uint64_t total, uint64_t cell_bytes)
{
    const ReadKindInfo i = read_kind_info(k);
    if (i.cells) return {1, {{0, cell_bytes}}};
    if (!i.esz || !total) return {0, {}};
    if (k == RK_TRIPLETS) return {1, {{0, total * 24}}};
    if (k == RK_EVENTS) return {4, {{0, total * 8}, {cap * 8, total * 4}, {cap * 12, total * 4}, {cap * 16, total * 4}}};
    return {i.esz > 8 ? 3u : 2u, {{0, total * 4}, {cap * 4, total * 4}, {cap * 8, total * (i.esz - 8)}}};
}
// queued by a submit right behind the emit kernel, before anything is known: all `cap` entries in one piece
inline CopyPlan read_copy_plan_early(ReadKind k, uint64_t cap) { return {cap ? 1u : 0u, {{0, cap * read_kind_info(k).esz}}}; }
// A submitted batch's page-locked output is filled early (one copy of cap entries under the next batch's work) unless the kind is held back
// or the codec may still refuse the batch on the device (the device inflate): then rc_expand_frames_wait fills it, behind the verdict.
inline bool read_copy_is_late(ReadKind k, bool device_inflate) { return read_kind_info(k).held || device_inflate; }
}  // namespace rc
