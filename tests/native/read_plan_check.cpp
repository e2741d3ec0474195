// read_plan_check.cpp - the host build of pyrecode_amd/csrc/rc_read_plan.h as a stand-alone program (tests/test_read_plan_cpu.py builds it,
// also under AddressSanitizer / UBSan): every result kind x the 16 values of the error word x {total < cap, == cap, > cap} x {synchronous,
// waited-for} for the verdict, every kind x {total 0, 1, cap} for the copy-back segments, and what a kind means for the kernels - against
// the tables below.  The tables were written out by hand from the chains of ifs rc_reader.hip had before the header existed (commit
// 4090e1e; the line numbers are that file's); nothing in them is computed by the code under test.  Prints "ok"; the exit status is 1 when
// an answer was wrong, and every wrong answer is printed.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../pyrecode_amd/csrc/rc_read_plan.h"

using namespace rc;

static_assert(RK_KINDS == 11, "a new kind: a row in every table below");
static const char *const KIND[RK_KINDS] = {"triplets", "coo16", "coo32", "l2", "events", "sum", "counted_sum", "dense", "trace", "corr", "bins"};
// the entry point a kind's `pageable` message names, and speaks for (the four kinds of entries share rc_expand_frames_submit's; a sum has no output)
static const char *const SUBMIT[RK_KINDS] = {"rc_expand_frames_submit: ", "rc_expand_frames_submit: ", "rc_expand_frames_submit: ", "rc_expand_frames_submit: ",
                                             "rc_count_frames_submit: ", nullptr, nullptr, "rc_expand_frames_dense_submit: ", "rc_trace_frames_submit: ",
                                             "rc_corr_frames_submit: ", "rc_bins_frames_submit: "};
// the kinds whose output is cells of a size the arguments give, all of them copied back whatever the total ... and those held back behind the verdict
static bool is_cells(uint32_t k) { return k == RK_DENSE || k == RK_TRACE || k == RK_CORR || k == RK_BINS; }
static bool is_held(uint32_t k) { return k == RK_EVENTS || is_cells(k); }
static int failures = 0;

// a verdict row: per error word 0..15 the statuses for total < cap, == cap, > cap - O = RC_OK, U = RC_ERR_UNSUPPORTED, C = RC_ERR_CORRUPT,
// S = RC_ERR_OUT_TOO_SMALL
typedef const char *Row[16];
#define U8 "UUU", "UUU", "UUU", "UUU", "UUU", "UUU", "UUU", "UUU"      /* bit 8 is tested first everywhere (lines 547, 600, 658, 781) */
// rc_expand_frames_wait, lines 781-784: 8, 1, then total > u.cap or bit 2, then 4 ...
static const Row WAIT_ENTRIES = {"OOS", "CCC", "SSS", "CCC", "CCS", "CCC", "SSS", "CCC", U8};
// ... with u.cap = ~0 for a sum (lines 540, 650) and for dense / trace (line 593): the total never passes it, bit 2 is still looked at
static const Row WAIT_NO_ENTRIES = {"OOO", "CCC", "SSS", "CCC", "CCC", "CCC", "SSS", "CCC", U8};
// the synchronous triplet / COO / level-2 tail, lines 658-672: 8, 1, (stats), no output -> OK, total > cap or bit 2, then the HOST's check of
// the value streams in place of bit 4 (which is not looked at) - the frames' value streams long enough ...
static const Row SYNC_ENTRIES = {"OOS", "CCC", "SSS", "CCC", "OOS", "CCC", "SSS", "CCC", U8};
// ... or one of them short (lines 669-672)
static const Row SYNC_ENTRIES_SHORT = {"CCS", "CCC", "SSS", "CCC", "CCS", "CCC", "SSS", "CCC", U8};
// ... no output array (line 667): the capacity and the value streams are not judged
static const Row SYNC_ENTRIES_NO_OUT = {"OOO", "CCC", "OOO", "CCC", "OOO", "CCC", "OOO", "CCC", U8};
// ... rc_expand_frames_l2 with stats too small (lines 203-205 drop the output, line 662 answers behind bits 8 and 1)
static const Row SYNC_STATS_SHORT = {"SSS", "CCC", "SSS", "CCC", "SSS", "CCC", "SSS", "CCC", U8};
// the synchronous counted tail, lines 547-552: 8, 1, 4, no event array -> OK, then total > cap or bit 2
static const Row SYNC_EVENTS = {"OOS", "CCC", "SSS", "CCC", "CCC", "CCC", "CCC", "CCC", U8};
// ... without an event array (rc_sum_add_counted always, line 550), and the dense / trace tail (lines 600-602) and the sum's (lines 658-661):
// 8, 1, 4 and never RC_ERR_OUT_TOO_SMALL
static const Row SYNC_QUIET = {"OOO", "CCC", "OOO", "CCC", "CCC", "CCC", "CCC", "CCC", U8};

static int status_of(char c) { return c == 'O' ? RC_OK : c == 'U' ? RC_ERR_UNSUPPORTED : c == 'C' ? RC_ERR_CORRUPT : RC_ERR_OUT_TOO_SMALL; }

// the message of a refusal: its first words, by status and route (lines 547-552, 600-602, 658-672, 781-784)
static const char *message_of(int status, uint32_t err, bool sync_events, bool stats_short)
{
    if (status == RC_OK) return nullptr;
    if (status == RC_ERR_UNSUPPORTED) return "rc_expand_frames: not the device DEFLATE encoder's stream";
    if (status == RC_ERR_CORRUPT) return (err & 1) ? "rc_expand_frames: a block does not decode" : "rc_expand_frames: value stream shorter";
    return stats_short ? "rc_expand_frames_l2: stats holds fewer" : sync_events ? "rc_count_frames: events holds fewer" : "rc_expand_frames: triplets holds fewer";
}

static void check_row(const char *what, VerdictRoute route, ReadKind k, const Row &row, bool has_output, bool stats_short, bool values_short)
{
    const uint64_t cap = 7, totals[3] = {6, 7, 8};
    for (uint32_t err = 0; err < 16; ++err)
        for (int j = 0; j < 3; ++j) {
            const VerdictFacts f{err, totals[j], cap, has_output, stats_short, values_short};
            const Verdict v = read_verdict(route, k, f);
            const int want = status_of(row[err][j]);
            const char *msg = message_of(want, err, route == VR_SYNC_EVENTS, stats_short);
            const bool msg_ok = msg ? v.msg && strncmp(v.msg, msg, strlen(msg)) == 0 : v.msg == nullptr;
            if (v.status != want || !msg_ok || (v.status == RC_OK) != (v.step == VS_END || v.step == VS_NO_OUTPUT)) {
                printf("verdict %s %s err %u total %llu: status %d (%s), expected %d (%s)\n", what, KIND[k], err, (unsigned long long)totals[j], v.status,
                       v.msg ? v.msg : "-", want, msg ? msg : "-");
                ++failures;
            }
        }
}

struct Seg { uint64_t off, bytes; };
static void check_plan(const char *what, ReadKind k, uint64_t total, const CopyPlan &got, uint32_t nseg, const Seg *want)
{
    bool ok = got.nseg == nseg;
    for (uint32_t i = 0; ok && i < nseg; ++i) ok = got.seg[i].off == want[i].off && got.seg[i].bytes == want[i].bytes;
    if (!ok) { printf("%s %s total %llu: wrong segments\n", what, KIND[k], (unsigned long long)total); ++failures; }
}

int main()
{
    // ---- what a kind means for the kernels: esz (line 161), values (line 176), klevel (line 177) -------------------------------------------
    const uint32_t esz[RK_KINDS] = {24, 10, 12, 8, 20, 0, 0, 0, 0, 0, 0};      // (0: no entries - the kinds whose capacity was ~0 or unused)
    const uint32_t coo[RK_KINDS] = {0, 2, 4, 2, 0, 0, 0, 0, 0, 0, 0};          // (the entry points' `coo` argument, lines 722, 738, 753)
    for (uint32_t i = 0; i < RK_KINDS; ++i) {
        const ReadKind k = (ReadKind)i;
        const ReadKindInfo info = read_kind_info(k);
        const bool l2 = k == RK_L2;
        bool ok = info.esz == esz[i] && info.coo == coo[i] && info.stats == l2;
        ok = ok && info.counts == (k == RK_EVENTS || k == RK_COUNTED_SUM) && info.sums == (k == RK_SUM || k == RK_COUNTED_SUM);
        ok = ok && info.cells == is_cells(i) && info.held == is_held(i);
        // (lines 176-177 say "level == 1 || l2out" and "level == 1 ? 1 : l2out ? 2 : 3": the level-2 kind at level 3 - refused before, line 167 -
        // answers as at level 2)
        ok = ok && read_kind_klevel(k, 1) == 1 && read_kind_klevel(k, 2) == (l2 ? 2u : 3u) && read_kind_klevel(k, 3) == (l2 ? 2u : 3u);
        ok = ok && read_kind_values(k, 1) && read_kind_values(k, 2) == l2 && read_kind_values(k, 3) == l2;
        ok = ok && ((info.pageable != nullptr) == (esz[i] != 0 || is_cells(i))) && (info.pageable != nullptr) == (SUBMIT[i] != nullptr);
        ok = ok && (!info.pageable || (strncmp(info.pageable, SUBMIT[i], strlen(SUBMIT[i])) == 0 && strstr(info.pageable, "page-locked")));
        if (!ok) { printf("kind %s: wrong info\n", KIND[i]); ++failures; }
    }
    // ---- the verdict ---------------------------------------------------------------------------------------------------------------------
    for (uint32_t i = 0; i < RK_KINDS; ++i) {
        const ReadKind k = (ReadKind)i;
        check_row("wait", VR_WAIT, k, esz[i] ? WAIT_ENTRIES : WAIT_NO_ENTRIES, true, false, false);
        check_row("wait, no facts", VR_WAIT, k, esz[i] ? WAIT_ENTRIES : WAIT_NO_ENTRIES, false, false, false);      // (as rc_expand_frames_wait calls it: never OK early)
        if (i <= RK_L2) {
            if (verdict_route_sync(read_kind_info(k)) != VR_SYNC_ENTRIES) { printf("%s: wrong synchronous route\n", KIND[i]); ++failures; }
            check_row("sync", VR_SYNC_ENTRIES, k, SYNC_ENTRIES, true, false, false);
            check_row("sync, a value stream short", VR_SYNC_ENTRIES, k, SYNC_ENTRIES_SHORT, true, false, true);
            check_row("sync, no output", VR_SYNC_ENTRIES, k, SYNC_ENTRIES_NO_OUT, false, false, false);
            check_row("sync, no output, a value stream short", VR_SYNC_ENTRIES, k, SYNC_ENTRIES_NO_OUT, false, false, true);
            if (k == RK_L2) check_row("sync, stats short", VR_SYNC_ENTRIES, k, SYNC_STATS_SHORT, false, true, false);
        } else if (k == RK_EVENTS || k == RK_COUNTED_SUM) {
            if (verdict_route_sync(read_kind_info(k)) != VR_SYNC_EVENTS) { printf("%s: wrong synchronous route\n", KIND[i]); ++failures; }
            if (k == RK_EVENTS) check_row("sync", VR_SYNC_EVENTS, k, SYNC_EVENTS, true, false, false);
            check_row("sync, no output", VR_SYNC_EVENTS, k, SYNC_QUIET, false, false, false);
        } else {
            if (verdict_route_sync(read_kind_info(k)) != VR_SYNC_QUIET) { printf("%s: wrong synchronous route\n", KIND[i]); ++failures; }
            check_row("sync", VR_SYNC_QUIET, k, SYNC_QUIET, k != RK_SUM, false, false);
        }
    }
    // ---- the copy-back, cap = 7 entries, a dense / trace / corr / bins output of 1000 bytes -------------------------------------------------
    // triplets: one copy of total * 24 (lines 696, 794); COO: rows, columns, values cap entries apart (lines 686-688, 796-799; level 2: no
    // values); events: copy_events, lines 123-129; dense / trace / corr / bins: all bytes whatever the total (lines 604, 787); a sum: nothing
    const uint64_t cap = 7, cells = 1000, totals[3] = {0, 1, 7};
    const Seg t1[] = {{0, 24}}, t7[] = {{0, 168}};
    const Seg c16_1[] = {{0, 4}, {28, 4}, {56, 2}}, c16_7[] = {{0, 28}, {28, 28}, {56, 14}};
    const Seg c32_1[] = {{0, 4}, {28, 4}, {56, 4}}, c32_7[] = {{0, 28}, {28, 28}, {56, 28}};
    const Seg l2_1[] = {{0, 4}, {28, 4}}, l2_7[] = {{0, 28}, {28, 28}};
    const Seg ev_1[] = {{0, 8}, {56, 4}, {84, 4}, {112, 4}}, ev_7[] = {{0, 56}, {56, 28}, {84, 28}, {112, 28}};
    const Seg all[] = {{0, 1000}};
    const struct { uint32_t nseg; const Seg *one, *full; } want[RK_KINDS] = {{1, t1, t7}, {3, c16_1, c16_7}, {3, c32_1, c32_7}, {2, l2_1, l2_7}, {4, ev_1, ev_7},
                                                                              {0, nullptr, nullptr}, {0, nullptr, nullptr}, {1, all, all}, {1, all, all},
                                                                              {1, all, all}, {1, all, all}};
    for (uint32_t i = 0; i < RK_KINDS; ++i)
        for (int j = 0; j < 3; ++j) {
            const uint32_t nseg = (j == 0 && !is_cells(i)) ? 0 : want[i].nseg;
            check_plan("copy-back", (ReadKind)i, totals[j], read_copy_plan((ReadKind)i, cap, totals[j], cells), nseg, j == 2 ? want[i].full : want[i].one);
        }
    // a submit's eager copy (line 641): cap * esz bytes in one piece, nothing for cap 0; late (lines 537, 589, 640): the held kinds always,
    // entries for the device inflate alone
    const Seg early[4][1] = {{{0, 168}}, {{0, 70}}, {{0, 84}}, {{0, 56}}};
    for (uint32_t i = 0; i <= RK_L2; ++i) {
        check_plan("early copy", (ReadKind)i, cap, read_copy_plan_early((ReadKind)i, cap), 1, early[i]);
        check_plan("early copy", (ReadKind)i, 0, read_copy_plan_early((ReadKind)i, 0), 0, nullptr);
    }
    for (uint32_t i = 0; i < RK_KINDS; ++i) {
        if (read_copy_is_late((ReadKind)i, false) != is_held(i) || !read_copy_is_late((ReadKind)i, true)) { printf("%s: wrong early / late\n", KIND[i]); ++failures; }
    }
    if (failures) { printf("%d answers wrong\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
