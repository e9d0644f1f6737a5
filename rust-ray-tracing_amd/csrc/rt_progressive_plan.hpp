// rt_progressive_plan.hpp — the host arithmetic of a progressive session (rt_progressive_*): the record
// buffer a session of a given sample capacity needs, and how one extend's sample window [done, spp_total)
// is dealt into work items, uniformly or with a sample count per pixel, and how a reduction's pixels are grouped
// by count.  Pure host C++ (no HIP): the library, the stand-alone sanitizer programs
// tests/sanitize/progressive_plan_san.cpp and map_plan_san.cpp and tests/group_by_count_check.cpp include it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

#include "rt_split_plan.hpp"

namespace rt {

constexpr uint32_t kProgFlagF32 = 0x1u, kProgFlagAll = 0x1Fu;   // RT_FLAG_F32, RT_FLAG_ALL (include/rt_mi355x.h)

// Positions of a pixel of `spp` samples: whole chunks of 4 (PackedRays<4>).
inline uint32_t prog_positions(uint32_t spp) { return 4u * ((spp + 3u) / 4u); }

// One pixel's region of the record buffer at P_cap positions: y[P] (T), c[P] (3 T), e[P] (u8; u32 when
// max_bounces > 254), rounded up to 256 bytes.  The value of paths_sbytes(P, tsz, paths_wide(P, depth))
// (rt_finish.hpp; rt_progressive_begin checks that they agree).
inline uint32_t prog_region_bytes(uint32_t P_cap, uint32_t tsz, uint32_t max_bounces) {
    const uint32_t esz = max_bounces > 254u ? 4u : 1u;
    return (P_cap * (4u * tsz + esz) + 255u) & ~255u;   // P_cap <= 2^20, 36 bytes each: below 2^26
}

// rt_progressive_bytes.  17 bytes per sample of capacity in fp32, 33 in fp64 (u8 e).
inline int progressive_bytes(uint64_t n_pixels, uint32_t spp_capacity, uint32_t max_bounces, uint32_t flags,
                             uint64_t* bytes) {
    if (!bytes) return kPlanInvalid;
    *bytes = 0;
    if (n_pixels == 0 || spp_capacity == 0) return kPlanInvalid;
    if (flags & ~kProgFlagAll) return kPlanInvalid;   // as rt_render_split_async: unknown bits are invalid,
    if (flags & ~kProgFlagF32) return kPlanUnsupported;   // RT_FLAG_ROOT2 and RT_FLAG_MODE_* unsupported
    if (spp_capacity > kSplitMaxSpp || n_pixels > kSplitMaxItems) return kPlanUnsupported;
    const uint32_t tsz = (flags & kProgFlagF32) ? 4u : 8u;
    *bytes = n_pixels * prog_region_bytes(prog_positions(spp_capacity), tsz, max_bounces);   // < 2^31 x 2^26
    return kPlanOk;
}

// One extend's items.  Item i is pixel i / nsub and, with j = i % nsub, the samples
//   [max(done, base + j S), min(spp_total, base + (j + 1) S)).
// Where S is a multiple of kSplitGrain, base is `done` rounded down to the grain, so every item boundary but
// the window's own ends is an absolute multiple of 128 (a short first item): no two items of a launch share a
// 128-byte line of a pixel's u8 e array, as in rt_render_split_async.  Any other S (the one-item-per-pixel
// plan, whose S is the window itself) starts at `done`.
struct ProgWindow {
    uint32_t S, nsub, base;
    uint64_t n_items;
};

inline void prog_item(const ProgWindow& w, uint32_t done, uint32_t spp_total, uint32_t j, uint32_t* first,
                      uint32_t* end) {
    const uint32_t a = w.base + j * w.S, b = a + w.S;   // <= spp_total + S <= 2^21
    *first = a > done ? a : done;
    *end = b < spp_total ? b : spp_total;
}

// The window [done, spp_total) in items of S samples (S >= 1, done < spp_total <= 2^20).
inline int progressive_window_s(uint64_t n_pixels, uint32_t done, uint32_t spp_total, uint32_t S, ProgWindow* w) {
    if (!w) return kPlanInvalid;
    *w = ProgWindow{0u, 0u, 0u, 0u};
    if (n_pixels == 0 || S == 0 || spp_total <= done) return kPlanInvalid;
    if (spp_total > kSplitMaxSpp || S > kSplitMaxSpp || n_pixels > kSplitMaxItems) return kPlanUnsupported;
    const uint32_t base = S % kSplitGrain == 0u ? done - done % kSplitGrain : done;
    const uint32_t nsub = split_nsub(spp_total - base, S);
    const uint64_t items = n_pixels * nsub;   // < 2^31 x 2^20
    if (items > kSplitMaxItems) return kPlanUnsupported;
    *w = ProgWindow{S, nsub, base, items};
    return kPlanOk;
}

// The plan of rt_progressive_extend_async: split_plan over the window's samples.
inline int progressive_window(uint64_t n_pixels, uint32_t done, uint32_t spp_total, uint32_t resident_waves,
                              ProgWindow* w) {
    if (!w) return kPlanInvalid;
    *w = ProgWindow{0u, 0u, 0u, 0u};
    if (spp_total <= done) return kPlanInvalid;
    uint32_t S = 0;
    uint64_t n = 0;
    const int rc = split_plan(n_pixels, spp_total - done, resident_waves, &S, &n);
    if (rc != kPlanOk) return rc;
    return progressive_window_s(n_pixels, done, spp_total, S, w);
}

// ---- per-pixel counts (rt_progressive_extend_map_async) ----
// One extend of a map: pixel p goes from done[p] to target[p] samples.  The items are records of four words
// {pixel, first, end, 0} (the item table trace_paths_items reads), in pixel order with a pixel's items adjacent.
constexpr uint32_t kMapItemWords = 4;

// The plan: with A the active pixels (target > done) and mean = ceil(sum of (target - done) / A), S is
// split_plan(A, mean, resident_waves)'s.  Where S is a multiple of kSplitGrain, pixel p's items are those of
// progressive_window_s(1, done[p], target[p], S): they lie on the grid base_p + j S, base_p = done[p] rounded down
// to the grain, so no two items of a launch share a 128-byte line of a pixel's u8 e array.  Any other S (the
// one-item-per-pixel plan at a mean off the grain) makes every active pixel one item [done[p], target[p]).  A
// uniform map therefore has the items of progressive_window.
// *samples_per_item: S (0: no pixel is active); *n_items: the items of the plan, always set when the arrays are
// valid.  items (may be NULL: count only) receives them when items_capacity (in items) holds them all.
// Invalid: a NULL array or output, no pixels, a target below done, items given with too small a capacity.
// Unsupported: a target above 2^20, more than 0x7FFFFFFF pixels or items.
inline int progressive_map_plan(uint64_t n_pixels, const uint32_t* done, const uint32_t* target,
                                uint32_t resident_waves, uint32_t* samples_per_item, uint64_t* n_items,
                                uint32_t* items, uint64_t items_capacity) {
    if (!samples_per_item || !n_items) return kPlanInvalid;
    *samples_per_item = 0;
    *n_items = 0;
    if (!done || !target || n_pixels == 0) return kPlanInvalid;
    if (n_pixels > kSplitMaxItems) return kPlanUnsupported;
    uint64_t active = 0, total = 0;
    for (uint64_t p = 0; p < n_pixels; ++p) {
        if (target[p] < done[p]) return kPlanInvalid;
        if (target[p] > kSplitMaxSpp) return kPlanUnsupported;
        if (target[p] > done[p]) { ++active; total += target[p] - done[p]; }   // < 2^31 x 2^20
    }
    if (active == 0) return kPlanOk;
    const uint32_t mean = (uint32_t)((total + active - 1u) / active);
    uint32_t S = 0;
    uint64_t n = 0;
    const int rc = split_plan(active, mean, resident_waves, &S, &n);
    if (rc != kPlanOk) return rc;
    const bool grid = S % kSplitGrain == 0u;
    uint64_t count = 0;
    for (uint64_t p = 0; p < n_pixels; ++p) {
        if (target[p] <= done[p]) continue;
        const uint32_t base = grid ? done[p] - done[p] % kSplitGrain : done[p];
        count += grid ? split_nsub(target[p] - base, S) : 1u;   // < 2^31 x 2^13
    }
    if (count > kSplitMaxItems) return kPlanUnsupported;
    *samples_per_item = S;
    *n_items = count;
    if (!items) return kPlanOk;
    if (items_capacity < count) return kPlanInvalid;
    uint32_t* it = items;
    for (uint64_t p = 0; p < n_pixels; ++p) {
        if (target[p] <= done[p]) continue;
        if (!grid) {
            it[0] = (uint32_t)p; it[1] = done[p]; it[2] = target[p]; it[3] = 0u;
            it += kMapItemWords;
            continue;
        }
        ProgWindow w;
        (void)progressive_window_s(1u, done[p], target[p], S, &w);   // valid: checked above
        for (uint32_t j = 0; j < w.nsub; ++j, it += kMapItemWords) {
            it[0] = (uint32_t)p;
            prog_item(w, done[p], target[p], j, &it[1], &it[2]);
            it[3] = 0u;
        }
    }
    return kPlanOk;
}

// ---- the reductions of a call over per-pixel counts (finish_window_list, a launch per count) ----
// The pixels of one reduction that share a sample count: list[first .. first + n) of the reduction's index list.
struct CountClass {
    uint32_t spp, first, n;
};
constexpr size_t kMaxCountClasses = 256;   // distinct counts one reduction may have (a launch each)

// Group the pixels by counts[p] (0: the pixel is left out): the classes in ascending count, and, with list, each
// class's pixel indices in pixel order.  false: more than kMaxCountClasses distinct counts.
inline bool group_by_count(const uint32_t* counts, uint32_t n_pix, uint32_t* list, std::vector<CountClass>& cls) {
    cls.clear();
    auto find = [&](uint32_t n) {
        return std::lower_bound(cls.begin(), cls.end(), n, [](const CountClass& k, uint32_t v) { return k.spp < v; });
    };
    size_t last = 0;   // the class of the previous pixel: neighbours mostly share a count
    for (uint32_t p = 0; p < n_pix; ++p) {
        if (counts[p] == 0u) continue;
        if (last >= cls.size() || cls[last].spp != counts[p]) {
            auto it = find(counts[p]);
            if (it == cls.end() || it->spp != counts[p]) {
                if (cls.size() == kMaxCountClasses) return false;
                it = cls.insert(it, CountClass{counts[p], 0u, 0u});
            }
            last = (size_t)(it - cls.begin());
        }
        ++cls[last].n;
    }
    uint32_t at = 0;
    for (CountClass& k : cls) { k.first = at; at += k.n; }
    if (!list) return true;
    for (CountClass& k : cls) k.n = 0u;
    for (uint32_t p = 0; p < n_pix; ++p) {
        if (counts[p] == 0u) continue;
        if (cls[last].spp != counts[p]) last = (size_t)(find(counts[p]) - cls.begin());
        CountClass& k = cls[last];
        list[k.first + k.n] = p;
        ++k.n;
    }
    return true;
}

}  // namespace rt
