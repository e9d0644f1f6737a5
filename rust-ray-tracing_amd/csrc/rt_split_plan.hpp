// rt_split_plan.hpp — the sample-parallel path's plan (rt_split_plan, rt_render_split_async): how many
// samples one work item holds when a pixel's samples are dealt to several waves.  Pure host C++ (no HIP):
// the library, the CLI's callers and the stand-alone sanitizer program tests/sanitize/split_plan_san.cpp
// include it.
#pragma once
#include <stdint.h>

namespace rt {

// Return codes, the values of RT_OK / RT_ERR_INVALID / RT_ERR_UNSUPPORTED (include/rt_mi355x.h).
constexpr int kPlanOk = 0, kPlanInvalid = 1, kPlanUnsupported = 4;

// Items the plan aims for per resident wave: the factor the claim scheme's T = kTMul x workgroups uses for
// its single-item tail.  4, 8 and 16 were measured (profiles/sample_parallel.txt).
constexpr uint32_t kSplitItemsPerWave = 8;
// An item's samples: a multiple of 128, so an item is two full camera batches at least and no two items
// share a 128-byte line of the u8 termination-bounce array.
constexpr uint32_t kSplitGrain = 128;
constexpr uint32_t kSplitMaxSpp = 1u << 20;          // the ABI's spp limit
constexpr uint64_t kSplitMaxItems = 0x7FFFFFFFull;   // work items of one launch (a 32-bit claim counter)

// Items per pixel when an item holds S samples (S >= 1).
inline uint32_t split_nsub(uint32_t spp, uint32_t S) { return (uint32_t)(((uint64_t)spp + S - 1u) / S); }

// The auto plan.  S: samples per item, a multiple of kSplitGrain, or spp itself when the plan is one item per
// pixel (then n_items == n_pixels and the render runs unsplit).  resident_waves == 0 plans one item per pixel.
// A launch is split only when it has fewer pixels than resident waves, the launches that leave waves without
// a pixel: measured, 0.45 pixels per wave (64x36) ran 4.2x faster split, 6.3 per wave (240x135 at 512 spp)
// 0.90x, the second kernel and the record round trip costing more than the finer items gain
// (profiles/sample_parallel.txt).
inline int split_plan(uint64_t n_pixels, uint32_t spp, uint32_t resident_waves, uint32_t* samples_per_item,
                      uint64_t* n_items) {
    if (!samples_per_item || !n_items) return kPlanInvalid;
    *samples_per_item = 0;
    *n_items = 0;
    if (n_pixels == 0 || spp == 0) return kPlanInvalid;
    if (spp > kSplitMaxSpp || n_pixels > kSplitMaxItems) return kPlanUnsupported;
    const uint64_t want = (uint64_t)kSplitItemsPerWave * resident_waves;   // items in the launch
    const uint64_t per_pixel = n_pixels >= resident_waves ? 1u : (want + n_pixels - 1u) / n_pixels;
    uint64_t S = ((uint64_t)spp + per_pixel - 1u) / per_pixel;
    S = (S + kSplitGrain - 1u) / kSplitGrain * kSplitGrain;
    if (S >= spp) {
        *samples_per_item = spp;
        *n_items = n_pixels;
        return kPlanOk;
    }
    const uint64_t items = n_pixels * split_nsub(spp, (uint32_t)S);   // <= 2^31 x 2^13: no overflow
    if (items > kSplitMaxItems) return kPlanUnsupported;
    *samples_per_item = (uint32_t)S;
    *n_items = items;
    return kPlanOk;
}

}  // namespace rt
