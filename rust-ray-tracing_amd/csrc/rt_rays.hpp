// rt_rays.hpp — rendering caller-supplied primary rays (rt_render_rays_async): full paths for the rays of any camera
// model (orthographic, fisheye, a panorama: rt_projection.hpp) or of the caller's own tensors.  Two kernels:
//   * rays_validate<T>: one thread per pixel checks the pixel's R rays against the query's precondition
//     (rt_query.hpp), sets the pixel's bit in the skip mask where a ray fails it, writes that pixel's outputs (NaN,
//     black) and counts the samples of the valid pixels (rt_stats.samples).
//   * trace_paths_rays<T, W, ROOT2, MEGA>: rt_trace_body.hpp with RAYS.  A fresh lane loads its primary ray from the
//     caller's arrays instead of running next_ray(cam = true); a claimed pixel whose skip bit is set is passed over
//     the way the camera batches pass over sky pixels.  Bounce 0 goes through the general sweep like every other
//     bounce; the scatter, the records, the replay and the reduction are the render's.
// The rays are read once per sample by the lane that traces them: consecutive samples of a pixel read consecutive
// 12- or 24-byte records.
#pragma once
#include "rt_trace.hpp"
#include "rt_query.hpp"

namespace rt {

// Waves per SIMD the register allocation targets: the default of the precision (no RT_WAVES variants).
template <typename T> constexpr int kWavesRays = sizeof(T) == 4 ? kWavesF32 : kWavesF64;

template <typename T>
__global__ __launch_bounds__(256) void rays_validate(RParams<T> rp) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n = rp.k.n_items;   // <= 0x7FFFFFFF pixels
    const uint32_t px = blockIdx.x * 256u + threadIdx.x;   // < n + 256
    const bool in = px < n;
    bool bad = false;
    if (in) {
        const uint32_t R = rp.R;
        const bool shared = rp.origins == nullptr;
        V3<T> o = mk(rp.k.center[0], rp.k.center[1], rp.k.center[2]);
        if (shared) bad = !query_finite(o);
        for (uint32_t r = 0; r < R; ++r) {
            const size_t ray = (size_t)px * R + r;
            const T* dp = rp.directions + 3 * ray;
            const V3<T> d = mk(dp[0], dp[1], dp[2]);
            if (!shared) {
                const T* op = rp.origins + 3 * ray;
                o = mk(op[0], op[1], op[2]);
            }
            const T a = pk_len2(d);
            const bool v = query_finite(o) && query_finite(d) && a >= kQueryLen2Min<T> && a <= kQueryLen2Max<T>;
            bad = bad || !v;
        }
        if (bad) {   // not traced: NaN and black, and no RT_ERR_RANGE
            for (uint32_t ch = 0; ch < 3u; ++ch) {
                if (rp.k.rgb) rp.k.rgb[(size_t)px * 3 + ch] = 0u;
                if (rp.k.lin) rp.k.lin[(size_t)px * 3 + ch] = __builtin_nan("");
            }
        }
    }
    const unsigned long long bm = __ballot(bad), vm = __ballot(in && !bad);
    if (lane == 0 && (blockIdx.x * 256u + (threadIdx.x & ~63u)) < n) {
        rp.skip[px >> 6] = bm;   // the wave's 64 pixels: word (n + 63) / 64 - 1 at most
        if (vm != 0ull) {
            const uint32_t gw = px >> 6;
            atomicAdd(&rp.k.segs[(gw & (kSegShards - 1)) * kSegStride + kQuerySlot],
                      (unsigned long long)__builtin_popcountll(vm) * rp.k.spp);
        }
    }
}

template <typename T, int W, bool ROOT2, bool MEGA>
__global__ __launch_bounds__(256, W) void trace_paths_rays(RParams<T> rp) {
    constexpr bool SPLIT = kSplitKernel<T, false>, WIN = kSplitKernel<T, false>, ITEMS = kSplitKernel<T, false>;
    constexpr bool RAYS = kSplitKernel<T, true>, CAMQ = false;
    constexpr int MODE = kModeV2;
#include "rt_trace_body.hpp"
}

}  // namespace rt
