// rt_guides.hpp — guide buffers (rt_render_guides_async): per pixel the mean first-hit albedo, normal, depth
// and coverage over the primary rays of the image at the same sample count, for a denoiser or an edge-aware
// filter behind a preview.  One kernel, guide_pixels<T, CAMQ, MEGA>: the trace kernels' primary ray
// (next_ray's camera branch) and bounce-0 hit (pixel_list + camera_listed, camera_sweep, or nearest_hit for a
// camera with defocus, as trace_paths has them), then PackedHitRecords::finalize (objects.rs:157-162) and a
// reduction in a fixed order.  It stops there: no scatter, no records, no replay.
//
// Mapping: the lane is the sample, a batch is 64 consecutive samples of one pixel, and a wave keeps its pixel
// until all the pixel's batches are done.  A lane's double accumulators are then the partials of the
// definition (include/rt_mi355x.h): partial j adds the samples with s % 64 == j in ascending s, the 64 partials
// are folded p[i] += p[i + h] for h = 32, 16, 8, 4, 2, 1, and lane 0 stores (float)(p[0] / n).  The order is
// fixed so that a value is a function of the pixel's samples alone, never of the launch shape.
#pragma once
#include "rt_sweep.hpp"
#include "rt_camera.hpp"

namespace rt {

// Arguments of guide_pixels: KParams first, so cold_args<T>() reads it from the same kernarg offsets (n_items:
// the pixels of the range, spp: the samples of each), then the outputs, compact over the range (any may be NULL).
template <typename T> struct GParams {
    KParams<T> k;
    float* albedo;     // [pixels][3]
    float* normal;     // [pixels][3]
    float* depth;      // [pixels]
    float* coverage;   // [pixels]
};

// Waves per SIMD the register allocation targets: the sample-parallel kernels' (they run the same sweeps).
template <typename T> constexpr int kWavesGuide = sizeof(T) == 4 ? 5 : 4;

// The fold of the 64 lanes' partials in the definition's order; lane 0 returns p[0].  A lane i < h reads lane
// i + h, whose value the steps before left correct (i + h < 2 h); what the lanes at and above h compute is
// never read by a lower lane again.  The fp64 value crosses lanes as two 32-bit halves (__shfl_down).
__device__ __forceinline__ double guide_fold(double p) {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) p += __shfl_down(p, (unsigned)h);
    return p;
}

constexpr uint32_t kGuideCh = 8;   // albedo r g b, normal x y z, depth, coverage

template <typename T, bool CAMQ, bool MEGA>
__global__ __launch_bounds__(256, kWavesGuide<T>) void guide_pixels(GParams<T> gp) {
    // the pixel's camera candidate list (pixel_list): [0] = count (0xFFFF: none, sweep per batch)
    __shared__ alignas(16) uint16_t s_clist[4][1][kCList];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (lane < kNWork) g_work[wave][lane] = 0ull;
#ifdef RT_KSTATS
    if (lane < kNKstat) g_kst[wave][lane] = 0;
#endif
    const uint32_t gw = blockIdx.x * 4u + wave, nw = gridDim.x * 4u;
    const uint32_t n_pix = cold_args<T>()->n_items;   // <= 0x7FFFFFFF: item + nw does not wrap
    unsigned long long n_seg = 0, n_slots = 0;
    for (uint32_t item = gw; item < n_pix; item += nw) {
        // range -> (col, row, pix), as the trace kernels' issue()
        uint32_t col, row, pix, spp;
        {
            const auto& q = *cold_args<T>();
            const uint32_t ri = item / q.col_count, ci = item % q.col_count;
            row = q.row_begin + ri * q.row_step;
            col = q.col_begin + ci;
            pix = row * q.W + col;
            spp = q.spp;
        }
        n_seg += spp;
        double acc[kGuideCh];
#pragma unroll
        for (uint32_t ch = 0; ch < kGuideCh; ++ch) acc[ch] = 0.0;
        uint32_t nl = 0xFFFFu;
        if constexpr (CAMQ) nl = __builtin_amdgcn_readfirstlane(pixel_list<T, MEGA>(col, row, s_clist[wave][0]));
        if (CAMQ && nl == 0u) {
            // no primary ray of the pixel can hit a sphere: every sample is a miss, albedo 1 and the rest 0, and
            // the definition's sums give exactly these (n ones sum to n <= 2^20, n / n = 1)
            acc[0] = acc[1] = acc[2] = (double)spp;
        } else {
            for (uint32_t s0 = 0; s0 < spp; s0 += 64u) {
                const uint32_t sid = s0 + lane;
                const bool v = sid < spp;
                V3<T> o = mk(T(0), T(0), T(0)), d = o, c = o;
                if (v) next_ray<T, false>(true, col, row, pix, sid, 0u, 0, T(0), o, d, c);   // Camera::get_ray
                T t = T(0);
                int hi = -1;
                if constexpr (CAMQ) {
                    if (nl != 0xFFFFu) hi = camera_listed<T, false, false>(v, d, t, s_clist[wave], 1u);
                    else hi = camera_sweep<T, false, false, MEGA>(v, d, t);   // whole wave: lanes are spheres in the cull
                } else {
                    if (v) hi = nearest_hit<T, false, false, MEGA>(o, d, t);
                }
                n_slots += 64u;
                const bool hit = v && hi >= 0;
                V3<T> alb = mk(T(1.0), T(1.0), T(1.0)), nrm = mk(T(0), T(0), T(0));
                T dep = T(0);
                if (hit) {
                    // PackedHitRecords::finalize (objects.rs:157-162), as next_ray's scatter branch has it
                    const auto& q = *cold_args<T>();
                    const T* sgp = q.cen + 4 * hi;
                    const V3<T> hcen = mk(sgp[0], sgp[1], sgp[2]);
                    const MatT<T> m = q.mats[hi];
                    const V3<T> loc = mk(o.x + d.x * t, o.y + d.y * t, o.z + d.z * t);   // at_t
                    const V3<T> vec = sub(loc, hcen);
                    const V3<T> u = dvs(vec, sqrt_len(pk_len2(vec)));
                    const bool front = pk_dot(d, u) < T(0.0);
                    nrm = front ? u : neg(u);
                    // the attenuation the path takes at bounce 0 (Material::get_hit_result): a Dielectric's is 1
                    if (m.kind != RT_DIELECTRIC) alb = mk(m.p[0], m.p[1], m.p[2]);
                    dep = t;
                }
                if (v) {
                    acc[0] += (double)alb.x; acc[1] += (double)alb.y; acc[2] += (double)alb.z;
                    acc[3] += (double)nrm.x; acc[4] += (double)nrm.y; acc[5] += (double)nrm.z;
                    acc[6] += (double)dep;
                    acc[7] += hit ? 1.0 : 0.0;
                }
            }
#pragma unroll
            for (uint32_t ch = 0; ch < kGuideCh; ++ch) acc[ch] = guide_fold(acc[ch]);
        }
        if (lane == 0) {
            const double n = (double)spp;
            if (gp.albedo) {
                float* a = gp.albedo + (size_t)3 * item;
                a[0] = (float)(acc[0] / n); a[1] = (float)(acc[1] / n); a[2] = (float)(acc[2] / n);
            }
            if (gp.normal) {
                float* a = gp.normal + (size_t)3 * item;
                a[0] = (float)(acc[3] / n); a[1] = (float)(acc[4] / n); a[2] = (float)(acc[5] / n);
            }
            if (gp.depth) gp.depth[item] = (float)(acc[6] / n);
            if (gp.coverage) gp.coverage[item] = (float)(acc[7] / n);
        }
    }
    if (lane == 0) {
        const auto& q = *cold_args<T>();
        unsigned long long* cc = &q.segs[(gw & (kSegShards - 1)) * kSegStride];
        if (n_seg) atomicAdd(cc + 0, n_seg);
        if (n_slots) atomicAdd(cc + 1, n_slots);
        for (uint32_t i = 0; i < kNWork; ++i)
            if (g_work[wave][i]) atomicAdd(cc + kWorkSlot + i, g_work[wave][i]);
#ifdef RT_KSTATS
        for (int i = 0; i < kNKstat; ++i) atomicAdd(cc + kstat_slot(i), g_kst[wave][i]);
#endif
    }
}

}  // namespace rt
