// rt_query.hpp — ray queries (rt_query_hits_async): the closest hit of caller-supplied rays, for picking, camera
// models the reference lacks, occlusion passes over first hits and integrators driven from the host's own tensors.
// One kernel, query_rays<T, ROOT2, SHARED, MEGA>: the live path's closest hit through the sweeps the trace kernels
// run (nearest_hit for rays with origins of their own, camera_sweep over the camera tables of a shared origin),
// then PackedHitRecords::finalize (objects.rs:157-162) as guide_pixels has it, and plain vector stores.  It stops
// there: no scatter, no records, no reduction.  occlusion_rays<T, ROOT2, MEGA> (rt_query_occluded_async, at the end of
// this file) answers "is anything in the way before t_max" under the same mapping and precondition.
//
// Mapping: the lane is the ray, a batch is 64 consecutive rays, and the waves stride over the batches.  A ray
// outside the precondition (include/rt_mi355x.h: a non-finite component, or |d|^2 outside [1e-6, 1e6], the range
// tests/test_gpu_cull_probe.py has proven the culls for) is not traced: it does not enter nearest_hit, and it is
// an idle lane (v = false) of camera_sweep, whose cone takes its axis from the first valid lane; a batch without a
// valid lane skips the sweep.
#pragma once
#include "rt_sweep.hpp"
#include "rt_camera.hpp"

namespace rt {

// Arguments of query_rays: KParams first, so cold_args<T>() reads it from the same kernarg offsets (n_items: the
// rays; center: the shared origin, with the camera tables built for it), then the rays and the outputs (any output
// may be NULL).
template <typename T> struct QParams {
    KParams<T> k;
    const T* origins;      // [n][3]; NULL under SHARED (k.center)
    const T* directions;   // [n][3]
    T* t;                  // [n]
    int32_t* index;        // [n]
    T* normal;             // [n][3]
    T* point;              // [n][3]
    uint8_t* front;        // [n]
};

// Waves per SIMD the register allocation targets: the guide kernel's (the same sweeps, the same finalize).
template <typename T> constexpr int kWavesQuery = sizeof(T) == 4 ? 5 : 4;
// Shard slot of the rays traced (rt_stats.samples of a query: the host cannot know how many rays were valid).
constexpr int kQuerySlot = 22;
static_assert(kQuerySlot >= kKstatSlot2 + (kNKstat - kNKstat1) && kQuerySlot < kSegStride, "the query's counter over another's slot");
constexpr int kQueryInvalid = RT_QUERY_INVALID;

// |d|^2 the culls are proven for, in T (the decimal constants rounded to T).
template <typename T> constexpr T kQueryLen2Min = T(1e-6);
template <typename T> constexpr T kQueryLen2Max = T(1e6);

template <typename T> __device__ __forceinline__ bool query_finite(const V3<T>& a) {
    return (a.x - a.x == T(0)) & (a.y - a.y == T(0)) & (a.z - a.z == T(0));   // inf - inf and NaN - NaN are NaN
}

template <typename T, bool ROOT2, bool SHARED, bool MEGA>
__global__ __launch_bounds__(256, kWavesQuery<T>) void query_rays(QParams<T> qp) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (lane < kNWork) g_work[wave][lane] = 0ull;
#ifdef RT_KSTATS
    if (lane < kNKstat) g_kst[wave][lane] = 0;
#endif
    const uint32_t gw = blockIdx.x * 4u + wave, nw = gridDim.x * 4u;
    const uint32_t n = cold_args<T>()->n_items;   // <= 0x7FFFFFFF rays
    const uint32_t n_batches = (n + 63u) / 64u;   // <= 2^25: batch + nw does not wrap
    unsigned long long n_seg = 0, n_slots = 0;
    for (uint32_t batch = gw; batch < n_batches; batch += nw) {
        const uint32_t ray = batch * 64u + lane;   // <= 0x7FFFFFFF + 63
        const bool in = ray < n;
        V3<T> o = mk(T(0), T(0), T(0)), d = o;
        if (in) {
            const T* dp = qp.directions + (size_t)3 * ray;
            d = mk(dp[0], dp[1], dp[2]);
            if constexpr (SHARED) {
                const auto& q = *cold_args<T>();
                o = mk(q.center[0], q.center[1], q.center[2]);
            } else {
                const T* op = qp.origins + (size_t)3 * ray;
                o = mk(op[0], op[1], op[2]);
            }
        }
        const T a = pk_len2(d);
        const bool v = in && query_finite(o) && query_finite(d) && a >= kQueryLen2Min<T> && a <= kQueryLen2Max<T>;
        const unsigned long long vm = __ballot(v);
        T t = T(INFINITY);
        int hi = -1;
        if (vm != 0ull) {   // wave-uniform
            if constexpr (SHARED) {
                hi = camera_sweep<T, ROOT2, false, MEGA>(v, d, t);   // whole wave: lanes are spheres in the cull
            } else {
                if (v) hi = nearest_hit<T, ROOT2, false, MEGA>(o, d, t);
            }
            n_slots += 64u;
            n_seg += (unsigned long long)__builtin_popcountll(vm);
        }
        const bool hit = v && hi >= 0;
        V3<T> nrm = mk(T(0), T(0), T(0)), loc = nrm;
        bool front = false;
        if (hit) {
            // PackedHitRecords::finalize (objects.rs:157-162), as guide_pixels has it
            const auto& q = *cold_args<T>();
            const T* sgp = q.cen + 4 * hi;
            const V3<T> hcen = mk(sgp[0], sgp[1], sgp[2]);
            loc = mk(o.x + d.x * t, o.y + d.y * t, o.z + d.z * t);   // at_t
            const V3<T> vec = sub(loc, hcen);
            const V3<T> u = dvs(vec, sqrt_len(pk_len2(vec)));
            front = pk_dot(d, u) < T(0.0);
            nrm = front ? u : neg(u);
        }
        if (in) {
            if (qp.t) qp.t[ray] = v ? (hit ? t : T(INFINITY)) : T(NAN);
            if (qp.index) qp.index[ray] = v ? (hit ? hi : -1) : kQueryInvalid;
            if (qp.normal) {
                T* np = qp.normal + (size_t)3 * ray;
                np[0] = nrm.x; np[1] = nrm.y; np[2] = nrm.z;
            }
            if (qp.point) {
                T* pp = qp.point + (size_t)3 * ray;
                pp[0] = loc.x; pp[1] = loc.y; pp[2] = loc.z;
            }
            if (qp.front) qp.front[ray] = front ? 1u : 0u;
        }
    }
    if (lane == 0) {
        const auto& q = *cold_args<T>();
        unsigned long long* cc = &q.segs[(gw & (kSegShards - 1)) * kSegStride];
        if (n_seg) {
            atomicAdd(cc + 0, n_seg);
            atomicAdd(cc + kQuerySlot, n_seg);
        }
        if (n_slots) atomicAdd(cc + 1, n_slots);
        for (uint32_t i = 0; i < kNWork; ++i)
            if (g_work[wave][i]) atomicAdd(cc + kWorkSlot + i, g_work[wave][i]);
#ifdef RT_KSTATS
        for (int i = 0; i < kNKstat; ++i) atomicAdd(cc + kstat_slot(i), g_kst[wave][i]);
#endif
    }
}

// ---- occlusion queries (rt_query_occluded_async): is anything in the way before t_max ----
// One kernel, occlusion_rays<T, ROOT2, MEGA>, under query_rays' mapping: one byte per ray, kOccluded* below.  A ray
// is valid under the query's precondition when its t_max is not NaN; a valid ray with t_max <= 0.001 has no
// accepted root below its bound and does not enter the sweep.  The others go through nearest_hit's any-hit variant
// (rt_sweep.hpp: the bound culls boxes from the first group, a lane is done at its first accepted hit, the wave
// leaves when every lane is).  Origins of their own or one shared origin (k.center), both through the general sweep.
// Arguments: KParams first, as QParams has it; t_max: per ray, or NULL for t_max_all.
template <typename T> struct OParams {
    KParams<T> k;
    const T* origins;      // [n][3]; NULL: the shared origin k.center
    const T* directions;   // [n][3]
    const T* t_max;        // [n]; NULL: t_max_all
    T t_max_all;
    uint8_t* occluded;     // [n]
};
constexpr uint8_t kOccludedNo = RT_OCCLUDED_NO, kOccludedYes = RT_OCCLUDED_YES, kOccludedInvalid = RT_OCCLUDED_INVALID;

template <typename T, bool ROOT2, bool MEGA>
__global__ __launch_bounds__(256, kWavesQuery<T>) void occlusion_rays(OParams<T> op) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (lane < kNWork) g_work[wave][lane] = 0ull;
#ifdef RT_KSTATS
    if (lane < kNKstat) g_kst[wave][lane] = 0;
#endif
    const uint32_t gw = blockIdx.x * 4u + wave, nw = gridDim.x * 4u;
    const uint32_t n = cold_args<T>()->n_items;   // <= 0x7FFFFFFF rays
    const uint32_t n_batches = (n + 63u) / 64u;   // <= 2^25: batch + nw does not wrap
    unsigned long long n_seg = 0, n_slots = 0;
    for (uint32_t batch = gw; batch < n_batches; batch += nw) {
        const uint32_t ray = batch * 64u + lane;   // <= 0x7FFFFFFF + 63
        const bool in = ray < n;
        V3<T> o = mk(T(0), T(0), T(0)), d = o;
        T tm = T(0);
        if (in) {
            const T* dp = op.directions + (size_t)3 * ray;
            d = mk(dp[0], dp[1], dp[2]);
            if (op.origins == nullptr) {   // wave-uniform
                const auto& q = *cold_args<T>();
                o = mk(q.center[0], q.center[1], q.center[2]);
            } else {
                const T* pp = op.origins + (size_t)3 * ray;
                o = mk(pp[0], pp[1], pp[2]);
            }
            tm = op.t_max != nullptr ? op.t_max[ray] : op.t_max_all;
        }
        const T a = pk_len2(d);
        const bool v = in && query_finite(o) && query_finite(d) && a >= kQueryLen2Min<T> && a <= kQueryLen2Max<T> && tm == tm;
        const bool go = v && tm > T(0.001);   // a root is accepted from 0.001 on: nothing lies below such a bound
        bool occ = false;
        if (__ballot(go) != 0ull) {   // wave-uniform
            if (go) {
                T t = tm;
                occ = nearest_hit<T, ROOT2, false, MEGA, true>(o, d, t) >= 0;
            }
            n_slots += 64u;
        }
        n_seg += (unsigned long long)__builtin_popcountll(__ballot(v));
        if (in) op.occluded[ray] = v ? (occ ? kOccludedYes : kOccludedNo) : kOccludedInvalid;
    }
    if (lane == 0) {
        const auto& q = *cold_args<T>();
        unsigned long long* cc = &q.segs[(gw & (kSegShards - 1)) * kSegStride];
        if (n_seg) {
            atomicAdd(cc + 0, n_seg);
            atomicAdd(cc + kQuerySlot, n_seg);
        }
        if (n_slots) atomicAdd(cc + 1, n_slots);
        for (uint32_t i = 0; i < kNWork; ++i)
            if (g_work[wave][i]) atomicAdd(cc + kWorkSlot + i, g_work[wave][i]);
#ifdef RT_KSTATS
        for (int i = 0; i < kNKstat; ++i) atomicAdd(cc + kstat_slot(i), g_kst[wave][i]);
#endif
    }
}

}  // namespace rt
