// rt_step.hpp — path steps for integrators driven by the caller: the material stage alone (rt_scatter_async) and the
// closest hit plus the material stage in one kernel (rt_path_step_async).  Two kernels over the render's own
// next_ray<T, false>(cam = false, ...): PackedHitRecords::finalize (objects.rs:157-162), then
// Material::get_hit_result (materials.rs:54-147) with its one draw from stream 2 at counter (sample, pixel, bounce).
//   * scatter_rays<T>: a map kernel, one thread per ray.  A ray with index[i] >= 0 becomes its scattered ray (origin:
//     the hit point; direction: not normalised; colour *= attenuation); any other ray is copied through bit for bit.
//   * path_step_rays<T, ROOT2, MEGA>: query_rays' mapping (the lane is the ray, a batch is 64 consecutive rays, the
//     waves stride over the batches), its validity test and nearest_hit (the general sweep, as trace_paths_rays runs it
//     every bounce), then the lanes with a hit go through next_ray.  Nothing goes to memory between the sweep and the
//     scatter: the ray is in registers.  Per ray it computes what query_rays followed by scatter_rays computes.
// next_ray gathers cen[4 hit_i] and mats[hit_i] before anything else, so a lane enters it only with an index inside
// the scene: a miss (-1), an invalid ray (-2), an index >= n_spheres and a sample >= 2^20 (the fp32 counter holds 20
// bits of it) stay outside; the last two also set word 1 of the error flags (RT_ERR_INVALID at rt_context_collect).
// Both argument structs start with KParams, so cold_args<T>() reads the tables and the key from the same kernarg
// offsets.
#pragma once
#include "rt_sweep.hpp"
#include "rt_camera.hpp"
#include "rt_query.hpp"

namespace rt {

constexpr uint32_t kStepSampleEnd = 1u << 20;   // samples a draw's counter can tell apart (rt_device.hpp rng)
constexpr uint8_t kStepMissed = RT_STEP_MISSED, kStepScattered = RT_STEP_SCATTERED, kStepInvalid = RT_STEP_INVALID;

// Arguments of scatter_rays: n_items: the rays; center: the shared origin; k0, k1: the key.
template <typename T> struct ScParams {
    KParams<T> k;
    const T* origins;        // [n][3]; NULL: the shared origin k.center
    const T* directions;     // [n][3]
    const int32_t* index;    // [n], as query_rays writes it
    const T* t;              // [n]
    const uint32_t* pixel;   // [n]
    const uint32_t* sample;  // [n]
    uint32_t bounce;
    T* colour;               // [n][3], in place; NULL: no colour is tracked
    T* out_origins;          // [n][3]; may be origins; NULL: not written
    T* out_directions;       // [n][3]; may be directions; NULL: not written
};

// Arguments of path_step_rays: the rays and the colour are updated in place; any of the query's outputs may be NULL.
template <typename T> struct PsParams {
    KParams<T> k;
    T* origins;              // [n][3]
    T* directions;           // [n][3]
    T* colour;               // [n][3]; NULL: no colour is tracked
    const uint32_t* pixel;   // [n]
    const uint32_t* sample;  // [n]
    uint32_t bounce;
    uint8_t* status;         // [n]: kStepScattered, kStepMissed (not scattered), kStepInvalid
    int32_t* index;          // [n]
    T* t;                    // [n]
    T* normal;               // [n][3]
    uint8_t* front;          // [n]
};

// May the lane enter next_ray with this hit?  Otherwise it is left as it came; bad: it also raises the error flag.
__device__ __forceinline__ bool step_scatters(int hit_i, uint32_t sample, uint32_t n_spheres, bool& bad) {
    const bool hit = hit_i >= 0;
    const bool ok = (uint32_t)hit_i < n_spheres && sample < kStepSampleEnd;   // a negative index is above n_spheres
    bad = hit && !ok;
    return hit && ok;
}

template <typename T>
__global__ __launch_bounds__(256) void scatter_rays(ScParams<T> sp) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n = cold_args<T>()->n_items;   // <= 0x7FFFFFFF rays
    const uint32_t ray = blockIdx.x * 256u + threadIdx.x;   // < n + 256
    const bool in = ray < n;
    V3<T> o = mk(T(0), T(0), T(0)), d = o, c = mk(T(1.0), T(1.0), T(1.0));
    int hi = -1;
    uint32_t sid = 0, pix = 0;
    T ht = T(0);
    if (in) {
        const T* dp = sp.directions + (size_t)3 * ray;
        d = mk(dp[0], dp[1], dp[2]);
        if (sp.origins == nullptr) {   // wave-uniform
            const auto& q = *cold_args<T>();
            o = mk(q.center[0], q.center[1], q.center[2]);
        } else {
            const T* op = sp.origins + (size_t)3 * ray;
            o = mk(op[0], op[1], op[2]);
        }
        hi = sp.index[ray];
        ht = sp.t[ray];
        pix = sp.pixel[ray];
        sid = sp.sample[ray];
        if (sp.colour) {
            const T* cp = sp.colour + (size_t)3 * ray;
            c = mk(cp[0], cp[1], cp[2]);
        }
    }
    bool bad = false;
    const bool go = in && step_scatters(hi, sid, cold_args<T>()->n_spheres, bad);
    if (go) {
        next_ray<T, false>(false, 0u, 0u, pix, sid, sp.bounce, hi, ht, o, d, c);
        if (sp.colour) {
            T* cp = sp.colour + (size_t)3 * ray;
            cp[0] = c.x; cp[1] = c.y; cp[2] = c.z;
        }
    }
    if (in) {   // a ray that was not scattered: its inputs, bit for bit
        if (sp.out_origins) {
            T* op = sp.out_origins + (size_t)3 * ray;
            op[0] = o.x; op[1] = o.y; op[2] = o.z;
        }
        if (sp.out_directions) {
            T* dp = sp.out_directions + (size_t)3 * ray;
            dp[0] = d.x; dp[1] = d.y; dp[2] = d.z;
        }
    }
    const unsigned long long gm = __ballot(go), bm = __ballot(bad);
    if (lane == 0 && (gm | bm) != 0ull) {
        const auto& q = *cold_args<T>();
        const uint32_t gw = ray >> 6;
        if (gm) atomicAdd(&q.segs[(gw & (kSegShards - 1)) * kSegStride + kQuerySlot], (unsigned long long)__builtin_popcountll(gm));
        if (bm) atomicOr(q.err + 1, 1u);
    }
}

template <typename T, bool ROOT2, bool MEGA>
__global__ __launch_bounds__(256, kWavesQuery<T>) void path_step_rays(PsParams<T> pp) {
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
    bool any_bad = false;
    for (uint32_t batch = gw; batch < n_batches; batch += nw) {
        const uint32_t ray = batch * 64u + lane;   // <= 0x7FFFFFFF + 63
        const bool in = ray < n;
        V3<T> o = mk(T(0), T(0), T(0)), d = o;
        if (in) {
            const T* dp = pp.directions + (size_t)3 * ray;
            d = mk(dp[0], dp[1], dp[2]);
            const T* op = pp.origins + (size_t)3 * ray;
            o = mk(op[0], op[1], op[2]);
        }
        const T a = pk_len2(d);
        const bool v = in && query_finite(o) && query_finite(d) && a >= kQueryLen2Min<T> && a <= kQueryLen2Max<T>;
        const unsigned long long vm = __ballot(v);
        T t = T(INFINITY);
        int hi = -1;
        if (vm != 0ull) {   // wave-uniform
            if (v) hi = nearest_hit<T, ROOT2, false, MEGA>(o, d, t);
            n_slots += 64u;
            n_seg += (unsigned long long)__builtin_popcountll(vm);
        }
        const bool hit = v && hi >= 0;
        if (hit) {
            // the query's outputs of the hit that is scattered: PackedHitRecords::finalize as query_rays has it
            // (next_ray below runs the same operations for its own use)
            const auto& q = *cold_args<T>();
            const T* sgp = q.cen + 4 * hi;
            const V3<T> hcen = mk(sgp[0], sgp[1], sgp[2]);
            const V3<T> loc = mk(o.x + d.x * t, o.y + d.y * t, o.z + d.z * t);   // at_t
            const V3<T> vec = sub(loc, hcen);
            const V3<T> u = dvs(vec, sqrt_len(pk_len2(vec)));
            const bool front = pk_dot(d, u) < T(0.0);
            const V3<T> nrm = front ? u : neg(u);
            if (pp.normal) {
                T* np = pp.normal + (size_t)3 * ray;
                np[0] = nrm.x; np[1] = nrm.y; np[2] = nrm.z;
            }
            if (pp.front) pp.front[ray] = front ? 1u : 0u;
        } else if (in) {
            if (pp.normal) {
                T* np = pp.normal + (size_t)3 * ray;
                np[0] = T(0); np[1] = T(0); np[2] = T(0);
            }
            if (pp.front) pp.front[ray] = 0u;
        }
        if (in) {
            if (pp.t) pp.t[ray] = v ? (hit ? t : T(INFINITY)) : T(NAN);
            if (pp.index) pp.index[ray] = v ? (hit ? hi : -1) : kQueryInvalid;
        }
        bool bad = false;
        const bool go = hit && step_scatters(hi, pp.sample[ray], cold_args<T>()->n_spheres, bad);
        any_bad = any_bad || bad;
        if (go) {
            V3<T> c = mk(T(1.0), T(1.0), T(1.0));
            if (pp.colour) {
                const T* cp = pp.colour + (size_t)3 * ray;
                c = mk(cp[0], cp[1], cp[2]);
            }
            next_ray<T, false>(false, 0u, 0u, pp.pixel[ray], pp.sample[ray], pp.bounce, hi, t, o, d, c);
            T* op = pp.origins + (size_t)3 * ray;
            op[0] = o.x; op[1] = o.y; op[2] = o.z;
            T* dp = pp.directions + (size_t)3 * ray;
            dp[0] = d.x; dp[1] = d.y; dp[2] = d.z;
            if (pp.colour) {
                T* cp = pp.colour + (size_t)3 * ray;
                cp[0] = c.x; cp[1] = c.y; cp[2] = c.z;
            }
        }
        if (in && pp.status) pp.status[ray] = v ? (go ? kStepScattered : kStepMissed) : kStepInvalid;
    }
    const unsigned long long bm = __ballot(any_bad);
    if (lane == 0) {
        const auto& q = *cold_args<T>();
        unsigned long long* cc = &q.segs[(gw & (kSegShards - 1)) * kSegStride];
        if (n_seg) {
            atomicAdd(cc + 0, n_seg);
            atomicAdd(cc + kQuerySlot, n_seg);
        }
        if (n_slots) atomicAdd(cc + 1, n_slots);
        if (bm) atomicOr(q.err + 1, 1u);
        for (uint32_t i = 0; i < kNWork; ++i)
            if (g_work[wave][i]) atomicAdd(cc + kWorkSlot + i, g_work[wave][i]);
#ifdef RT_KSTATS
        for (int i = 0; i < kNKstat; ++i) atomicAdd(cc + kstat_slot(i), g_kst[wave][i]);
#endif
    }
}

}  // namespace rt
