// rt_common.hpp — device-side building blocks shared by every stage of the megakernel: the scene's
// group layouts (scalar-cache loads), the kernel arguments, the executed-work counters and the
// two-deep scalar-load pipelines.  Part of the single translation unit rt_kernel.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <array>
#include <initializer_list>
#include <chrono>
#include <cmath>
#include <limits>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/rt_mi355x.h"
#include "rt_device.hpp"
#include "rt_formats.hpp"
#include "rt_experiments.hpp"

namespace rt {

// The scene's group layouts (kGroup, kBoxFloats) and MatT: rt_formats.hpp.
template <typename T> struct alignas(64) SphGroup { T v[64 / sizeof(T)]; };

// One 64-byte scalar load worth of spheres (s_load_dwordx16 into SGPRs).
template <typename T>
__device__ __forceinline__ SphGroup<T> load_group(const __attribute__((address_space(4))) T* f, uint32_t g) {
    constexpr int NE = 64 / sizeof(T);
    SphGroup<T> r;
#pragma unroll
    for (int e = 0; e < NE; ++e) r.v[e] = f[g * NE + e];
    return r;
}

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float F4 __attribute__((ext_vector_type(4)));
struct Q4 { uint32_t x, y, z, w; };

// One top group of the general sweep (kBoxFloats floats; layout at rt_formats.hpp).
struct alignas(32) BoxGroup { float v[kBoxFloats]; };
__device__ __forceinline__ BoxGroup load_box(const __attribute__((address_space(4))) float* f, uint32_t g) {
    BoxGroup r;
#pragma unroll
    for (uint32_t e = 0; e < kBoxFloats; ++e) r.v[e] = f[g * kBoxFloats + e];
    return r;
}
__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

template <typename T> struct KParams {
    // rsv0 .. rsv6: the places of seven members that fed the camera-origin sweep (removed with it; nothing sets
    // or reads them: they are the zeros of context_params' memset).  They stay so that every other member keeps
    // its kernarg offset: without them 104 of the 109 kernels other than build_cam_table compile to other code
    // (scalar loads pair up differently, SGPR spill counts move: profiles/r12/dead_camt.txt).  Compacting the
    // struct is a performance experiment.
    const T* rsv0;
    const T* cen;              // [n][4] = cx, cy, cz, signed radius (AoS: finalize gather, build_cam_table)
    uint32_t rsv1;
    const MatT<T>* mats;       // [n] each sphere's material record, materials[material[i]] (one gather)
    uint32_t n_spheres;
    uint32_t W, H;
    double rW, rH;             // RN(1/W), RN(1/H) for div_dim (0: divide)
    T center[3], ulc[3], vu[3], vv[3], du[3], dv[3];
    uint32_t spp, P, C, depth, flags, s_sel, k0, k1;
    uint32_t row_begin, row_step, col_begin, col_count;
    uint8_t* rgb;
    double* lin;
    unsigned long long* segs;  // kSegShards shards of kSegStride counters (256 B per shard; direct_sky_samples at slot 16)
    uint32_t* err;
    uint32_t* counter;         // next block of work items (guided_block)
    uint32_t blk_g;            // largest block (a power of two <= kMaxBlock; claim_block)
    uint32_t n_items;
    char* scratch;             // per-wave scratch regions
    size_t scratch_stride;
    uint32_t vbytes, sbytes;   // trace_paths: position-map bytes, per-slot record bytes (WaveSlots)
    uint32_t swide;            // Records::wide
    const T* rsv2;
    const float* rsv3;
    const float* rsv4;
    uint32_t rsv5;
    float f_cmax, f_r2max;     // filter margin bounds: max |c|_1 and max r2f over non-exact spheres
    float rsv6;
    float f_ir2, f_hir2, f_isr; // 1/r2min, 0.5/r2min and 8 u/sqrt(r2min), rounded up (build_scene_image)
    const float* cull;         // camera cone-cull records {wx, wy, wz, rp} per slot of the sweep layout
    const float* cullc;        // ... and per cluster, then per super (build_cam_table)
    uint32_t n_clp, n_supc;    // cluster records (x64), super records after them (x64; 0: none)
    const T* camx;             // camera-origin table per sphere {ocx, ocy, ocz, c} (AoS; build_cam_table)
    // general sweep, two-level (build_layout / pack_sweep): slot-order exact and filter streams,
    // cluster bounds (fp32 groups of 4 {cx, cy, cz, R2}), slot -> scene index; n_top top groups,
    // n_xg leading groups of always-exact spheres, then cluster k at groups n_xg + 4k .. + 3
    const T* rsph;
    const float* rfsph;        // its fp32 filter groups, inline: cluster k's 4 groups at 16 n_xg + 96 k, then
                               // their 4 records {r^2 of the pairs (fp32 rays), 4 scene indices} (inline_stream)
    const float* ftop;
    const float* fsup;         // super boxes (4 clusters each), 4 per group
    const float* rflat;        // fp32 rays: one {cx, cy, cz, r^2} record per slot, ridx's order and length (pack_flat;
                               // fp64: NULL).  At the offset of the scene-frame mega boxes no kernel read any more
    uint32_t n_mg;             // mega groups (4 megas each), 0: no mega level
    // MEGA kernels: the sphere filter in cluster-local frames (pack_local): filter groups with centres
    // relative to their cluster's centre, inline with each cluster's records (rt_layout.hpp's inline_stream: the
    // scene indices, and the frame {Cx, Cy, Cz, Rc} / {r2max, 1/r2min} in the r^2 words of records 0 / 1)
    const float* lfsph;
    const float* lclb;         // ... the box levels in group-local frames (pack_local_boxes): per super its
    const float* lsup;         //     4 cluster boxes, per mega its 4 supers, per mega group its 4 megas
    const float* lmeg;
    const float* lgig;         //     and per giga group its 4 gigas (a giga: one mega group, 4 megas)
    uint32_t n_gg;             // giga groups (0: the megas are tested without the giga pre-test)
    float l_r2max, l_hir2, l_isr;   // their margin constants: max local r2f, 48 u 0.5 / min, 8 u / sqrt(min)
    // ... and the mega walk's order (<= 64 megas): a grid over the megas' union, per cell 4 u64 words
    // {touching, within 1/4 of a mega's size, within 1/2, 0} (pack_mega_tiers)
    const uint64_t* mtiers;
    float mt_lo[3], mt_inv;
    uint32_t mt_n[3];
    const uint32_t* ridx;
    uint32_t n_top, n_xg, n_xs;   // n_xs: always-exact spheres (the rest of their last group are dummies)
};
static_assert(sizeof(KParams<float>) == 520 && offsetof(KParams<float>, ridx) == 496 &&
              sizeof(KParams<double>) == 592 && offsetof(KParams<double>, ridx) == 568,
              "the kernel-argument layout the kernels were measured with (rsv0 .. rsv6 keep it)");

// Arguments of the sample-parallel kernels (trace_paths_split, finish_records): KParams first, so
// cold_args<T>() reads it from the same kernarg offsets, then what only they need.  n_items counts
// (pixel, sample sub-range) items there: item i is pixel i / nsub, samples [j S, min(spp, (j + 1) S)),
// j = i % nsub.  scratch / scratch_stride: finish_records' per-wave position maps.
template <typename T> struct SParams {
    KParams<T> k;
    char* rec;                 // record buffer: pixel x's region at x * k.sbytes (Records' y, c, e formats)
    uint32_t S, nsub;          // samples per item, items per pixel
    uint32_t n_pix;            // pixels of the rendered set (k.n_items / nsub)
};

// Arguments of a progressive session's kernels (trace_paths_window, finish_window;
// rt_progressive_extend_async): SParams first, at the same kernarg offsets, then the session's own.
//   * The trace launch covers the sample window [s_begin, s.k.spp) of every pixel: item i is pixel i / nsub and,
//     j = i % nsub, samples [max(s_begin, s_base + j S), min(s.k.spp, s_base + (j + 1) S)) (rt_progressive_plan.hpp).
//     Its s.k.P and s.k.sbytes are the session's capacity (the strides of a region).
//   * The finish launch reduces the prefix [0, s.k.spp): s.k.spp, P, C, s_sel, vbytes and bit 1 of swide are
//     the snapshot's, P_cap and s.k.sbytes the capacity's.
template <typename T> struct WParams {
    SParams<T> s;
    uint32_t s_begin, s_base;
    uint32_t P_cap;            // positions a region is laid out for: y[P_cap], c[P_cap], e[P_cap]
};

// Arguments of a session's per-pixel-count kernels (rt_progressive_extend_map_async): WParams first, at the
// same kernarg offsets, then one table in device memory.
//   * trace_paths_items: s.s.k.n_items records {pixel, first, end, 0} of 16 bytes; item i traces the samples
//     [first, end) of that pixel of the range.  No launch-wide sample count is read (S, nsub, s_begin, s_base and
//     s.s.k.spp are unused); s.s.k.P and s.s.k.sbytes are the capacity's.
//   * finish_window_list: s.s.n_pix pixel indices, the pixels that are reduced at the count in s.s.k (one launch
//     per distinct count).
struct MapItem { uint32_t pixel, first, end, pad; };
template <typename T> struct IParams {
    WParams<T> w;
    const MapItem* items;
};
template <typename T> struct LParams {
    WParams<T> w;
    const uint32_t* list;
};

// Arguments of the caller-ray kernel (trace_paths_rays, rt_rays.hpp; rt_render_rays_async): KParams first, at the
// same kernarg offsets (n_items: the pixels), then the caller's rays.  Pixel p's sample s starts as ray
// p R + s % R; its RNG pixel is pixel_base + p.
template <typename T> struct RParams {
    KParams<T> k;
    const T* origins;          // [n_items R][3]; NULL: one shared origin, k.center
    const T* directions;       // [n_items R][3], not normalised
    uint64_t* skip;            // bit p % 64 of word p / 64: pixel p has an invalid ray and is not traced (rays_validate)
    uint32_t R, pixel_base;
};

constexpr int kSegShards = 256;
constexpr uint32_t kFlagPinholeInternal = 0x80000000u;   // set by the host: defocus vectors are +-0
constexpr int kWavesF32 = 6;   // default min-waves-per-SIMD targets (measured sweep);
constexpr int kWavesF64 = 4;   // RT_WAVES (read per launch) selects another for the live-path kernels
constexpr int kWavesMegaF32 = 6;   // the mega-level kernels (config E; RT_WAVES=5 selects the W5 build)
// fp32 launches with fewer pixels than this per resident W6 wave run at W5: W6's extra waves then split
// the pixels thinner and the tail costs more than the occupancy gains.  tools/waves_ab.py with the claim
// streams (rt_trace.hpp), W6/W5 speed: C whole 1.058, 8-way shards (42 px per W6 wave) 1.032, 16-way
// (21) 0.971; B 4-way (37.5) 1.056, 8-way (18.8) 0.966.  (Round 3's one claim counter put the 8-way
// C shard on the other side.)
constexpr uint64_t kW6PixelsPerWave = 24;
// RT_WAVES=7 selects a 7-waves-per-SIMD fp32 live-path build (72 VGPRs; the LDS of 7 workgroups
// just fits): +2 % on C and D, but it spills ~7 VGPRs around every sweep, and the scratch lines
// (4 MB per XCD) push HBM writes from 23 to 41 B/sample, so the default stays at 6
template <typename T> constexpr int kWavesModes = sizeof(T) == 4 ? 6 : 4;   // ROOT2 and semantics modes
constexpr int kSegStride = 32;  // u64 per shard (256 B)

// Executed-work counters (product build): per wave, the wave-level tests the culls and
// exact tests actually run, one LDS add per sweep or camera batch, flushed to shard slots
// kWorkSlot.. at the end.  The host turns them into executed FLOP (rt_work_stats).
enum WorkCounter : uint32_t {
    kWBox = 0,      // general sweep: box groups tested (4 boxes, 18 v_pk_fma_f32)
    kWFilt = 1,     // general sweep: filter groups tested (4 spheres, 14 v_pk_fma_f32)
    kWExact = 2,    // general sweep: spheres through the reference's exact test (17 FLOP in T each); a per-lane
                    // step (nearest_hit's flush: each lane one sphere of its own) counts one
    kWCone = 3,     // camera sweep: cone tests (64 records per wave test, 23 fp32 FLOP)
    kWCExact = 4,   // camera sweep: exact tests from the camera-origin table (8 FLOP in T each)
    kNWork = 5,
};
constexpr int kWorkSlot = 11;   // shard slots 11..15 (kstats uses 3..10 and 17..21: kstat_slot, rt_experiments.hpp)
constexpr int kDirectSkySlot = 16;   // samples of pixels finished at claim time (rt_stats.direct_sky_samples)
static_assert(kWorkSlot + kNWork <= kDirectSkySlot && kDirectSkySlot < kSegStride, "counters past the shard's slots");
static_assert(kKstatSlot >= 3 && kKstatSlot + kNKstat1 <= kWorkSlot && kKstatSlot2 > kDirectSkySlot &&
              kKstatSlot2 + (kNKstat - kNKstat1) <= kSegStride, "kstats counters over another counter's slot");
// u64: a wave of a persistent launch can run billions of tests (config E: ~1.3M filter groups per
// wave; spp up to 2^20 on a 4K frame is ~3000x that), past a u32.
__shared__ unsigned long long g_work[4][kNWork];
// Add wave-uniform counts from the first active lane (the caller may be inside a divergent branch).
__device__ __forceinline__ void work_add(uint32_t i, uint32_t n) {
    const uint32_t first = (uint32_t)__builtin_ctzll(__builtin_amdgcn_read_exec());
    if ((threadIdx.x & 63u) == first) atomicAdd(&g_work[threadIdx.x >> 6][i], (unsigned long long)n);
}


// #{set bits of m in the lanes below this one}: v_mbcnt_lo/hi, no lane mask held in VGPRs
__device__ __forceinline__ uint32_t lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Uniform (scalar-cache) view of a read-only kernel buffer: the sphere loop index is
// wave-uniform, so these become s_load into SGPRs — a free broadcast to all 64 lanes.
template <typename T> using cptr = const __attribute__((address_space(4))) T*;

// Cold kernel arguments (the camera) are read through an opaque pointer to the kernarg segment
// at their point of use: otherwise the backend hoists every kernarg load to the kernel entry and
// keeps ~40 camera SGPRs live across the whole persistent loop (SGPR spills into VGPR lanes).
// P: the kernel's argument struct, or one it starts with (every struct above begins with KParams<T>).
template <typename P> __device__ __forceinline__ cptr<P> cold() {
    cptr<P> k = (cptr<P>)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(k));
    return k;
}
template <typename T> __device__ __forceinline__ cptr<KParams<T>> cold_args() { return cold<KParams<T>>(); }
// Same, but ordered after `dep` is computed: loads through it cannot be hoisted above that value's
// producer (used to keep the camera constants out of SGPRs while a Philox block is in flight).
template <typename T> __device__ __forceinline__ cptr<KParams<T>> cold_args_after(uint32_t dep) {
    cptr<KParams<T>> k = (cptr<KParams<T>>)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(k) : "v"(dep));
    return k;
}

// x / W for the camera's pixel coordinate (ray_tracing.rs:78-79), W the image width or height.
// fp32: RN_f(RN_d(x * RN_d(1/W))) == RN_f(x / W).  The double product is within 2^-52 relative of
// x / W; a quotient of a float by an integer W < 2^20 that is not a float midpoint lies at least
// 2^-25 / W (>= 2^-45) relative from every midpoint, and it is never one (an odd 25-bit mantissa
// times W has more than 24 significant bits).  3 ops instead of the ~10 of a correctly rounded fp32 divide.  The
// host sets r = 0 (plain division) for larger images; fp64 always divides.
template <typename T> __device__ __forceinline__ T div_dim(T x, uint32_t W, double r) {
    if constexpr (sizeof(T) == 4) {
        if (r != 0.0) return (float)((double)x * r);
    }
    return x / (T)W;
}

// Walk the sphere groups with a two-deep scalar-load pipeline over two SGPR buffers (no
// per-group SGPR copies).  Scalar loads return out of order, so any use waits lgkmcnt(0): the
// next group's load is pinned (sched_barrier) BEFORE the current group's math and waited right
// after it, so it is always one whole group of VALU work old when it is consumed.  The device
// buffer holds a dummy group past the end, so the prefetches never need clamping.
// The same two-deep pipeline over the general sweep's box groups (cluster bounds).
template <typename F>
__device__ __forceinline__ void box_loop(cptr<float> f, uint32_t ng, F&& group) {
    BoxGroup A = load_box(f, 0);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_sched_barrier(0);
    uint32_t g = 0;
    for (; g + 1 < ng; g += 2) {
        const BoxGroup B = load_box(f, g + 1);
        __builtin_amdgcn_sched_barrier(0);
        group(A, g);
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_sched_barrier(0);
        A = load_box(f, g + 2);
        __builtin_amdgcn_sched_barrier(0);
        group(B, g + 1);
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (g < ng) group(A, g);
}

// A box group in a group-local frame (MEGA kernels, pack_local_boxes): 24 floats of boxes (BoxGroup
// layout), then the frame {Sx, Sy, Sz, Rg}, padded to 128 bytes (two s_load_dwordx16).
struct alignas(64) LBoxGroup { float v[32]; };
__device__ __forceinline__ LBoxGroup load_lbox(const __attribute__((address_space(4))) float* f, uint32_t g) {
    LBoxGroup r;
#pragma unroll
    for (uint32_t e = 0; e < 28; ++e) r.v[e] = f[g * 32u + e];
    return r;
}
template <typename F>
__device__ __forceinline__ void lbox_loop(cptr<float> f, uint32_t ng, F&& group) {
    LBoxGroup A = load_lbox(f, 0);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_sched_barrier(0);
    uint32_t g = 0;
    for (; g + 1 < ng; g += 2) {
        const LBoxGroup B = load_lbox(f, g + 1);
        __builtin_amdgcn_sched_barrier(0);
        group(A, g);
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_sched_barrier(0);
        A = load_lbox(f, g + 2);
        __builtin_amdgcn_sched_barrier(0);
        group(B, g + 1);
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (g < ng) group(A, g);
}

template <typename T, typename F>
__device__ __forceinline__ void sphere_loop(cptr<T> f, uint32_t ng, F&& group) {
    SphGroup<T> A = load_group(f, 0);
    // Wait for the first group here: otherwise the loop header inherits its pending load and the
    // compiler's wait before the first use also waits for the group just prefetched in the body.
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_sched_barrier(0);
    uint32_t g = 0;
    for (; g + 1 < ng; g += 2) {
        const SphGroup<T> B = load_group(f, g + 1);
        __builtin_amdgcn_sched_barrier(0);
        group(A, g);
        __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): B has landed
        __builtin_amdgcn_sched_barrier(0);
        A = load_group(f, g + 2);
        __builtin_amdgcn_sched_barrier(0);
        group(B, g + 1);
        __builtin_amdgcn_s_waitcnt(0xC07F);   // A has landed
        __builtin_amdgcn_sched_barrier(0);
    }
    if (g < ng) group(A, g);
}

}  // namespace rt
