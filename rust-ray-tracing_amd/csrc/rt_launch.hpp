// rt_launch.hpp — the launches of the C ABI, host only: what the launches of a context share (LaunchContext),
// the kernel selection and rt_stats.kernel_id, the steps of a launch (context_params, frame_params,
// ensure_cam_tables, frame_setup, plan_grid) and the launchers (launch_plain, launch_split, launch_window,
// launch_guides, launch_query, launch_occlusion, launch_scatter, launch_step, launch_step_list, launch_compact,
// launch_rays), between begin_launch and end_launch.
#pragma once
#include "rt_trace.hpp"
#include "rt_guides.hpp"
#include "rt_query.hpp"
#include "rt_step.hpp"
#include "rt_list.hpp"
#include "rt_rays.hpp"
#include "rt_host.hpp"
#include "rt_split_plan.hpp"
#include "rt_progressive_plan.hpp"

namespace rt {

// What the launches of a context share; rt_context (rt_kernel.hip) adds the progressive session.
struct LaunchContext {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_first = nullptr, ev_last = nullptr;
    bool have_first = false;
    // the scene: the tables of each precision, what both share, and the image's counts
    DeviceScene<float> d32;
    DeviceScene<double> d64;
    DeviceBuffer ridx, mtiers;   // slot -> scene index; the mega walk's order table (pack_mega_tiers)
    SceneCounts n;
    bool has_scene = false;   // rt_context_set_scene has succeeded since the context was made
    template <typename T> DeviceScene<T>& scene() {
        if constexpr (sizeof(T) == 8) return d64; else return d32;
    }
    DeviceBuffer segs, err;
    DeviceBuffer counter;   // persistent-kernel claim-stream counters (zeroed before each launch)
    DeviceBuffer scratch;   // per-wave ray state (grown on demand)
    DeviceBuffer records;   // the sample-parallel path's record buffer (grown on demand)
    DeviceBuffer rayskip;   // rt_render_rays_async: one bit per pixel, set where a ray is invalid (grown on demand)
    DeviceBuffer ballots, tiles;   // ray lists: a 64-bit survivor word per batch, a sum per tile (grown on demand)
    int n_cu = 0;
    uint64_t samples = 0, pixels = 0;
    hipStream_t last_stream = nullptr;   // stream of the previous render (they share scratch and tables)
    bool have_last = false;
    uint32_t last_kernel_id = 0, last_wg_per_cu = 0;   // rt_stats.kernel_id / kernel_wg_per_cu of the last launch
};

// ---- rt_stats.kernel_id (RT_KERNEL_* in rt_mi355x.h): a bit field per template argument, a bit per kernel family ----
constexpr uint32_t kKernelRoot2Bit = 1u << 4, kKernelCamqBit = 1u << 7, kKernelMegaBit = 1u << 8;
constexpr uint32_t kKernelSplitBit = 1u << 9;     // the sample-parallel kernels (a render's and a session's)
constexpr uint32_t kKernelItemsBit = 1u << 10;    // with kKernelSplitBit: a session's item-table kernel
constexpr uint32_t kKernelGuidesBit = 1u << 11;   // guide_pixels
constexpr uint32_t kKernelQueryBit = 1u << 12;    // query_rays (its SHARED takes the camera-batch bit)
constexpr uint32_t kKernelRaysBit = 1u << 13;     // trace_paths_rays
constexpr uint32_t kKernelOcclusionBit = 1u << 14;   // occlusion_rays
constexpr uint32_t kKernelScatterBit = 1u << 16;   // scatter_rays (bit 15: any kernel)
constexpr uint32_t kKernelStepBit = 1u << 17;      // path_step_rays
constexpr uint32_t kKernelListBit = 1u << 18;      // with kKernelStepBit: path_step_list; alone: a list compaction
template <typename T>
constexpr uint32_t kernel_id(int W, bool root2, int mode, bool camq, bool mega, uint32_t family) {
    return 0x8000u | (sizeof(T) == 8 ? 1u : 0u) | ((uint32_t)W << 1) | (root2 ? kKernelRoot2Bit : 0u) |
           ((uint32_t)mode << 5) | (camq ? kKernelCamqBit : 0u) | (mega ? kKernelMegaBit : 0u) | family;
}

// The kernel instantiation for (flags, waves-per-SIMD target, camera batches, mega level).  W < 0:
// the defaults (RT_WAVES unset).  The mega level (scenes with more than 8 super groups) has its own
// live-path kernels (fp32 at 5 or 6 waves, default 6; fp64 at 4); at other W such scenes are swept
// from the super boxes (the same result, more box tests).  id: rt_stats.kernel_id (rt_mi355x.h).
template <typename T> struct KernelPick {
    void (*fn)(KParams<T>);
    uint32_t id;
    int W;
};
template <typename T, int W, bool ROOT2, int MODE, bool CAMQ, bool MEGA = false>
static KernelPick<T> kp() {
    return KernelPick<T>{trace_paths<T, W, ROOT2, MODE, CAMQ, MEGA>, kernel_id<T>(W, ROOT2, MODE, CAMQ, MEGA, 0u), W};
}
template <typename T, bool CAMQ>
static KernelPick<T> pick_kernel(uint32_t flags, int W, bool mega, bool big) {
    const bool r2 = (flags & RT_FLAG_ROOT2) != 0u;
    constexpr bool F32 = sizeof(T) == 4;
    constexpr int WM = kWavesModes<T>;
    if (flags & RT_FLAG_MODE_SCALAR) return kp<T, WM, false, kModeScalar, CAMQ>();
    if (flags & RT_FLAG_MODE_VECTORIZED3)
        return r2 ? kp<T, WM, true, kModeV3, CAMQ>() : kp<T, WM, false, kModeV3, CAMQ>();
    if (flags & RT_FLAG_MODE_VECTORIZED)
        return r2 ? kp<T, WM, true, kModeV1, CAMQ>() : kp<T, WM, false, kModeV1, CAMQ>();
    if (r2) return kp<T, WM, true, kModeV2, CAMQ>();
    if (mega) {
        const int Wm = W < 0 ? (F32 ? (big ? kWavesMegaF32 : 5) : kWavesF64) : W;
        if constexpr (F32) {
            if (Wm == 5) return kp<T, 5, false, kModeV2, CAMQ, true>();
            if (Wm == 6) return kp<T, 6, false, kModeV2, CAMQ, true>();
        } else {
            if (Wm == 4) return kp<T, 4, false, kModeV2, CAMQ, true>();
        }
    }
    if (W < 0) W = F32 ? (big ? kWavesF32 : 5) : kWavesF64;
    // RT_WAVES above what the kernel's LDS allows is clamped: fp32 6 (round 2's W7 build lost its
    // seventh workgroup to the camera lists and the parking: 5 resident), fp64 5 (its W6 build: 3)
    if constexpr (F32) {
        return W >= 6 ? kp<T, 6, false, kModeV2, CAMQ>() : W >= 5 ? kp<T, 5, false, kModeV2, CAMQ>()
                                                         : kp<T, 4, false, kModeV2, CAMQ>();
    } else {
        return W >= 5 ? kp<T, 5, false, kModeV2, CAMQ>() : kp<T, 4, false, kModeV2, CAMQ>();
    }
}

// The sample-parallel kernels (rt_render_split_async): trace_paths_split<T, W, CAMQ, MEGA> at one occupancy
// per precision, the one small launches take today (fp32 5 waves per SIMD, fp64 4), and finish_records<T>.
template <typename T> constexpr int kWavesSplit = sizeof(T) == 4 ? 5 : 4;
template <typename T> struct SplitPick {
    void (*fn)(SParams<T>);
    uint32_t id;
    int W;
};
template <typename T>
static SplitPick<T> pick_split(bool camq, bool mega) {
    constexpr int W = kWavesSplit<T>;
    void (*const fn)(SParams<T>) =
        with_bools([](auto cq, auto mg) { return trace_paths_split<T, W, cq.value, mg.value>; }, camq, mega);
    return SplitPick<T>{fn, kernel_id<T>(W, false, kModeV2, camq, mega, kKernelSplitBit), W};
}
// A progressive session's tracing kernels, at the same occupancy and under pick_split's id: trace_paths_window,
// and trace_paths_items over an item table (kKernelItemsBit in the id).
template <typename T>
static void (*pick_window(bool camq, bool mega))(WParams<T>) {
    return with_bools([](auto cq, auto mg) { return trace_paths_window<T, kWavesSplit<T>, cq.value, mg.value>; }, camq, mega);
}
template <typename T>
static void (*pick_items(bool camq, bool mega))(IParams<T>) {
    return with_bools([](auto cq, auto mg) { return trace_paths_items<T, kWavesSplit<T>, cq.value, mg.value>; }, camq, mega);
}
// The guide-buffer kernel (rt_render_guides_async): guide_pixels<T, CAMQ, MEGA>.
template <typename T>
static void (*pick_guides(bool camq, bool mega))(GParams<T>) {
    return with_bools([](auto cq, auto mg) { return guide_pixels<T, cq.value, mg.value>; }, camq, mega);
}
// The ray-query kernel (rt_query_hits_async): query_rays<T, ROOT2, SHARED, MEGA>.
template <typename T>
static void (*pick_query(bool root2, bool shared, bool mega))(QParams<T>) {
    return with_bools([](auto r2, auto sh, auto mg) { return query_rays<T, r2.value, sh.value, mg.value>; }, root2, shared, mega);
}
// The occlusion kernel (rt_query_occluded_async): occlusion_rays<T, ROOT2, MEGA>.
template <typename T>
static void (*pick_occlusion(bool root2, bool mega))(OParams<T>) {
    return with_bools([](auto r2, auto mg) { return occlusion_rays<T, r2.value, mg.value>; }, root2, mega);
}
// The fused path-step kernel (rt_path_step_async): path_step_rays<T, ROOT2, MEGA>.
template <typename T>
static void (*pick_step(bool root2, bool mega))(PsParams<T>) {
    return with_bools([](auto r2, auto mg) { return path_step_rays<T, r2.value, mg.value>; }, root2, mega);
}
// The list step's kernel (rt_path_step_list_async): path_step_list<T, ROOT2, MEGA>.
template <typename T>
static void (*pick_step_list(bool root2, bool mega))(PlParams<T>) {
    return with_bools([](auto r2, auto mg) { return path_step_list<T, r2.value, mg.value>; }, root2, mega);
}
// The caller-ray kernel (rt_render_rays_async): trace_paths_rays<T, W, ROOT2, MEGA> at the precision's default W.
template <typename T>
static void (*pick_rays(bool root2, bool mega))(RParams<T>) {
    return with_bools([](auto r2, auto mg) { return trace_paths_rays<T, kWavesRays<T>, r2.value, mg.value>; }, root2, mega);
}
constexpr uint64_t kScratchBudget = 24ull << 30;   // scratch (and record buffer) bytes a launch may ask for

// Resident waves of the sample-parallel kernels: 4-wave workgroups at their occupancy target on every CU.
static uint32_t split_waves(const LaunchContext* c, bool f32) {
    return (uint32_t)c->n_cu * 4u * (uint32_t)(f32 ? kWavesSplit<float> : kWavesSplit<double>);
}

// ---- the steps of a launch ----
// What an entry point asks a launch for.
struct FrameArgs {
    const rt_camera* cam;
    uint32_t depth, spp;
    uint64_t seed;
    uint32_t flags;
    rt_tile_range rg;
    void* rgb;
    void* lin;
};
// One extend of a progressive session (rt_progressive_plan.hpp).  The launch's spp is the session's new
// sample count: the trace kernel (trace) covers the window [s_begin, spp) on the item grid s_base + j S,
// nsub items per pixel, writing regions laid out for cap samples in rec, and finish_window (finish)
// reduces [0, spp).
struct SessionWindow {
    char* rec;
    uint32_t cap, s_begin, s_base, S, nsub;
    bool trace, finish;
};

// diagnostics (RT_FILTER_OFF, read at every launch): every general-sweep and camera-sweep group through the exact test
static bool filter_off_env() {
    const char* e = getenv("RT_FILTER_OFF");
    return e && atoi(e) != 0;
}

// The scene's tables, constants and counts, and the context's counters.
template <typename T>
static void context_params(LaunchContext* c, bool filter_off, KParams<T>& p) {
    memset(&p, 0, sizeof(p));
    scene_params(c->scene<T>(), c->n, c->ridx, c->mtiers, filter_off, p);
    p.segs = (unsigned long long*)c->segs.p;
    p.err = (uint32_t*)c->err.p;
    p.counter = (uint32_t*)c->counter.p;
}

// The RNG key of a seed.  fp64: Philox4x32-10 keyed by (seed lo, seed hi).  fp32: Philox2x32-10 has a 32-bit key,
// folded here as seed lo ^ fmix32(seed hi) (rng<float> reads k0 only): fmix32(0) = 0, so a seed below 2^32 keys as
// itself, and seeds such as (m << 32) | m no longer all key as 0.
template <typename T>
static void key_params(uint64_t seed, KParams<T>& p) {
    if (sizeof(T) == 8) { p.k0 = (uint32_t)seed; p.k1 = (uint32_t)(seed >> 32); }
    else { p.k0 = (uint32_t)seed ^ fmix32((uint32_t)(seed >> 32)); p.k1 = 0u; }
}

// The camera, the sample counts, the RNG key, the tile range and the outputs; n_items: one per pixel.
template <typename T>
static void frame_params(const FrameArgs& a, KParams<T>& p) {
    const rt_camera* cam = a.cam;
    p.W = cam->image_width; p.H = cam->image_height;
    p.rW = p.W < (1u << 20) ? 1.0 / (double)p.W : 0.0;   // div_dim
    p.rH = p.H < (1u << 20) ? 1.0 / (double)p.H : 0.0;
    for (int i = 0; i < 3; ++i) {
        p.center[i] = (T)cam->center[i]; p.ulc[i] = (T)cam->ulc[i]; p.vu[i] = (T)cam->vu[i];
        p.vv[i] = (T)cam->vv[i]; p.du[i] = (T)cam->du[i]; p.dv[i] = (T)cam->dv[i];
    }
    p.spp = a.spp;
    p.C = (a.spp + 3) / 4;
    p.P = 4 * p.C;
    p.depth = a.depth;
    p.flags = a.flags;
    {
        bool pinhole = true;
        for (int i = 0; i < 3; ++i) {
            if (p.du[i] != T(0) || p.dv[i] != T(0)) pinhole = false;
            if (p.center[i] == T(0) && std::signbit(p.center[i])) pinhole = false;
        }
        if (pinhole) p.flags |= kFlagPinholeInternal;
    }
    p.s_sel = (p.C - 1) % 2;   // ray_tracing.rs:486
    key_params(a.seed, p);
    const rt_tile_range& rg = a.rg;
    p.row_begin = rg.row_begin; p.row_step = rg.row_step; p.col_begin = rg.col_begin; p.col_count = rg.col_count;
    p.rgb = (uint8_t*)a.rgb;
    p.lin = (double*)a.lin;
    p.n_items = rg.row_count * rg.col_count;
    p.swide = paths_wide(p.P, a.depth);
    p.vbytes = paths_vbytes(p.P, p.swide, (a.flags & RT_FLAG_MODE_VECTORIZED3) != 0u);
    p.sbytes = paths_sbytes(p.P, sizeof(T), p.swide);
}

// Point p at the camera tables of this precision and rebuild them for p.center unless the last launch left them
// for the same key.
template <typename T>
static int ensure_cam_tables(LaunchContext* c, KParams<T>& p, uint32_t flags, bool filter_off, hipStream_t st) {
    DeviceScene<T>& d = c->scene<T>();
    cam_table_params(d, c->n, p);
    auto& ck = d.camkey;
    const uint32_t scalar = (flags & RT_FLAG_MODE_SCALAR) ? 1u : 0u;
    double cen[3] = {(double)p.center[0], (double)p.center[1], (double)p.center[2]};
    const bool same = ck.valid && ck.scalar == scalar && ck.off == (uint32_t)filter_off &&
                      memcmp(ck.center, cen, sizeof(cen)) == 0;   // bit for bit (-0 is not +0)
    if (same) return RT_OK;
    const int rc = launch_cam_table(d, c->n, c->ridx, p.center, scalar != 0u, filter_off, st);
    if (rc != RT_OK) return rc;
    ck.valid = true;
    ck.scalar = scalar;
    ck.off = (uint32_t)filter_off;
    memcpy(ck.center, cen, sizeof(cen));
    return RT_OK;
}

// What every launcher starts with: the kernel arguments of a frame with items_per_pixel work items per
// pixel (<= 0x7FFFFFFF items in all: the entry points check), and the camera tables where the frame's
// kernels run camera batches (camq).
template <typename T>
static int frame_setup(LaunchContext* c, const FrameArgs& a, uint32_t items_per_pixel, hipStream_t st, KParams<T>& p,
                       bool& camq) {
    const bool filter_off = filter_off_env();
    context_params(c, filter_off, p);
    frame_params(a, p);
    p.n_items *= items_per_pixel;
    camq = (p.flags & kFlagPinholeInternal) && a.depth >= 1u;
    return camq ? ensure_cam_tables(c, p, a.flags, filter_off, st) : RT_OK;
}

// G, the largest block of work items a wave claims at once: the largest power of two <= min(kMaxBlock,
// kBlockSamples / item_spp, items per wave / kBlockShare), raised to kClaimSpp / item_spp (claim rate,
// rt_trace.hpp) where the share bound would go under it.
static uint32_t claim_block(uint64_t n_items, uint64_t nblocks, uint32_t item_spp) {
    const uint64_t per_wave = n_items / (4u * nblocks);
    const uint64_t g = std::max<uint64_t>({1u, std::min<uint64_t>({(uint64_t)kMaxBlock, kBlockSamples / item_spp,
                                                                   per_wave / kBlockShare}),
                                           std::min<uint64_t>((uint64_t)kMaxBlock, (kClaimSpp + item_spp - 1) / item_spp)});
    uint32_t G = 1;
    while (2u * G <= g) G *= 2u;
    // diagnostics (tools/waves_ab.py --block): RT_BLOCK_G overrides the largest block (1..16, a power of two)
    const char* ge = getenv("RT_BLOCK_G");
    if (ge && atoi(ge) >= 1 && atoi(ge) <= (int)kMaxBlock && (atoi(ge) & (atoi(ge) - 1)) == 0) G = (uint32_t)atoi(ge);
    return G;
}

// Persistent grid of kernel kfn (built for kW waves per SIMD; id: rt_stats.kernel_id): as many 4-wave
// workgroups as stay resident, never more waves than work items; and the claim block for items of
// item_spp samples each.
static int plan_grid(LaunchContext* c, const void* kfn, int kW, uint32_t id, uint32_t n_items, uint32_t item_spp,
                     uint64_t& nblocks, uint32_t& blk_g) {
    int per_cu = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfn, 256, 0));
    if (per_cu < 1) per_cu = 1;
    // 4-wave workgroups: W waves per SIMD is W workgroups per CU.  Fewer means the kernel's LDS (or
    // registers) cut its occupancy below the target it was built for (kParkC takes fp32 W6 to 26.8 of the
    // 27.3 KB six workgroups allow): an error, in every build kind, so that neither the product nor an
    // A/B build is ever measured at an occupancy other than the one it names (rt_stats reports both).
    c->last_kernel_id = 0;   // 0: no kernel (ids have bit 15 set)
    c->last_wg_per_cu = 0;
    if (per_cu < kW)
        return fail(RT_ERR_UNSUPPORTED, std::string(RT_BUILD_KIND) + " build: " + std::to_string(per_cu) +
                                            " workgroups per CU resident, kernel built for " + std::to_string(kW) +
                                            " (its LDS or registers grew past the occupancy target)");
    c->last_kernel_id = id;   // only a kernel that passed the check is ever reported
    c->last_wg_per_cu = (uint32_t)per_cu;
    nblocks = (uint64_t)c->n_cu * (uint64_t)per_cu;
    const uint64_t need = ((uint64_t)n_items + 3) / 4;
    if (nblocks > need) nblocks = need;
    blk_g = claim_block(n_items, nblocks, item_spp);
    return RT_OK;
}

static int zero_claim_counters(LaunchContext* c, hipStream_t st) {
    HIPCHK(hipMemsetAsync(c->counter.p, 0, kStreams * kCtrStride * sizeof(uint32_t), st));
    return RT_OK;
}

// ---- the launchers ----
// trace_paths: one work item per pixel, every sample of it.
template <typename T>
static int launch_plain(LaunchContext* c, const FrameArgs& a, hipStream_t st) {
    KParams<T> p;
    bool camq = false;
    int rc = frame_setup(c, a, 1u, st, p, camq);
    if (rc != RT_OK) return rc;
    // Minimum waves per SIMD the register allocation targets.  RT_WAVES (4..7; read at every
    // launch, so one process can compare them) overrides it for the live-path kernels (pinhole and
    // defocus cameras); the ROOT2 and semantics-mode kernels always run at kWavesModes.
    const char* waves_env = getenv("RT_WAVES");
    const int W = waves_env && atoi(waves_env) > 0 ? atoi(waves_env) : -1;
    const bool big = (uint64_t)p.n_items >= kW6PixelsPerWave * 24u * (uint64_t)c->n_cu;   // 24 W6 waves per CU
    const KernelPick<T> pick =
        with_bools([&](auto cq) { return pick_kernel<T, cq.value>(a.flags, W, p.n_mg > 0, big); }, camq);
    uint64_t nblocks = 0;
    if ((rc = plan_grid(c, (const void*)pick.fn, pick.W, pick.id, p.n_items, a.spp, nblocks, p.blk_g)) != RT_OK) return rc;
    p.scratch_stride = (size_t)p.vbytes + (size_t)kSlots * p.sbytes;
    // Keep the scratch within a fixed budget: fewer resident waves for very large spp.
    const uint64_t max_blocks = kScratchBudget / (4 * p.scratch_stride);
    if (nblocks > max_blocks) nblocks = max_blocks > 0 ? max_blocks : 1;
    if ((rc = ensure_bytes(c->scratch, p.scratch_stride * nblocks * 4, st)) != RT_OK) return rc;
    p.scratch = (char*)c->scratch.p;
    if ((rc = zero_claim_counters(c, st)) != RT_OK) return rc;
    hipLaunchKernelGGL(pick.fn, dim3((uint32_t)nblocks), dim3(256), 0, st, p);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

// guide_pixels: the waves stride over the pixels of the range, each keeping a pixel for all its samples.  No
// scratch, no records, no claim counter; the frame is set up as a render's of one bounce, so the camera tables
// follow a render's rebuild rule.
template <typename T>
static int launch_guides(LaunchContext* c, const FrameArgs& a, float* albedo, float* normal, float* depth, float* coverage,
                         hipStream_t st) {
    KParams<T> p;
    bool camq = false;
    int rc = frame_setup(c, a, 1u, st, p, camq);
    if (rc != RT_OK) return rc;
    const bool mega = p.n_mg > 0;
    void (*const gfn)(GParams<T>) = pick_guides<T>(camq, mega);
    constexpr int W = kWavesGuide<T>;
    const uint32_t id = kernel_id<T>(W, false, kModeV2, camq, mega, kKernelGuidesBit);
    uint64_t nblocks = 0;
    if ((rc = plan_grid(c, (const void*)gfn, W, id, p.n_items, a.spp, nblocks, p.blk_g)) != RT_OK) return rc;
    GParams<T> gp;
    memset(&gp, 0, sizeof(gp));
    gp.k = p;
    gp.albedo = albedo;
    gp.normal = normal;
    gp.depth = depth;
    gp.coverage = coverage;
    hipLaunchKernelGGL(gfn, dim3((uint32_t)nblocks), dim3(256), 0, st, gp);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

// What rt_query_hits_async asks for: the rays (origins: device, per ray; or origin: host, shared) and the outputs.
struct QueryArgs {
    uint64_t n_rays;
    const void* origins;
    const double* origin;
    const void* directions;
    uint32_t flags;
    void *t, *index, *normal, *point, *front;
};

// query_rays: the waves stride over the batches of 64 consecutive rays.  No scratch, no records, no claim counter.
// A shared origin is a camera centre to the tables: KParams points at the camera tables of that origin, which are
// rebuilt under a render's key rule (so a later render with another centre rebuilds them in turn).  An origin that
// is not finite in T makes every ray invalid and no sweep runs: its tables are not built, and the key stays.
template <typename T>
static int launch_query(LaunchContext* c, const QueryArgs& a, hipStream_t st) {
    KParams<T> p;
    const bool filter_off = filter_off_env();
    context_params(c, filter_off, p);
    p.flags = a.flags;
    p.n_items = (uint32_t)a.n_rays;
    const bool shared = a.origin != nullptr, root2 = (a.flags & RT_FLAG_ROOT2) != 0u, mega = p.n_mg > 0;
    int rc = RT_OK;
    if (shared) {
        bool finite = true;
        for (int i = 0; i < 3; ++i) {
            p.center[i] = (T)a.origin[i];
            finite = finite && std::isfinite(p.center[i]);
        }
        if (finite && (rc = ensure_cam_tables(c, p, a.flags, filter_off, st)) != RT_OK) return rc;
    }
    void (*const qfn)(QParams<T>) = pick_query<T>(root2, shared, mega);
    constexpr int W = kWavesQuery<T>;
    const uint32_t id = kernel_id<T>(W, root2, kModeV2, shared, mega, kKernelQueryBit);
    const uint32_t n_batches = (uint32_t)((a.n_rays + 63u) / 64u);   // a wave's work item
    uint64_t nblocks = 0;
    if ((rc = plan_grid(c, (const void*)qfn, W, id, n_batches, 1u, nblocks, p.blk_g)) != RT_OK) return rc;
    QParams<T> qp;
    memset(&qp, 0, sizeof(qp));
    qp.k = p;
    qp.origins = (const T*)a.origins;
    qp.directions = (const T*)a.directions;
    qp.t = (T*)a.t;
    qp.index = (int32_t*)a.index;
    qp.normal = (T*)a.normal;
    qp.point = (T*)a.point;
    qp.front = (uint8_t*)a.front;
    hipLaunchKernelGGL(qfn, dim3((uint32_t)nblocks), dim3(256), 0, st, qp);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

// What rt_query_occluded_async asks for: a query's rays, a bound per ray (d_t_max) or one for all (t_max), one byte out.
struct OcclusionArgs {
    uint64_t n_rays;
    const void* origins;
    const double* origin;
    const void* directions;
    const void* d_t_max;
    double t_max;
    uint32_t flags;
    void* occluded;
};

// occlusion_rays: launch_query's grid.  A shared origin is rounded as a camera centre is and broadcast by the kernel;
// both origin forms run the general sweep, so no camera tables are built or read.
template <typename T>
static int launch_occlusion(LaunchContext* c, const OcclusionArgs& a, hipStream_t st) {
    KParams<T> p;
    context_params(c, filter_off_env(), p);
    p.flags = a.flags;
    p.n_items = (uint32_t)a.n_rays;
    if (a.origin) for (int i = 0; i < 3; ++i) p.center[i] = (T)a.origin[i];
    const bool root2 = (a.flags & RT_FLAG_ROOT2) != 0u, mega = p.n_mg > 0;
    void (*const ofn)(OParams<T>) = pick_occlusion<T>(root2, mega);
    constexpr int W = kWavesQuery<T>;
    const uint32_t id = kernel_id<T>(W, root2, kModeV2, false, mega, kKernelOcclusionBit);
    const uint32_t n_batches = (uint32_t)((a.n_rays + 63u) / 64u);   // a wave's work item
    uint64_t nblocks = 0;
    const int rc = plan_grid(c, (const void*)ofn, W, id, n_batches, 1u, nblocks, p.blk_g);
    if (rc != RT_OK) return rc;
    OParams<T> op;
    memset(&op, 0, sizeof(op));
    op.k = p;
    op.origins = (const T*)a.origins;
    op.directions = (const T*)a.directions;
    op.t_max = (const T*)a.d_t_max;
    op.t_max_all = (T)a.t_max;
    op.occluded = (uint8_t*)a.occluded;
    hipLaunchKernelGGL(ofn, dim3((uint32_t)nblocks), dim3(256), 0, st, op);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

// What rt_scatter_async asks for: a query's rays and its index and t, the draw's counter (pixel, sample, bounce) and
// seed, the colour (in place, may be NULL) and the scattered rays (may be the inputs).
struct ScatterArgs {
    uint64_t n_rays;
    const void* origins;
    const double* origin;
    const void* directions;
    const void *index, *t, *pixel, *sample;
    uint32_t bounce;
    uint64_t seed;
    uint32_t flags;
    void *colour, *out_origins, *out_directions;
};

// scatter_rays: a map kernel, one thread per ray.  No sweep: of the scene it reads the centre and material tables.
// The key is a render's (key_params); a shared origin is rounded as a camera centre is and broadcast by the kernel.
template <typename T>
static int launch_scatter(LaunchContext* c, const ScatterArgs& a, hipStream_t st) {
    ScParams<T> sp;
    memset(&sp, 0, sizeof(sp));
    context_params(c, filter_off_env(), sp.k);
    sp.k.flags = a.flags;
    sp.k.n_items = (uint32_t)a.n_rays;
    key_params(a.seed, sp.k);
    if (a.origin) for (int i = 0; i < 3; ++i) sp.k.center[i] = (T)a.origin[i];
    sp.origins = (const T*)a.origins;
    sp.directions = (const T*)a.directions;
    sp.index = (const int32_t*)a.index;
    sp.t = (const T*)a.t;
    sp.pixel = (const uint32_t*)a.pixel;
    sp.sample = (const uint32_t*)a.sample;
    sp.bounce = a.bounce;
    sp.colour = (T*)a.colour;
    sp.out_origins = (T*)a.out_origins;
    sp.out_directions = (T*)a.out_directions;
    c->last_kernel_id = kernel_id<T>(0, false, kModeV2, false, false, kKernelScatterBit);   // no occupancy target: W 0
    c->last_wg_per_cu = 0;
    hipLaunchKernelGGL(scatter_rays<T>, dim3((uint32_t)((a.n_rays + 255u) / 256u)), dim3(256), 0, st, sp);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

// What rt_path_step_async asks for: the rays and the colour (updated in place), the draw's counter and seed, and the
// outputs (any may be NULL).
struct StepArgs {
    uint64_t n_rays;
    void *origins, *directions, *colour;
    const void *pixel, *sample;
    uint32_t bounce;
    uint64_t seed;
    uint32_t flags;
    void *status, *index, *t, *normal, *front;
};

// path_step_rays: launch_query's grid for rays with origins of their own (the general sweep: no camera tables).
template <typename T>
static int launch_step(LaunchContext* c, const StepArgs& a, hipStream_t st) {
    KParams<T> p;
    context_params(c, filter_off_env(), p);
    p.flags = a.flags;
    p.n_items = (uint32_t)a.n_rays;
    key_params(a.seed, p);
    const bool root2 = (a.flags & RT_FLAG_ROOT2) != 0u, mega = p.n_mg > 0;
    void (*const sfn)(PsParams<T>) = pick_step<T>(root2, mega);
    constexpr int W = kWavesQuery<T>;
    const uint32_t id = kernel_id<T>(W, root2, kModeV2, false, mega, kKernelStepBit);
    const uint32_t n_batches = (uint32_t)((a.n_rays + 63u) / 64u);   // a wave's work item
    uint64_t nblocks = 0;
    const int rc = plan_grid(c, (const void*)sfn, W, id, n_batches, 1u, nblocks, p.blk_g);
    if (rc != RT_OK) return rc;
    PsParams<T> pp;
    memset(&pp, 0, sizeof(pp));
    pp.k = p;
    pp.origins = (T*)a.origins;
    pp.directions = (T*)a.directions;
    pp.colour = (T*)a.colour;
    pp.pixel = (const uint32_t*)a.pixel;
    pp.sample = (const uint32_t*)a.sample;
    pp.bounce = a.bounce;
    pp.status = (uint8_t*)a.status;
    pp.index = (int32_t*)a.index;
    pp.t = (T*)a.t;
    pp.normal = (T*)a.normal;
    pp.front = (uint8_t*)a.front;
    hipLaunchKernelGGL(sfn, dim3((uint32_t)nblocks), dim3(256), 0, st, pp);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

// A ray list in and out (rt_path_step_list_async, rt_ray_list_compact_async): any of the four may be NULL as the
// header says; keep: the compaction call's mask.
struct ListArgs {
    const void *list_in, *count_in;
    void *list_out, *count_out;
    const void* keep;
};

// Rays per tile of the compaction's scan: RT_LIST_TILE (64 .. 65536, a power of two; read at every call, any other
// value ignored), else kListTileDefault.  It changes no result.
static uint32_t list_tile_env() {
    const char* e = getenv("RT_LIST_TILE");
    const long v = e ? atol(e) : 0;
    return v >= 64 && v <= 65536 && (v & (v - 1)) == 0 ? (uint32_t)v : kListTileDefault;
}

// The compaction's arguments over a capacity of n rays, its two scratch buffers grown to that capacity.
static int compact_params(LaunchContext* c, uint64_t n, const ListArgs& l, hipStream_t st, LcParams& p) {
    const uint32_t tile = list_tile_env();
    const uint64_t n_batches = (n + 63u) / 64u, n_tiles = (n + tile - 1u) / tile;
    int rc = ensure_bytes(c->ballots, (size_t)n_batches * sizeof(unsigned long long), st);
    if (rc != RT_OK) return rc;
    if ((rc = ensure_bytes(c->tiles, (size_t)n_tiles * sizeof(uint32_t), st)) != RT_OK) return rc;
    memset(&p, 0, sizeof(p));
    p.n = (uint32_t)n;
    p.tile_batches = tile / 64u;
    p.list_in = (const uint32_t*)l.list_in;
    p.count_in = (const uint32_t*)l.count_in;
    p.keep = (const uint8_t*)l.keep;
    p.ballots = (unsigned long long*)c->ballots.p;
    p.tiles = (uint32_t*)c->tiles.p;
    p.list_out = (uint32_t*)l.list_out;
    p.count_out = (uint32_t*)l.count_out;
    p.err = (uint32_t*)c->err.p;
    return RT_OK;
}

// The three levels of the compaction over the ballots a producer left: the launches are what orders them.  The grids
// are sized for the capacity (the count stays on the device) and stride; a short list leaves most of them idle.
static int launch_scan(LaunchContext* c, const LcParams& p, hipStream_t st) {
    const uint64_t n_batches = ((uint64_t)p.n + 63u) / 64u, n_tiles = (n_batches + p.tile_batches - 1u) / p.tile_batches;
    const uint64_t cap = (uint64_t)c->n_cu * 8u;   // workgroups
    hipLaunchKernelGGL(list_tile_sums, dim3((uint32_t)std::min(n_tiles, cap)), dim3(256), 0, st, p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(list_scan_tiles, dim3(1), dim3(kListScanChunk), 0, st, p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(list_scatter, dim3((uint32_t)std::min((n_batches + 3u) / 4u, cap)), dim3(256), 0, st, p);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

// path_step_list over the capacity's batches (launch_step's grid), then the compaction where an output list is asked for.
template <typename T>
static int launch_step_list(LaunchContext* c, const StepArgs& a, const ListArgs& l, hipStream_t st) {
    KParams<T> p;
    context_params(c, filter_off_env(), p);
    p.flags = a.flags;
    p.n_items = (uint32_t)a.n_rays;
    key_params(a.seed, p);
    const bool root2 = (a.flags & RT_FLAG_ROOT2) != 0u, mega = p.n_mg > 0;
    void (*const sfn)(PlParams<T>) = pick_step_list<T>(root2, mega);
    constexpr int W = kWavesQuery<T>;
    const uint32_t id = kernel_id<T>(W, root2, kModeV2, false, mega, kKernelStepBit | kKernelListBit);
    const uint32_t n_batches = (uint32_t)((a.n_rays + 63u) / 64u);   // a wave's work item
    uint64_t nblocks = 0;
    int rc = plan_grid(c, (const void*)sfn, W, id, n_batches, 1u, nblocks, p.blk_g);
    if (rc != RT_OK) return rc;
    LcParams cp;
    memset(&cp, 0, sizeof(cp));
    if (l.list_out && (rc = compact_params(c, a.n_rays, l, st, cp)) != RT_OK) return rc;
    PlParams<T> lp;
    memset(&lp, 0, sizeof(lp));
    lp.s.k = p;
    lp.s.origins = (T*)a.origins;
    lp.s.directions = (T*)a.directions;
    lp.s.colour = (T*)a.colour;
    lp.s.pixel = (const uint32_t*)a.pixel;
    lp.s.sample = (const uint32_t*)a.sample;
    lp.s.bounce = a.bounce;
    lp.s.status = (uint8_t*)a.status;
    lp.s.index = (int32_t*)a.index;
    lp.s.t = (T*)a.t;
    lp.s.normal = (T*)a.normal;
    lp.s.front = (uint8_t*)a.front;
    lp.list_in = (const uint32_t*)l.list_in;
    lp.count_in = (const uint32_t*)l.count_in;
    lp.ballots = cp.ballots;   // NULL: no output list
    hipLaunchKernelGGL(sfn, dim3((uint32_t)nblocks), dim3(256), 0, st, lp);
    HIPCHK(hipGetLastError());
    return l.list_out ? launch_scan(c, cp, st) : RT_OK;
}

// keep_ballots, then the compaction.  The id is the list bit alone unless a kernel with an id of its own ran since the
// last collect.
static int launch_compact(LaunchContext* c, uint64_t n, const ListArgs& l, hipStream_t st) {
    LcParams cp;
    const int rc = compact_params(c, n, l, st, cp);
    if (rc != RT_OK) return rc;
    if (c->last_kernel_id == 0u) {
        c->last_kernel_id = 0x8000u | kKernelListBit;   // no precision, no occupancy target: F64 0, W 0
        c->last_wg_per_cu = 0;
    }
    const uint64_t n_batches = (n + 63u) / 64u;
    hipLaunchKernelGGL(keep_ballots, dim3((uint32_t)std::min((n_batches + 3u) / 4u, (uint64_t)c->n_cu * 8u)), dim3(256), 0, st, cp);
    HIPCHK(hipGetLastError());
    return launch_scan(c, cp, st);
}

// What rt_render_rays_async asks for: the rays (R per pixel; origins as a query's) and a render's outputs.
struct RayArgs {
    uint64_t n_pixels;
    uint32_t spp, R;
    const void* origins;
    const double* origin;
    const void* directions;
    uint32_t depth;
    uint64_t seed;
    uint32_t pixel_base, flags;
    void *rgb, *lin;
};

// rays_validate, then trace_paths_rays: one work item per pixel, every sample of it, as launch_plain has them.  The
// frame is a render's of one row of n_pixels columns under a camera that has only a centre (the shared origin,
// rounded as a camera centre is; unused with per-ray origins): frame_params sets the sample counts, the RNG key and
// the record layout.  No camera tables: every bounce goes through the general sweep.
template <typename T>
static int launch_rays(LaunchContext* c, const RayArgs& a, hipStream_t st) {
    rt_camera cam;
    memset(&cam, 0, sizeof(cam));
    cam.image_width = cam.image_height = 1u;
    if (a.origin) for (int i = 0; i < 3; ++i) cam.center[i] = a.origin[i];
    const FrameArgs fa{&cam, a.depth, a.spp, a.seed, a.flags, rt_tile_range{0u, 1u, 1u, 0u, (uint32_t)a.n_pixels}, a.rgb, a.lin};
    KParams<T> p;
    context_params(c, filter_off_env(), p);
    frame_params(fa, p);
    const bool root2 = (a.flags & RT_FLAG_ROOT2) != 0u, mega = p.n_mg > 0;
    void (*const rfn)(RParams<T>) = pick_rays<T>(root2, mega);
    constexpr int W = kWavesRays<T>;
    const uint32_t id = kernel_id<T>(W, root2, kModeV2, false, mega, kKernelRaysBit);
    uint64_t nblocks = 0;
    int rc = plan_grid(c, (const void*)rfn, W, id, p.n_items, a.spp, nblocks, p.blk_g);
    if (rc != RT_OK) return rc;
    p.scratch_stride = (size_t)p.vbytes + (size_t)kSlots * p.sbytes;
    const uint64_t max_blocks = kScratchBudget / (4 * p.scratch_stride);   // as launch_plain keeps its scratch
    if (nblocks > max_blocks) nblocks = max_blocks > 0 ? max_blocks : 1;
    if ((rc = ensure_bytes(c->scratch, p.scratch_stride * nblocks * 4, st)) != RT_OK) return rc;
    p.scratch = (char*)c->scratch.p;
    if ((rc = ensure_bytes(c->rayskip, (size_t)((a.n_pixels + 63u) / 64u) * sizeof(uint64_t), st)) != RT_OK) return rc;
    RParams<T> rp;
    memset(&rp, 0, sizeof(rp));
    rp.k = p;
    rp.origins = (const T*)a.origins;
    rp.directions = (const T*)a.directions;
    rp.skip = (uint64_t*)c->rayskip.p;
    rp.R = a.R;
    rp.pixel_base = a.pixel_base;
    if ((rc = zero_claim_counters(c, st)) != RT_OK) return rc;
    hipLaunchKernelGGL(rays_validate<T>, dim3((uint32_t)((a.n_pixels + 255u) / 256u)), dim3(256), 0, st, rp);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(rfn, dim3((uint32_t)nblocks), dim3(256), 0, st, rp);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

// The workgroups of a finish launch over n pixels whose position maps take vbytes each: four waves of one pixel
// at a time, up to 8 workgroups per CU, their maps within the scratch budget.
static uint64_t finish_grid(const LaunchContext* c, uint32_t n, uint32_t vbytes) {
    const uint64_t fb = std::min<uint64_t>(((uint64_t)n + 3) / 4, (uint64_t)c->n_cu * 8u);
    return std::max<uint64_t>(1u, std::min<uint64_t>(fb, kScratchBudget / (4ull * vbytes)));
}

// The sample-parallel kernels' arguments over (pixel, sample sub-range) items: the trace kernel writes the record
// buffer rec (one region per pixel, p.sbytes each) and needs no scratch; the finish kernel's waves stride over
// the pixels, each with a position map of its own in the scratch (fblocks workgroups of them, finish_grid).
template <typename T>
static int split_params(LaunchContext* c, KParams<T>& p, char* rec, uint32_t S, uint32_t nsub, uint32_t n_pix,
                        hipStream_t st, SParams<T>& sp, uint64_t& fblocks) {
    p.scratch_stride = (size_t)p.vbytes;
    fblocks = finish_grid(c, n_pix, p.vbytes);
    const int rc = ensure_bytes(c->scratch, p.scratch_stride * fblocks * 4, st);
    if (rc != RT_OK) return rc;
    p.scratch = (char*)c->scratch.p;
    memset(&sp, 0, sizeof(sp));
    sp.k = p;
    sp.rec = rec;
    sp.S = S;
    sp.nsub = nsub;
    sp.n_pix = n_pix;
    return RT_OK;
}

// trace_paths_split over nsub items of S samples per pixel (rt_split_plan.hpp), then finish_records.
template <typename T>
static int launch_split(LaunchContext* c, const FrameArgs& a, uint32_t S, uint32_t nsub, hipStream_t st) {
    KParams<T> p;
    bool camq = false;
    int rc = frame_setup(c, a, nsub, st, p, camq);
    if (rc != RT_OK) return rc;
    const uint32_t n_pix = p.n_items / nsub;
    const SplitPick<T> pick = pick_split<T>(camq, p.n_mg > 0);
    uint64_t nblocks = 0, fblocks = 0;
    rc = plan_grid(c, (const void*)pick.fn, pick.W, pick.id, p.n_items, std::min(S, a.spp), nblocks, p.blk_g);
    if (rc != RT_OK) return rc;
    if ((rc = ensure_bytes(c->records, (size_t)n_pix * p.sbytes, st)) != RT_OK) return rc;
    SParams<T> sp;
    if ((rc = split_params(c, p, (char*)c->records.p, S, nsub, n_pix, st, sp, fblocks)) != RT_OK) return rc;
    if ((rc = zero_claim_counters(c, st)) != RT_OK) return rc;
    hipLaunchKernelGGL(pick.fn, dim3((uint32_t)nblocks), dim3(256), 0, st, sp);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(finish_records<T>, dim3((uint32_t)fblocks), dim3(256), 0, st, sp);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

// One extend of a progressive session: trace_paths_window over the window's items, then finish_window.
template <typename T>
static int launch_window(LaunchContext* c, const FrameArgs& a, const SessionWindow& w, hipStream_t st) {
    KParams<T> p;
    bool camq = false;
    int rc = frame_setup(c, a, w.nsub, st, p, camq);
    if (rc != RT_OK) return rc;
    const uint32_t n_pix = p.n_items / w.nsub;
    const SplitPick<T> pick = pick_split<T>(camq, p.n_mg > 0);
    void (*const wfn)(WParams<T>) = pick_window<T>(camq, p.n_mg > 0);
    uint64_t nblocks = 0, fblocks = 0;
    rc = plan_grid(c, (const void*)wfn, pick.W, pick.id, p.n_items, std::max(1u, std::min(w.S, a.spp - w.s_begin)),
                   nblocks, p.blk_g);
    if (rc != RT_OK) return rc;
    // a session's regions keep the layout of its capacity whatever the count (the width of e, bit 0 of
    // swide, depends on the depth alone)
    const uint32_t P_cap = prog_positions(w.cap);
    p.sbytes = paths_sbytes(P_cap, sizeof(T), p.swide);
    WParams<T> wp;
    memset(&wp, 0, sizeof(wp));
    if ((rc = split_params(c, p, w.rec, w.S, w.nsub, n_pix, st, wp.s, fblocks)) != RT_OK) return rc;   // the snapshot's counts: finish_window
    wp.s_begin = w.s_begin;
    wp.s_base = w.s_base;
    wp.P_cap = P_cap;
    if (w.trace) {
        WParams<T> wt = wp;
        wt.s.k.P = P_cap;   // the record view's stride (split_records); the trace kernels read no other count
        if ((rc = zero_claim_counters(c, st)) != RT_OK) return rc;
        hipLaunchKernelGGL(wfn, dim3((uint32_t)nblocks), dim3(256), 0, st, wt);
        HIPCHK(hipGetLastError());
    }
    if (w.finish) {
        hipLaunchKernelGGL(finish_window<T>, dim3((uint32_t)fblocks), dim3(256), 0, st, wp);
        HIPCHK(hipGetLastError());
    }
    return RT_OK;
}

// ---- around every call that enqueues work ----
// Renders on one context share its work counter, scratch and camera tables: a launch on a new
// stream first waits for the previous stream, so cross-stream use serialises instead of racing.
// st: NULL = the HIP null stream.
static int begin_launch(LaunchContext* c, hipStream_t st) {
    HIPCHK(hipSetDevice(c->device));
    if (c->have_last && c->last_stream != st) HIPCHK(hipStreamSynchronize(c->last_stream));
    c->last_stream = st;
    c->have_last = true;
    if (!c->have_first) {
        HIPCHK(hipEventRecord(c->ev_first, st));
        c->have_first = true;
    }
    return RT_OK;
}
static int end_launch(LaunchContext* c, hipStream_t st, uint64_t pixels, uint64_t samples) {
    HIPCHK(hipEventRecord(c->ev_last, st));
    c->pixels += pixels;
    c->samples += samples;
    return RT_OK;
}

}  // namespace rt
