// rt_kernel.hip — MI355X (gfx950) megakernel for the reference's per-pixel sample loop.
//
// Replaces TileRenderTask::render_vectorized2 (src/renderer.rs:141-176) and everything it
// calls: Camera::get_ray (ray_tracing.rs:77-89), Scene::trace_vectorized2
// (ray_tracing.rs:375-505), Sphere::hit_packed (objects.rs:249-290), PackedHitRecords
// (objects.rs:121-176), Material::get_hit_result (materials.rs:54-147), the final sky pass and
// reduction (ray_tracing.rs:486-504), /spp and Color::to_u8_array (renderer.rs:161,
// color.rs:54-64).
//
// Mapping:
//   * path regeneration: a persistent wave keeps one ray per lane from its camera ray to its
//     termination, then takes the next sample (of this pixel or of the next one its workgroup
//     claims from an atomic block counter; up to kSlots pixels in flight).  Every ray's bounce k depends only
//     on its own state and the counter-based RNG key (sample, pixel, k, stream), so no ray waits
//     for the others; lane utilisation is ~1.0.
//   * each sweep finds every sphere the reference could hit through conservative fp32 culls and
//     runs the reference's exact test on those only: spheres stream through the scalar cache in
//     64-byte groups (s_load_dwordx16 into SGPRs, a free broadcast to all 64 lanes), two spheres
//     per packed-FP32 instruction; bounced rays first slab-test 16-sphere cluster boxes, then a
//     per-sphere distance filter on the clusters some lane may hit (nearest_hit).
//   * pinhole cameras: primary rays run in full-wave camera batches; a cone around the batch's
//     rays culls clusters and spheres with lanes as spheres (camera_sweep), survivors get the
//     exact test from a per-launch camera-origin table (oc and c are the same for every primary
//     ray); hits wait in an LDS queue for free lanes.
//   * the reference's positions (its per-bounce stable shuffle) are a function of the per-sample
//     termination bounces alone; when a pixel's last sample ends, finish_pixel replays them,
//     applies quirk Q3's buffer read ("retire rule") and sums in the reference's order, so fp64
//     and fp32 results are bit-identical to the CPU restatement in oracle/.
//
// Source layout (one translation unit): rt_experiments.hpp (build kinds), rt_formats.hpp (the formats host
// layout and device code share; no HIP), rt_common.hpp (kernel arguments, scalar-load pipelines),
// rt_sweep.hpp (general sweep), rt_camera.hpp (primary rays, scatter), rt_finish.hpp (replay + reduction),
// rt_trace.hpp + rt_trace_body.hpp (the persistent kernel), rt_guides.hpp (guide buffers: first hits only),
// rt_query.hpp (ray queries: the closest hit of the caller's rays);
// and, host only, without HIP: rt_layout.hpp (the scene image: every device table of a scene,
// build_scene_image), rt_split_plan.hpp (the sample-parallel plan), rt_progressive_plan.hpp (a progressive
// session's record buffer and sample windows).  This file holds the C ABI: the context and its device tables,
// the launch steps (scene_params, frame_params, ensure_cam_tables, plan_grid) and the launchers (launch_plain,
// launch_split, launch_window; launch_items and launch_classes for a session's per-pixel counts;
// launch_guides, launch_query).
#include "rt_trace.hpp"
#include "rt_guides.hpp"
#include "rt_query.hpp"
#include "rt_layout.hpp"
#include "rt_split_plan.hpp"
#include "rt_progressive_plan.hpp"

#include <chrono>
#include <mutex>
#include <string>

// ============================== host side ==============================
using namespace rt;

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define HIPCHK(x)                                                                     \
    do {                                                                              \
        hipError_t e_ = (x);                                                          \
        if (e_ != hipSuccess) return fail(RT_ERR_HIP, std::string(#x ": ") + hipGetErrorString(e_)); \
    } while (0)

// One hipMalloc and its size; move-only, freed with its owner.
struct DeviceBuffer {
    void* p = nullptr;
    size_t bytes = 0;
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
        if (this != &o) { reset(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DeviceBuffer() { reset(); }
    hipError_t release() {
        const hipError_t e = p ? hipFree(p) : hipSuccess;
        p = nullptr;
        bytes = 0;
        return e;
    }
    void reset() { (void)release(); }
    hipError_t alloc(size_t n) {   // n == 0: hipMalloc gives no memory (p stays NULL)
        reset();
        const hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n; else p = nullptr;
        return e;
    }
};
static int upload(DeviceBuffer& d, const void* src, size_t bytes) {
    HIPCHK(d.alloc(bytes));
    HIPCHK(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
    return RT_OK;
}
static int reserve(DeviceBuffer& d, size_t bytes) {
    HIPCHK(d.alloc(bytes));
    return RT_OK;
}
// A table the scene does not have (empty: the mega levels of a small scene) stays NULL.
template <typename V> static int upload(DeviceBuffer& d, const std::vector<V>& v) {
    return v.empty() ? RT_OK : upload(d, v.data(), v.size() * sizeof(V));
}
// Grow a buffer the launches of a context share (scratch, records): nothing may still be using the old one.
static int ensure_bytes(DeviceBuffer& b, size_t bytes, hipStream_t st) {
    if (bytes <= b.bytes) return RT_OK;
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(b.release());
    HIPCHK(b.alloc(bytes));
    return RT_OK;
}

// A pinned host buffer that is copied to the device asynchronously, and the event behind its last copy: the
// host writes it again only after that copy has run.  Move-only, freed with its owner.
struct PinnedStage {
    void* p = nullptr;
    size_t bytes = 0;
    hipEvent_t ev = nullptr;
    bool pending = false;
    PinnedStage() = default;
    PinnedStage(const PinnedStage&) = delete;
    PinnedStage& operator=(const PinnedStage&) = delete;
    PinnedStage& operator=(PinnedStage&& o) noexcept {
        if (this != &o) {
            reset();
            p = o.p; bytes = o.bytes; ev = o.ev; pending = o.pending;
            o.p = nullptr; o.bytes = 0; o.ev = nullptr; o.pending = false;
        }
        return *this;
    }
    ~PinnedStage() { reset(); }
    void reset() {
        if (pending) (void)hipEventSynchronize(ev);
        if (ev) (void)hipEventDestroy(ev);
        if (p) (void)hipHostFree(p);
        p = nullptr; bytes = 0; ev = nullptr; pending = false;
    }
};
// Room for n bytes the host may write now (blocks on the previous copy out of the buffer).
static int stage_reserve(PinnedStage& g, size_t n) {
    if (!g.ev) HIPCHK(hipEventCreateWithFlags(&g.ev, hipEventDisableTiming));
    if (g.pending) {
        HIPCHK(hipEventSynchronize(g.ev));
        g.pending = false;
    }
    if (n <= g.bytes) return RT_OK;
    if (g.p) HIPCHK(hipHostFree(g.p));
    g.p = nullptr;
    g.bytes = 0;
    HIPCHK(hipHostMalloc(&g.p, n, hipHostMallocDefault));
    g.bytes = n;
    return RT_OK;
}

// The device side of SceneTables<T> (rt_layout.hpp), one allocation per table, its constants, and the
// tables build_cam_table fills at a launch.  The camera tables depend only on the scene, the camera
// centre, the scalar mode and RT_FILTER_OFF: a launch with the same key reuses them (bench frames, shards).
template <typename T> struct DeviceScene {
    DeviceBuffer sph, cen, fsph, rsph, rfsph, rflat, top, sup, lfs, lbx[4], clus, mats;
    DeviceBuffer cam, camf, camx, cull, cullc;   // camera-origin, camera filter, per-sphere, cone-cull, per-cluster
    TableConsts k;
    struct CamKey { bool valid = false; double center[3] = {0, 0, 0}; uint32_t scalar = 0, off = 0; } camkey;
    void reset() { *this = DeviceScene(); }
};
template <typename T> static int upload_scene(DeviceScene<T>& d, const SceneTables<T>& t) {
    int rc = RT_OK;
    auto up = [&](DeviceBuffer& dst, const auto& v) { if (rc == RT_OK) rc = upload(dst, v); };
    auto room = [&](DeviceBuffer& dst, size_t bytes) { if (rc == RT_OK) rc = reserve(dst, bytes); };
    up(d.sph, t.sph); up(d.cen, t.cen); up(d.fsph, t.fsph);
    up(d.rsph, t.rsph); up(d.rfsph, t.rfsph); up(d.rflat, t.rflat);
    up(d.top, t.top); up(d.sup, t.sup);   // t.meg stays on the host: the mega kernels read the local levels (lbx)
    up(d.lfs, t.lfs);
    for (int lv = 0; lv < 4; ++lv) up(d.lbx[lv], t.lbx[lv]);
    up(d.clus, t.clus); up(d.mats, t.mats);
    room(d.cam, t.cam_bytes.cam); room(d.camf, t.cam_bytes.camf); room(d.camx, t.cam_bytes.camx);
    room(d.cull, t.cam_bytes.cull); room(d.cullc, t.cam_bytes.cullc);
    d.k = t.k;
    return rc;
}

// The pixels of one reduction that share a sample count: list[first .. first + n) of the reduction's index list.
struct CountClass {
    uint32_t spp, first, n;
};

struct rt_context {
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
    int n_cu = 0;
    uint64_t samples = 0, pixels = 0;
    hipStream_t last_stream = nullptr;   // stream of the previous render (they share scratch and tables)
    bool have_last = false;
    uint32_t last_kernel_id = 0, last_wg_per_cu = 0;   // rt_stats.kernel_id / kernel_wg_per_cu of the last launch
    // The progressive session (rt_progressive_*): what rt_progressive_begin fixed, the samples each pixel's
    // region holds so far (done, in the range's compact order; done_min == done_max: a uniform session), and the
    // record buffer, which only the session's launches touch.  The per-pixel-count calls send their tables (the
    // item table, the classes' index lists, the counts) through stage into tables, and the error estimate keeps
    // its two linear snapshots in lin_full and lin_half.
    struct Session {
        bool open = false;
        rt_camera cam{};
        rt_tile_range rg{};
        uint32_t depth = 0, cap = 0, flags = 0, done_min = 0, done_max = 0;
        std::vector<uint32_t> done;
        uint64_t seed = 0;
        void* rec = nullptr;
        uint64_t bytes = 0;
        hipStream_t stream = nullptr;   // of the last call that enqueued work
        bool have_stream = false;
        PinnedStage stage;
        DeviceBuffer tables, lin_full, lin_half;
        void set_done(uint32_t n) { std::fill(done.begin(), done.end(), n); done_min = done_max = n; }
        // The refinement run (rt_progressive_refine; one per session): its tolerance and cap, the candidates of the
        // next step (the n_cand pixels of act[cur], all at n_k samples; the run's first step takes every pixel),
        // the classes of the pixels that stopped (spp, first, n: their pixels are cls_list[first .. first + n) on
        // the device), and the last step's plan.  While a run is unbroken the device array counts is what the
        // pixels hold, and done_stale says that `done` has not been copied down since the last step.
        struct Refine {
            bool started = false, broken = false;
            double tol = 0.0;
            uint32_t spp_max = 0, n_k = 0, n_cand = 0, cls_used = 0, S = 0;
            int cur = 0;
            uint64_t n_items = 0;
            std::vector<CountClass> cls;
        } run;
        bool done_stale = false;
        DeviceBuffer counts, act[2], cls_list, sel, blk, ret, items, lin_cur, lin_new;
    } prog;
};

extern "C" const char* rt_last_error(void) { return g_err.c_str(); }
// "rt_mi355x <version> gfx950 <product|experiment> src=<hash of the sources it was built from>"
extern "C" const char* rt_version(void) { return "rt_mi355x 0.3 gfx950 " RT_BUILD_KIND " src=" RT_SRC_HASH; }

extern "C" double rt_metal_clamp_fuzz(double fuzz) { return fuzz < 1.0 ? fuzz : 1.0; }

// Camera::new, ray_tracing.rs:27-62 (f64, Vec3 ops without FMA; compiled -ffp-contract=off).
extern "C" int rt_camera_new(rt_camera* out, uint32_t w, uint32_t h, double focal_length, double view_angle_deg,
                             const double center[3], const double look_at[3], const double up[3],
                             double defocus_angle_deg) {
    if (!out || !center || !look_at || !up || w == 0 || h == 0) return fail(RT_ERR_INVALID, "rt_camera_new: bad argument");
    const double rads_per_deg = 3.141592653589793 / 180.0;              // f64::to_radians
    const double aspect = (double)w / (double)h;                         // :28
    const double vh = std::tan((view_angle_deg * rads_per_deg) / 2.0) * focal_length * 2.0;  // :29
    const double vw = vh * aspect;                                       // :32
    auto unit3 = [](const double a[3], double o[3]) {
        const double l = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
        o[0] = a[0] / l; o[1] = a[1] / l; o[2] = a[2] / l;
    };
    double dirv[3] = {look_at[0] - center[0], look_at[1] - center[1], look_at[2] - center[2]};
    double dir[3]; unit3(dirv, dir);                                     // :34
    const double wv[3] = {-dir[0], -dir[1], -dir[2]};                    // :35
    const double cr[3] = {up[1] * wv[2] - up[2] * wv[1], up[2] * wv[0] - up[0] * wv[2], up[0] * wv[1] - up[1] * wv[0]};
    double u[3]; unit3(cr, u);                                           // :36
    const double v[3] = {wv[1] * u[2] - wv[2] * u[1], wv[2] * u[0] - wv[0] * u[2], wv[0] * u[1] - wv[1] * u[0]};  // :37
    const double dr = focal_length * std::tan((defocus_angle_deg / 2.0) * rads_per_deg);  // :43
    out->image_width = w; out->image_height = h;
    for (int i = 0; i < 3; ++i) {
        out->center[i] = center[i];
        out->vu[i] = u[i] * vw;                                          // :39
        out->vv[i] = (-v[i]) * vh;                                       // :40
        out->ulc[i] = ((center[i] - wv[i] * focal_length) - out->vu[i] / 2.0) - out->vv[i] / 2.0;  // :41
        out->du[i] = u[i] * dr;                                          // :44
        out->dv[i] = v[i] * dr;                                          // :45
    }
    return RT_OK;
}

extern "C" int rt_context_create(int device, rt_context** out) {
    if (!out) return fail(RT_ERR_INVALID, "rt_context_create: out is NULL");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(RT_ERR_INVALID, "rt_context_create: no such device");
    HIPCHK(hipSetDevice(device));
    rt_context* c = new rt_context();
    c->device = device;
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&c->ev_first));
    HIPCHK(hipEventCreate(&c->ev_last));
    HIPCHK(c->segs.alloc(sizeof(unsigned long long) * kSegShards * kSegStride));
    HIPCHK(c->err.alloc(16));
    HIPCHK(c->counter.alloc(kStreams * kCtrStride * sizeof(uint32_t)));   // claim streams (rt_trace.hpp)
    HIPCHK(hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device));
    HIPCHK(hipMemset(c->segs.p, 0, c->segs.bytes));
    HIPCHK(hipMemset(c->err.p, 0, 16));
    *out = c;
    return RT_OK;
}

// A context without a scene: no table, every count zero.
static void free_scene(rt_context* c) {
    c->d32.reset();
    c->d64.reset();
    c->ridx.reset();
    c->mtiers.reset();
    c->n = SceneCounts{};
    c->has_scene = false;
}

extern "C" int rt_context_destroy(rt_context* c) {
    if (!c) return RT_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->prog.open) (void)rt_progressive_end(c);
    free_scene(c);
    c->segs.reset(); c->err.reset(); c->counter.reset(); c->scratch.reset(); c->records.reset();
    (void)hipEventDestroy(c->ev_first); (void)hipEventDestroy(c->ev_last);
    (void)hipStreamDestroy(c->stream);
    delete c;
    return RT_OK;
}

extern "C" int rt_context_set_scene(rt_context* c, const rt_scene* s) {
    if (!c || !s) return fail(RT_ERR_INVALID, "rt_context_set_scene: NULL argument");
    if (c->prog.open)
        return fail(RT_ERR_INVALID, "rt_context_set_scene: a progressive session is open (its records belong to the "
                                    "current scene; rt_progressive_end first)");
    if (s->n_spheres && (!s->center || !s->radius || !s->material || !s->materials))
        return fail(RT_ERR_INVALID, "rt_context_set_scene: NULL array");
    for (uint32_t i = 0; i < s->n_spheres; ++i)
        if (s->material[i] >= s->n_materials)
            return fail(RT_ERR_INVALID, "rt_context_set_scene: material index out of range (objects.rs:296 would panic)");
    for (uint32_t i = 0; i < s->n_materials; ++i)
        if (s->materials[i].kind > RT_DIELECTRIC)
            return fail(RT_ERR_INVALID, "rt_context_set_scene: unknown material kind (materials.rs:31 would panic)");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    free_scene(c);   // with it the camera tables built for the previous scene, and their keys
    const SceneImage im = build_scene_image(s);
    int rc = upload_scene(c->d64, im.t64);
    if (rc == RT_OK) rc = upload_scene(c->d32, im.t32);
    if (rc == RT_OK) rc = upload(c->ridx, im.ridx);
    if (rc == RT_OK) rc = upload(c->mtiers, im.mtiers);
    if (rc != RT_OK) {
        free_scene(c);
        return rc;
    }
    c->n = im.n;
    c->has_scene = true;
    return RT_OK;
}

static bool check_range(const rt_camera* cam, const rt_tile_range* r) {
    if (r->row_count == 0 || r->col_count == 0 || r->row_step == 0) return false;
    if (r->col_begin + (uint64_t)r->col_count > cam->image_width) return false;
    const uint64_t last_row = r->row_begin + (uint64_t)(r->row_count - 1) * r->row_step;
    return last_row < cam->image_height;
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
    const uint32_t id = 0x8000u | (sizeof(T) == 8 ? 1u : 0u) | ((uint32_t)W << 1) | (ROOT2 ? 1u << 4 : 0u) |
                        ((uint32_t)MODE << 5) | (CAMQ ? 1u << 7 : 0u) | (MEGA ? 1u << 8 : 0u);
    return KernelPick<T>{trace_paths<T, W, ROOT2, MODE, CAMQ, MEGA>, id, W};
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
template <typename T, bool CAMQ>
static SplitPick<T> pick_split(bool mega) {
    constexpr int W = kWavesSplit<T>;
    const uint32_t id = 0x8000u | (sizeof(T) == 8 ? 1u : 0u) | ((uint32_t)W << 1) | (CAMQ ? 1u << 7 : 0u) |
                        (mega ? 1u << 8 : 0u) | (1u << 9);
    return SplitPick<T>{mega ? trace_paths_split<T, W, CAMQ, true> : trace_paths_split<T, W, CAMQ, false>, id, W};
}
// A progressive session's tracing kernel (trace_paths_window), at the same occupancy.
template <typename T, bool CAMQ>
static void (*pick_window(bool mega))(WParams<T>) {
    constexpr int W = kWavesSplit<T>;
    return mega ? trace_paths_window<T, W, CAMQ, true> : trace_paths_window<T, W, CAMQ, false>;
}
// ... and its tracing kernel over an item table (trace_paths_items; RT_KERNEL_ITEMS in the kernel id).
constexpr uint32_t kKernelItemsBit = 1u << 10;
template <typename T, bool CAMQ>
static void (*pick_items(bool mega))(IParams<T>) {
    constexpr int W = kWavesSplit<T>;
    return mega ? trace_paths_items<T, W, CAMQ, true> : trace_paths_items<T, W, CAMQ, false>;
}
// The guide-buffer kernel (rt_render_guides_async): guide_pixels<T, CAMQ, MEGA> (RT_KERNEL_GUIDES in the kernel id).
constexpr uint32_t kKernelGuidesBit = 1u << 11;
template <typename T, bool CAMQ>
static void (*pick_guides(bool mega))(GParams<T>) {
    return mega ? guide_pixels<T, CAMQ, true> : guide_pixels<T, CAMQ, false>;
}
// The ray-query kernel (rt_query_hits_async): query_rays<T, ROOT2, SHARED, MEGA> (RT_KERNEL_QUERY in the kernel id).
constexpr uint32_t kKernelQueryBit = 1u << 12;
template <typename T, bool ROOT2, bool SHARED>
static void (*pick_query(bool mega))(QParams<T>) {
    return mega ? query_rays<T, ROOT2, SHARED, true> : query_rays<T, ROOT2, SHARED, false>;
}
template <typename T>
static void (*pick_query(bool root2, bool shared, bool mega))(QParams<T>) {
    if (root2) return shared ? pick_query<T, true, true>(mega) : pick_query<T, true, false>(mega);
    return shared ? pick_query<T, false, true>(mega) : pick_query<T, false, false>(mega);
}
constexpr uint64_t kScratchBudget = 24ull << 30;   // scratch (and record buffer) bytes a launch may ask for

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

// The scene's tables, constants and counts, and the context's counters.
template <typename T>
static void scene_params(rt_context* c, KParams<T>& p) {
    const DeviceScene<T>& d = c->scene<T>();
    const SceneCounts& n = c->n;
    p.sph = (const T*)d.sph.p;
    p.cen = (const T*)d.cen.p;
    p.n_groups = d.k.n_groups;
    p.fsph = (const float*)d.fsph.p;
    p.n_fgroups = n.n_fgroups;
    p.rsph = (const T*)d.rsph.p;
    p.rfsph = (const float*)d.rfsph.p;
    p.ftop = (const float*)d.top.p;
    p.fsup = (const float*)d.sup.p;
    p.rflat = (const float*)d.rflat.p;
    p.n_mg = n.n_mg;
    p.lfsph = (const float*)d.lfs.p;
    p.lclb = (const float*)d.lbx[0].p;
    p.lsup = (const float*)d.lbx[1].p;
    p.lmeg = (const float*)d.lbx[2].p;
    p.lgig = (const float*)d.lbx[3].p;
    p.n_gg = n.n_gg;
    p.mtiers = (const uint64_t*)c->mtiers.p;
    for (int a = 0; a < 3; ++a) { p.mt_lo[a] = n.mt_lo[a]; p.mt_n[a] = n.mt_n[a]; }
    p.mt_inv = n.mt_inv;
    p.l_r2max = d.k.l_r2max;
    p.l_hir2 = d.k.l_hir2;
    p.l_isr = d.k.l_isr;
    p.ridx = (const uint32_t*)c->ridx.p;
    p.n_top = n.n_top;
    p.n_xg = n.n_xg;
    p.n_xs = n.n_xs;
    p.f_cmax = d.k.f_cmax;
    p.f_r2max = d.k.f_r2max;
    p.f_r2min = d.k.f_r2min;
    p.f_ir2 = d.k.f_ir2;
    p.f_hir2 = d.k.f_hir2;
    p.f_isr = d.k.f_isr;
    p.mats = (const MatT<T>*)d.mats.p;
    p.n_spheres = n.n_spheres;
    p.segs = (unsigned long long*)c->segs.p;
    p.err = (uint32_t*)c->err.p;
    p.counter = (uint32_t*)c->counter.p;
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
    // fp64: Philox4x32-10 keyed by (seed lo, seed hi).  fp32: Philox2x32-10 has a 32-bit key, folded here as
    // seed lo ^ fmix32(seed hi) (rng<float> reads k0 only): fmix32(0) = 0, so a seed below 2^32 keys as itself,
    // and seeds such as (m << 32) | m no longer all key as 0.
    if (sizeof(T) == 8) { p.k0 = (uint32_t)a.seed; p.k1 = (uint32_t)(a.seed >> 32); }
    else { p.k0 = (uint32_t)a.seed ^ fmix32((uint32_t)(a.seed >> 32)); p.k1 = 0u; }
    const rt_tile_range& rg = a.rg;
    p.row_begin = rg.row_begin; p.row_step = rg.row_step; p.col_begin = rg.col_begin; p.col_count = rg.col_count;
    p.rgb = (uint8_t*)a.rgb;
    p.lin = (double*)a.lin;
    p.n_items = rg.row_count * rg.col_count;
    p.swide = paths_wide(p.P, a.depth);
    p.vbytes = paths_vbytes(p.P, p.swide, (a.flags & RT_FLAG_MODE_VECTORIZED3) != 0u);
    p.sbytes = paths_sbytes(p.P, sizeof(T), p.swide);
}

// Camera batches + camera-origin tables (every primary ray starts at the centre): point p at the camera
// tables of this precision and rebuild them unless the last launch left them for the same key.
template <typename T>
static int ensure_cam_tables(rt_context* c, KParams<T>& p, uint32_t flags, bool filter_off, hipStream_t st) {
    DeviceScene<T>& d = c->scene<T>();
    const SceneCounts& n = c->n;
    p.camsph = (const T*)d.cam.p;
    p.camf = (const float*)d.camf.p;
    p.camx = (const T*)d.camx.p;
    p.cull = (const float*)d.cull.p;
    const uint32_t n_slots = (p.n_groups + 1) * kGroup<T>, n_fslots = (p.n_fgroups + 1) * 4;
    p.cullc = (const float*)d.cullc.p;
    p.n_clp = n.n_clp;
    p.n_supc = n.n_supc;
    const uint32_t n_thr = std::max(std::max(std::max(n_slots, n_fslots), n.n_cull),
                                    std::max(n.n_cslots, n.n_clp + n.n_supc));
    auto& ck = d.camkey;
    const uint32_t scalar = (flags & RT_FLAG_MODE_SCALAR) ? 1u : 0u;
    double cen[3] = {(double)p.center[0], (double)p.center[1], (double)p.center[2]};
    const bool same = ck.valid && ck.scalar == scalar && ck.off == (uint32_t)filter_off &&
                      memcmp(ck.center, cen, sizeof(cen)) == 0;   // bit for bit (-0 is not +0)
    if (same) return RT_OK;
    auto build = scalar ? build_cam_table<T, true> : build_cam_table<T, false>;
    hipLaunchKernelGGL(build, dim3((n_thr + 255) / 256), dim3(256), 0, st, p.sph, (T*)p.camsph, n_slots,
                       (float*)p.camf, n_fslots, p.center[0], p.center[1], p.center[2], (uint32_t)filter_off,
                       (T*)p.camx, (float*)p.cull, n.n_cull, n.n_spheres, p.ridx, n.n_cslots,
                       (const double*)d.clus.p, (float*)p.cullc, n.n_clp + n.n_supc);
    HIPCHK(hipGetLastError());
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
static int frame_setup(rt_context* c, const FrameArgs& a, uint32_t items_per_pixel, hipStream_t st, KParams<T>& p,
                       bool& camq) {
    memset(&p, 0, sizeof(p));
    scene_params(c, p);
    // diagnostics: every general-sweep and camera-sweep group through the exact test
    const char* e = getenv("RT_FILTER_OFF");
    const bool filter_off = e && atoi(e) != 0;
    if (filter_off) p.f_cmax = std::numeric_limits<float>::infinity();
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
static int plan_grid(rt_context* c, const void* kfn, int kW, uint32_t id, uint32_t n_items, uint32_t item_spp,
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

static int zero_claim_counters(rt_context* c, hipStream_t st) {
    HIPCHK(hipMemsetAsync(c->counter.p, 0, kStreams * kCtrStride * sizeof(uint32_t), st));
    return RT_OK;
}

// trace_paths: one work item per pixel, every sample of it.
template <typename T>
static int launch_plain(rt_context* c, const FrameArgs& a, hipStream_t st) {
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
    const KernelPick<T> pick = camq ? pick_kernel<T, true>(a.flags, W, p.n_mg > 0, big)
                                    : pick_kernel<T, false>(a.flags, W, p.n_mg > 0, big);
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
static int launch_guides(rt_context* c, const FrameArgs& a, float* albedo, float* normal, float* depth, float* coverage,
                         hipStream_t st) {
    KParams<T> p;
    bool camq = false;
    int rc = frame_setup(c, a, 1u, st, p, camq);
    if (rc != RT_OK) return rc;
    const bool mega = p.n_mg > 0;
    void (*const gfn)(GParams<T>) = camq ? pick_guides<T, true>(mega) : pick_guides<T, false>(mega);
    constexpr int W = kWavesGuide<T>;
    const uint32_t id = 0x8000u | (sizeof(T) == 8 ? 1u : 0u) | ((uint32_t)W << 1) | (camq ? 1u << 7 : 0u) |
                        (mega ? 1u << 8 : 0u) | kKernelGuidesBit;
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
static int launch_query(rt_context* c, const QueryArgs& a, hipStream_t st) {
    KParams<T> p;
    memset(&p, 0, sizeof(p));
    scene_params(c, p);
    const char* e = getenv("RT_FILTER_OFF");   // diagnostics, as frame_setup has it
    const bool filter_off = e && atoi(e) != 0;
    if (filter_off) p.f_cmax = std::numeric_limits<float>::infinity();
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
    const uint32_t id = 0x8000u | (sizeof(T) == 8 ? 1u : 0u) | ((uint32_t)W << 1) | (root2 ? 1u << 4 : 0u) |
                        (shared ? 1u << 7 : 0u) | (mega ? 1u << 8 : 0u) | kKernelQueryBit;
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

// The sample-parallel kernels' arguments over (pixel, sample sub-range) items: the trace kernel writes the record
// buffer rec (one region per pixel, p.sbytes each) and needs no scratch; the finish kernel's waves stride over
// the pixels, each with a position map of its own in the scratch (fblocks workgroups of them).
template <typename T>
static int split_params(rt_context* c, KParams<T>& p, char* rec, uint32_t S, uint32_t nsub, uint32_t n_pix,
                        hipStream_t st, SParams<T>& sp, uint64_t& fblocks) {
    p.scratch_stride = (size_t)p.vbytes;
    fblocks = std::min<uint64_t>(((uint64_t)n_pix + 3) / 4, (uint64_t)c->n_cu * 8u);
    fblocks = std::max<uint64_t>(1u, std::min<uint64_t>(fblocks, kScratchBudget / (4 * p.scratch_stride)));
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
static int launch_split(rt_context* c, const FrameArgs& a, uint32_t S, uint32_t nsub, hipStream_t st) {
    KParams<T> p;
    bool camq = false;
    int rc = frame_setup(c, a, nsub, st, p, camq);
    if (rc != RT_OK) return rc;
    const uint32_t n_pix = p.n_items / nsub;
    const SplitPick<T> pick = camq ? pick_split<T, true>(p.n_mg > 0) : pick_split<T, false>(p.n_mg > 0);
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
static int launch_window(rt_context* c, const FrameArgs& a, const SessionWindow& w, hipStream_t st) {
    KParams<T> p;
    bool camq = false;
    int rc = frame_setup(c, a, w.nsub, st, p, camq);
    if (rc != RT_OK) return rc;
    const uint32_t n_pix = p.n_items / w.nsub;
    const SplitPick<T> pick = camq ? pick_split<T, true>(p.n_mg > 0) : pick_split<T, false>(p.n_mg > 0);
    void (*const wfn)(WParams<T>) = camq ? pick_window<T, true>(p.n_mg > 0) : pick_window<T, false>(p.n_mg > 0);
    uint64_t nblocks = 0, fblocks = 0;
    rc = plan_grid(c, (const void*)wfn, pick.W, pick.id, p.n_items, std::max(1u, std::min(w.S, a.spp - w.s_begin)),
                   nblocks, p.blk_g);
    if (rc != RT_OK) return rc;
    // a session's regions keep the layout of its capacity whatever the count (the width of e, bit 0 of
    // swide, depends on the depth alone)
    const uint32_t P_cap = 4u * ((w.cap + 3u) / 4u);
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

// ---- per-pixel counts (rt_progressive_extend_map_async and its kin; DESIGN.md §4 "Per-pixel counts") ----
static_assert(sizeof(MapItem) == kMapItemWords * sizeof(uint32_t), "the plan's records are the kernel's");
constexpr size_t kMaxCountClasses = 256;   // distinct counts one reduction may have (a launch each)

// Group the pixels by counts[p] (0: the pixel is left out): the classes in ascending count, and, with list, each
// class's pixel indices in pixel order.  false: more than kMaxCountClasses distinct counts.
static bool group_by_count(const uint32_t* counts, uint32_t n_pix, uint32_t* list, std::vector<CountClass>& cls) {
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

// The session's frame at `spp` samples with the given outputs.
static FrameArgs session_frame(const rt_context::Session& s, uint32_t spp, void* rgb, void* lin) {
    return FrameArgs{&s.cam, s.depth, spp, s.seed, s.flags, s.rg, rgb, lin};
}

// Send the first `bytes` of the session's staging buffer to its device tables, on st.
static int send_tables(rt_context::Session& s, size_t bytes, hipStream_t st) {
    const int rc = ensure_bytes(s.tables, bytes, st);
    if (rc != RT_OK) return rc;
    HIPCHK(hipMemcpyAsync(s.tables.p, s.stage.p, bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(s.stage.ev, st));
    s.stage.pending = true;
    return RT_OK;
}

// trace_paths_items over the n_items records at `items` (device), item_spp samples each on average.
template <typename T>
static int launch_items(rt_context* c, const rt_context::Session& s, const MapItem* items, uint32_t n_items,
                        uint32_t item_spp, hipStream_t st) {
    KParams<T> p;
    bool camq = false;
    int rc = frame_setup(c, session_frame(s, s.cap, nullptr, nullptr), 1u, st, p, camq);
    if (rc != RT_OK) return rc;
    const SplitPick<T> pick = camq ? pick_split<T, true>(p.n_mg > 0) : pick_split<T, false>(p.n_mg > 0);
    void (*const ifn)(IParams<T>) = camq ? pick_items<T, true>(p.n_mg > 0) : pick_items<T, false>(p.n_mg > 0);
    p.n_items = n_items;
    uint64_t nblocks = 0;
    rc = plan_grid(c, (const void*)ifn, pick.W, pick.id | kKernelItemsBit, n_items, item_spp, nblocks, p.blk_g);
    if (rc != RT_OK) return rc;
    // the records' strides are the capacity's (frame_setup laid the frame out for s.cap); the trace kernels read
    // no sample count from the arguments: every item carries its own
    IParams<T> ip;
    memset(&ip, 0, sizeof(ip));
    ip.w.s.k = p;
    ip.w.s.rec = (char*)s.rec;
    ip.w.s.n_pix = s.rg.row_count * s.rg.col_count;
    ip.w.P_cap = p.P;
    ip.items = items;
    if ((rc = zero_claim_counters(c, st)) != RT_OK) return rc;
    hipLaunchKernelGGL(ifn, dim3((uint32_t)nblocks), dim3(256), 0, st, ip);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

// finish_window_list once per class, over the classes' index lists at `list` (device).  set_id: no trace kernel
// ran in this call, so the kernel id is the session's sample-parallel kernels' without RT_KERNEL_ITEMS.
template <typename T>
static int launch_classes(rt_context* c, const rt_context::Session& s, const std::vector<CountClass>& cls,
                          const uint32_t* list, void* rgb, void* lin, bool set_id, hipStream_t st) {
    const uint32_t P_cap = prog_positions(s.cap);
    // the scratch (one position map per wave) for the largest class, before the first launch reads it
    uint64_t need = 0;
    for (const CountClass& k : cls) {
        const uint32_t P = prog_positions(k.spp), vb = paths_vbytes(P, paths_wide(P, s.depth), false);
        uint64_t fb = std::min<uint64_t>(((uint64_t)k.n + 3) / 4, (uint64_t)c->n_cu * 8u);
        fb = std::max<uint64_t>(1u, std::min<uint64_t>(fb, kScratchBudget / (4ull * vb)));
        need = std::max<uint64_t>(need, (uint64_t)vb * fb * 4u);
    }
    int rc = ensure_bytes(c->scratch, need, st);
    if (rc != RT_OK) return rc;
    for (const CountClass& k : cls) {
        KParams<T> p;
        bool camq = false;
        if ((rc = frame_setup(c, session_frame(s, k.spp, rgb, lin), 1u, st, p, camq)) != RT_OK) return rc;
        if (set_id) {
            const SplitPick<T> pick = camq ? pick_split<T, true>(p.n_mg > 0) : pick_split<T, false>(p.n_mg > 0);
            void (*const wfn)(WParams<T>) = camq ? pick_window<T, true>(p.n_mg > 0) : pick_window<T, false>(p.n_mg > 0);
            uint64_t nb = 0;
            uint32_t g = 0;
            if ((rc = plan_grid(c, (const void*)wfn, pick.W, pick.id, p.n_items, 1u, nb, g)) != RT_OK) return rc;
            set_id = false;
        }
        p.sbytes = paths_sbytes(P_cap, sizeof(T), p.swide);   // a region's size: the capacity's (launch_window)
        LParams<T> lp;
        memset(&lp, 0, sizeof(lp));
        uint64_t fblocks = 0;
        if ((rc = split_params(c, p, (char*)s.rec, 1u, 1u, k.n, st, lp.w.s, fblocks)) != RT_OK) return rc;
        lp.w.P_cap = P_cap;
        lp.list = list + k.first;
        hipLaunchKernelGGL(finish_window_list<T>, dim3((uint32_t)fblocks), dim3(256), 0, st, lp);
        HIPCHK(hipGetLastError());
    }
    return RT_OK;
}

// The checks rt_render*_async and rt_progressive_begin share, after their own of the arguments: the flags
// (live_only: a path that has the live kernels only), the sample and bounce limits, the image and the tile
// range, which *rg receives (range == NULL: the whole image).  count_name: what the entry point calls spp.
static int check_frame(const std::string& who, const rt_camera* cam, uint32_t flags, bool live_only,
                       const char* count_name, uint32_t count, uint32_t max_bounces, const rt_tile_range* range,
                       rt_tile_range* rg) {
    if (flags & ~RT_FLAG_ALL) return fail(RT_ERR_INVALID, who + ": unknown flag bits");
    if (live_only) {
        if (flags & ~RT_FLAG_F32) return fail(RT_ERR_UNSUPPORTED, who + ": the live path only (no RT_FLAG_ROOT2, no RT_FLAG_MODE_*)");
    } else {
        const uint32_t modes = flags & (RT_FLAG_MODE_VECTORIZED | RT_FLAG_MODE_SCALAR | RT_FLAG_MODE_VECTORIZED3);
        if (modes & (modes - 1u))
            return fail(RT_ERR_INVALID, who + ": the RT_FLAG_MODE_* flags are exclusive");
    }
    if (count > (1u << 20)) return fail(RT_ERR_UNSUPPORTED, who + ": " + count_name + " > 2^20");
    if ((flags & RT_FLAG_F32) && max_bounces > RT_MAX_BOUNCES_F32)   // rng<float>'s counter (rt_device.hpp)
        return fail(RT_ERR_UNSUPPORTED, who + ": fp32 with max_bounces > RT_MAX_BOUNCES_F32 (3839)");
    if (cam->image_width == 0 || cam->image_height == 0) return fail(RT_ERR_INVALID, who + ": empty image");
    if ((uint64_t)cam->image_width * cam->image_height > 0xFFFFFFFFull) return fail(RT_ERR_UNSUPPORTED, who + ": image too large");
    *rg = range ? *range : rt_tile_range{0, 1, cam->image_height, 0, cam->image_width};
    if (!check_range(cam, rg)) return fail(RT_ERR_INVALID, who + ": tile range outside the image");
    return RT_OK;
}

// Renders on one context share its work counter, scratch and camera tables: a launch on a new
// stream first waits for the previous stream, so cross-stream use serialises instead of racing.
// st: NULL = the HIP null stream.
static int begin_launch(rt_context* c, hipStream_t st) {
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
static int end_launch(rt_context* c, hipStream_t st, uint64_t pixels, uint64_t samples) {
    HIPCHK(hipEventRecord(c->ev_last, st));
    c->pixels += pixels;
    c->samples += samples;
    return RT_OK;
}

// rt_render_async (split_mode < 0) and rt_render_split_async (split_mode 0: the auto plan; 1: samples_per_item
// forced).  who: the entry point's name, for the error messages.
static int render_async(rt_context* c, const rt_camera* cam, uint32_t max_bounces, uint32_t spp, uint64_t seed,
                        uint32_t flags, const rt_tile_range* range, void* d_rgb8, void* d_linear, void* stream,
                        const char* who_, int split_mode, uint32_t samples_per_item) {
    const std::string who = who_;
    if (!c || !cam) return fail(RT_ERR_INVALID, who + ": NULL argument");
    if (spp == 0) return fail(RT_ERR_INVALID, who + ": spp == 0 (the reference panics: 0/0 in to_u8_array)");
    FrameArgs a{cam, max_bounces, spp, seed, flags, rt_tile_range{}, d_rgb8, d_linear};
    int rc = check_frame(who, cam, flags, false, "spp", spp, max_bounces, range, &a.rg);
    if (rc != RT_OK) return rc;
    const uint64_t n_pix = (uint64_t)a.rg.row_count * a.rg.col_count;
    if (n_pix > 0x7FFFFFFFull) return fail(RT_ERR_UNSUPPORTED, who + ": too many pixels in one call");
    const bool f32 = (flags & RT_FLAG_F32) != 0;
    uint32_t S = spp, nsub = 1u;   // a render's split: S samples per work item, nsub items per pixel
    bool split = false;
    if (split_mode >= 0) {
        if (flags & ~RT_FLAG_F32) return fail(RT_ERR_UNSUPPORTED, who + ": the live path only (no RT_FLAG_ROOT2, no RT_FLAG_MODE_*)");
        const uint32_t P = 4u * ((spp + 3u) / 4u);
        const uint64_t rec_bytes = n_pix * paths_sbytes(P, f32 ? 4u : 8u, paths_wide(P, max_bounces));
        if (split_mode == 0) {
            // resident waves of the split kernels: 4-wave workgroups at their occupancy target on every CU
            const uint32_t waves = (uint32_t)c->n_cu * 4u * (uint32_t)(f32 ? kWavesSplit<float> : kWavesSplit<double>);
            uint64_t n_items = 0;
            const int prc = split_plan(n_pix, spp, waves, &S, &n_items);
            if (prc != kPlanOk) return fail(prc, who + ": no plan for this launch shape");
            nsub = split_nsub(spp, S);
            split = nsub > 1u && rec_bytes <= kScratchBudget;   // else: this call is rt_render_async
        } else {
            if (samples_per_item == 0 || samples_per_item > (1u << 20))
                return fail(RT_ERR_INVALID, who + ": samples_per_item outside 1..2^20");
            S = samples_per_item;
            nsub = split_nsub(spp, S);
            if (n_pix * nsub > 0x7FFFFFFFull) return fail(RT_ERR_UNSUPPORTED, who + ": too many work items in one call");
            if (rec_bytes > kScratchBudget) return fail(RT_ERR_UNSUPPORTED, who + ": record buffer over the scratch budget");
            split = true;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    if ((rc = begin_launch(c, st)) != RT_OK) return rc;
    if (split) rc = f32 ? launch_split<float>(c, a, S, nsub, st) : launch_split<double>(c, a, S, nsub, st);
    else rc = f32 ? launch_plain<float>(c, a, st) : launch_plain<double>(c, a, st);
    if (rc != RT_OK) return rc;
    return end_launch(c, st, n_pix, n_pix * spp);
}

extern "C" int rt_render_async(rt_context* c, const rt_camera* cam, uint32_t max_bounces, uint32_t spp, uint64_t seed,
                               uint32_t flags, const rt_tile_range* range, void* d_rgb8, void* d_linear, void* stream) {
    return render_async(c, cam, max_bounces, spp, seed, flags, range, d_rgb8, d_linear, stream, "rt_render_async", -1, 0u);
}

extern "C" int rt_render_split_async(rt_context* c, const rt_camera* cam, uint32_t max_bounces, uint32_t spp,
                                     uint64_t seed, uint32_t flags, const rt_tile_range* range, void* d_rgb8,
                                     void* d_linear, void* stream, uint32_t samples_per_item) {
    return render_async(c, cam, max_bounces, spp, seed, flags, range, d_rgb8, d_linear, stream, "rt_render_split_async",
                        samples_per_item == 0u ? 0 : 1, samples_per_item);
}

extern "C" int rt_render_guides_async(rt_context* c, const rt_camera* cam, uint32_t spp, uint64_t seed, uint32_t flags,
                                      const rt_tile_range* range, void* d_albedo, void* d_normal, void* d_depth,
                                      void* d_coverage, void* stream) {
    const std::string who = "rt_render_guides_async";
    if (!c || !cam) return fail(RT_ERR_INVALID, who + ": NULL argument");
    if (spp == 0) return fail(RT_ERR_INVALID, who + ": spp == 0");
    if (!d_albedo && !d_normal && !d_depth && !d_coverage) return fail(RT_ERR_INVALID, who + ": all four outputs are NULL");
    // the frame of a render that stops after its first hit: one bounce
    FrameArgs a{cam, 1u, spp, seed, flags, rt_tile_range{}, nullptr, nullptr};
    int rc = check_frame(who, cam, flags, true, "spp", spp, 1u, range, &a.rg);
    if (rc != RT_OK) return rc;
    const uint64_t n_pix = (uint64_t)a.rg.row_count * a.rg.col_count;
    if (n_pix > 0x7FFFFFFFull) return fail(RT_ERR_UNSUPPORTED, who + ": too many pixels in one call");
    hipStream_t st = (hipStream_t)stream;
    if ((rc = begin_launch(c, st)) != RT_OK) return rc;
    rc = (flags & RT_FLAG_F32) ? launch_guides<float>(c, a, (float*)d_albedo, (float*)d_normal, (float*)d_depth, (float*)d_coverage, st)
                               : launch_guides<double>(c, a, (float*)d_albedo, (float*)d_normal, (float*)d_depth, (float*)d_coverage, st);
    if (rc != RT_OK) return rc;
    return end_launch(c, st, n_pix, n_pix * spp);
}

extern "C" int rt_query_hits_async(rt_context* c, uint64_t n_rays, const void* d_origins, const double* origin,
                                   const void* d_directions, uint32_t flags, void* d_t, void* d_index, void* d_normal,
                                   void* d_point, void* d_front, void* stream) {
    const std::string who = "rt_query_hits_async";
    if (!c || !d_directions) return fail(RT_ERR_INVALID, who + ": NULL argument (ctx or d_directions)");
    if ((d_origins != nullptr) == (origin != nullptr))
        return fail(RT_ERR_INVALID, who + ": exactly one of d_origins (per ray) and origin (shared) must be given");
    if (!d_t && !d_index && !d_normal && !d_point && !d_front) return fail(RT_ERR_INVALID, who + ": all five outputs are NULL");
    if (flags & ~RT_FLAG_ALL) return fail(RT_ERR_INVALID, who + ": unknown flag bits");
    if (flags & ~(RT_FLAG_F32 | RT_FLAG_ROOT2))
        return fail(RT_ERR_UNSUPPORTED, who + ": the live path's hit only (RT_FLAG_F32, RT_FLAG_ROOT2; no RT_FLAG_MODE_*)");
    if (n_rays > 0x7FFFFFFFull) return fail(RT_ERR_UNSUPPORTED, who + ": too many rays in one call");
    if (!c->has_scene) return fail(RT_ERR_INVALID, who + ": no scene set (rt_context_set_scene first)");
    if (n_rays == 0) return RT_OK;
    const QueryArgs a{n_rays, d_origins, origin, d_directions, flags, d_t, d_index, d_normal, d_point, d_front};
    hipStream_t st = (hipStream_t)stream;
    int rc = begin_launch(c, st);
    if (rc != RT_OK) return rc;
    rc = (flags & RT_FLAG_F32) ? launch_query<float>(c, a, st) : launch_query<double>(c, a, st);
    if (rc != RT_OK) return rc;
    return end_launch(c, st, n_rays, 0u);   // samples: the valid rays, counted on the device (kQuerySlot)
}

extern "C" int rt_split_plan(uint64_t n_pixels, uint32_t spp, uint32_t resident_waves, uint32_t* samples_per_item,
                             uint64_t* n_items) {
    const int rc = split_plan(n_pixels, spp, resident_waves, samples_per_item, n_items);
    if (rc != kPlanOk) return fail(rc, "rt_split_plan: no plan (NULL output, no pixels or samples, spp > 2^20 or too many items)");
    return RT_OK;
}

// ---- progressive sessions (rt_progressive_plan.hpp) ----
extern "C" int rt_progressive_bytes(uint64_t n_pixels, uint32_t spp_capacity, uint32_t max_bounces, uint32_t flags,
                                    uint64_t* bytes) {
    const int rc = progressive_bytes(n_pixels, spp_capacity, max_bounces, flags, bytes);
    if (rc != kPlanOk)
        return fail(rc, "rt_progressive_bytes: NULL output, no pixels or samples, an unknown flag (invalid); "
                        "spp_capacity > 2^20, more than 0x7FFFFFFF pixels or a flag other than RT_FLAG_F32 (unsupported)");
    return RT_OK;
}

extern "C" int rt_progressive_begin(rt_context* c, const rt_camera* cam, uint32_t max_bounces, uint32_t spp_capacity,
                                    uint64_t seed, uint32_t flags, const rt_tile_range* range, uint64_t max_bytes) {
    const std::string who = "rt_progressive_begin";
    if (!c || !cam) return fail(RT_ERR_INVALID, who + ": NULL argument");
    if (c->prog.open) return fail(RT_ERR_INVALID, who + ": a session is already open on this context");
    if (spp_capacity == 0) return fail(RT_ERR_INVALID, who + ": spp_capacity == 0");
    rt_tile_range rg{};
    const int frc = check_frame(who, cam, flags, true, "spp_capacity", spp_capacity, max_bounces, range, &rg);
    if (frc != RT_OK) return frc;
    const uint64_t n_pix = (uint64_t)rg.row_count * rg.col_count;
    // an extend has one work item per pixel at least
    if (n_pix > kSplitMaxItems) return fail(RT_ERR_UNSUPPORTED, who + ": more than 0x7FFFFFFF work items in one extend");
    uint64_t bytes = 0;
    const int prc = progressive_bytes(n_pix, spp_capacity, max_bounces, flags, &bytes);
    if (prc != kPlanOk) return fail(prc, who + ": no record buffer for this shape");
    const uint32_t P_cap = prog_positions(spp_capacity), tsz = (flags & RT_FLAG_F32) ? 4u : 8u;
    if (bytes != n_pix * paths_sbytes(P_cap, tsz, paths_wide(P_cap, max_bounces)))
        return fail(RT_ERR_INVALID, who + ": internal: rt_progressive_plan.hpp and rt_finish.hpp disagree on a region's size");
    const uint64_t limit = max_bytes ? max_bytes : kScratchBudget;
    if (bytes > limit)
        return fail(RT_ERR_UNSUPPORTED, who + ": the record buffer (" + std::to_string(bytes) + " bytes) is over " +
                                            (max_bytes ? "max_bytes" : "the scratch budget; pass max_bytes"));
    HIPCHK(hipSetDevice(c->device));
    void* rec = nullptr;
    HIPCHK(hipMalloc(&rec, (size_t)bytes));
    rt_context::Session& s = c->prog;
    s = rt_context::Session{};
    s.open = true;
    s.cam = *cam;
    s.rg = rg;
    s.depth = max_bounces;
    s.cap = spp_capacity;
    s.flags = flags;
    s.seed = seed;
    s.rec = rec;
    s.bytes = bytes;
    s.done.assign((size_t)n_pix, 0u);
    return RT_OK;
}

// An extend of a session whose pixels all hold s.done_min samples, to spp_total for every pixel:
// rt_progressive_extend_async, and a map that is uniform.
static int extend_uniform(rt_context* c, const std::string& who, uint32_t spp_total, void* d_rgb8, void* d_linear,
                          void* stream) {
    rt_context::Session& s = c->prog;
    const uint32_t done = s.done_min;
    if (spp_total == 0) return fail(RT_ERR_INVALID, who + ": spp_total == 0");
    if (spp_total < done) return fail(RT_ERR_INVALID, who + ": spp_total below the samples already traced");
    if (spp_total > s.cap) return fail(RT_ERR_INVALID, who + ": spp_total above the session's spp_capacity");
    const bool f32 = (s.flags & RT_FLAG_F32) != 0;
    const uint64_t n_pix = (uint64_t)s.rg.row_count * s.rg.col_count;
    SessionWindow w{(char*)s.rec, s.cap, done, done, 1u, 1u, spp_total > done, d_rgb8 != nullptr || d_linear != nullptr};
    if (!w.trace && !w.finish) return RT_OK;
    if (w.trace) {
        const uint32_t waves = (uint32_t)c->n_cu * 4u * (uint32_t)(f32 ? kWavesSplit<float> : kWavesSplit<double>);
        ProgWindow pw;
        const int prc = progressive_window(n_pix, done, spp_total, waves, &pw);
        if (prc != kPlanOk) return fail(prc, who + ": no plan for this window (more than 0x7FFFFFFF work items)");
        w.S = pw.S;
        w.nsub = pw.nsub;
        w.s_base = pw.base;
    }
    const FrameArgs a = session_frame(s, spp_total, d_rgb8, d_linear);
    hipStream_t st = (hipStream_t)stream;
    int rc = begin_launch(c, st);   // the session shares the counter, scratch and camera tables
    if (rc != RT_OK) return rc;
    rc = f32 ? launch_window<float>(c, a, w, st) : launch_window<double>(c, a, w, st);
    if (rc != RT_OK) return rc;
    if ((rc = end_launch(c, st, n_pix, n_pix * (uint64_t)(spp_total - done))) != RT_OK) return rc;
    if (w.trace) s.run.broken = s.run.started;   // a refinement run's lists no longer say what the pixels hold
    s.set_done(spp_total);
    s.stream = st;
    s.have_stream = true;
    return RT_OK;
}

// One reduction of a call over per-pixel counts: the pixels with counts[p] > 0, each at its count, into the outputs.
struct MapReduce {
    const uint32_t* counts;
    void* rgb;
    void* lin;
};

// The work of the per-pixel-count calls.  Traces [s.done[p], target[p]) of every pixel (target == NULL: nothing),
// then runs the n_red reductions in order; `extra` (n_extra words, may be NULL) is sent to the device behind the
// other tables and *d_extra receives its device address.  The callers have checked the arrays.  Returns with
// *enqueued false when there was nothing to do.
static int run_map(rt_context* c, const std::string& who, const uint32_t* target, const MapReduce* red, size_t n_red,
                   const uint32_t* extra, size_t n_extra, const uint32_t** d_extra, hipStream_t st, bool* enqueued) {
    rt_context::Session& s = c->prog;
    const bool f32 = (s.flags & RT_FLAG_F32) != 0;
    const uint32_t n_pix = s.rg.row_count * s.rg.col_count;
    const uint32_t waves = (uint32_t)c->n_cu * 4u * (uint32_t)(f32 ? kWavesSplit<float> : kWavesSplit<double>);
    *enqueued = false;
    uint32_t S = 0;
    uint64_t n_items = 0, traced = 0;
    if (target) {
        const int prc = progressive_map_plan(n_pix, s.done.data(), target, waves, &S, &n_items, nullptr, 0u);
        if (prc != kPlanOk) return fail(prc, who + ": no plan for this map (more than 0x7FFFFFFF work items)");
        for (uint32_t p = 0; p < n_pix; ++p) traced += target[p] - s.done[p];
    }
    std::vector<std::vector<CountClass>> cls(n_red);
    size_t list_words = 0;
    for (size_t r = 0; r < n_red; ++r) {
        if (!group_by_count(red[r].counts, n_pix, nullptr, cls[r]))
            return fail(RT_ERR_UNSUPPORTED, who + ": more than 256 distinct sample counts in one reduction");
        if (!cls[r].empty()) list_words += n_pix;
    }
    if (n_items == 0 && list_words == 0) return RT_OK;
    // the tables, in one copy: the items' records, the reductions' index lists, the caller's words.  The host
    // fills them before the launch begins, so that the collect's kernel_ms is the device's time alone
    HIPCHK(hipSetDevice(c->device));
    const size_t item_words = (size_t)n_items * kMapItemWords, words = item_words + list_words + n_extra;
    int rc = stage_reserve(s.stage, words * sizeof(uint32_t));
    if (rc != RT_OK) return rc;
    uint32_t* const tab = (uint32_t*)s.stage.p;
    if (n_items && progressive_map_plan(n_pix, s.done.data(), target, waves, &S, &n_items, tab, n_items) != kPlanOk)
        return fail(RT_ERR_INVALID, who + ": internal: the plan's two passes disagree");
    size_t at = item_words;
    std::vector<size_t> list_at(n_red, 0);
    for (size_t r = 0; r < n_red; ++r) {
        if (cls[r].empty()) continue;
        (void)group_by_count(red[r].counts, n_pix, tab + at, cls[r]);
        list_at[r] = at;
        at += n_pix;
    }
    if (n_extra) memcpy(tab + at, extra, n_extra * sizeof(uint32_t));
    if ((rc = begin_launch(c, st)) != RT_OK) return rc;   // the session shares the counter, scratch and camera tables
    if ((rc = send_tables(s, words * sizeof(uint32_t), st)) != RT_OK) return rc;
    const uint32_t* const d_tab = (const uint32_t*)s.tables.p;
    if (d_extra) *d_extra = d_tab + at;
    if (n_items) {
        const uint32_t item_spp = (uint32_t)std::max<uint64_t>(1u, traced / n_items);   // the mean item
        rc = f32 ? launch_items<float>(c, s, (const MapItem*)d_tab, (uint32_t)n_items, item_spp, st)
                 : launch_items<double>(c, s, (const MapItem*)d_tab, (uint32_t)n_items, item_spp, st);
        if (rc != RT_OK) return rc;
    }
    bool set_id = n_items == 0;
    for (size_t r = 0; r < n_red; ++r) {
        if (cls[r].empty()) continue;
        rc = f32 ? launch_classes<float>(c, s, cls[r], d_tab + list_at[r], red[r].rgb, red[r].lin, set_id, st)
                 : launch_classes<double>(c, s, cls[r], d_tab + list_at[r], red[r].rgb, red[r].lin, set_id, st);
        if (rc != RT_OK) return rc;
        set_id = false;
    }
    if (target) {
        if (n_items) s.run.broken = s.run.started;   // as in extend_uniform
        s.done.assign(target, target + n_pix);
        s.done_min = *std::min_element(s.done.begin(), s.done.end());
        s.done_max = *std::max_element(s.done.begin(), s.done.end());
    }
    s.stream = st;
    s.have_stream = true;
    *enqueued = true;
    return end_launch(c, st, n_pix, traced);
}

static int open_session(rt_context* c, const std::string& who) {
    if (!c) return fail(RT_ERR_INVALID, who + ": NULL context");
    if (!c->prog.open) return fail(RT_ERR_INVALID, who + ": no session open on this context");
    return RT_OK;
}

// After a step of rt_progressive_refine the counts are on the device: copy them down (4 bytes per pixel) before
// a call reads `done`.
static int sync_done(rt_context* c) {
    rt_context::Session& s = c->prog;
    if (!s.done_stale) return RT_OK;
    HIPCHK(hipSetDevice(c->device));
    if (s.have_stream) HIPCHK(hipStreamSynchronize(s.stream));
    HIPCHK(hipMemcpy(s.done.data(), s.counts.p, s.done.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    s.done_min = *std::min_element(s.done.begin(), s.done.end());
    s.done_max = *std::max_element(s.done.begin(), s.done.end());
    s.done_stale = false;
    return RT_OK;
}

// ---- refinement on the device (rt_progressive_refine; DESIGN.md §4 "Planning on the device") ----
// finish_window over every pixel of the session at `spp` samples into lin (no tracing).
template <typename T>
static int reduce_uniform(rt_context* c, const rt_context::Session& s, uint32_t spp, void* lin, hipStream_t st) {
    const SessionWindow w{(char*)s.rec, s.cap, spp, spp, 1u, 1u, false, true};
    return launch_window<T>(c, session_frame(s, spp, nullptr, lin), w, st);
}

// rt_progressive_snapshot_map_async(ctx, NULL, ...) of a session in an unbroken run: one finish_window_list per
// class the run has built, then one over the candidates of its next step, which all hold n_k samples.
static int snapshot_run(rt_context* c, void* d_rgb8, void* d_linear, hipStream_t st) {
    rt_context::Session& s = c->prog;
    const rt_context::Session::Refine& r = s.run;
    const bool f32 = (s.flags & RT_FLAG_F32) != 0;
    int rc = begin_launch(c, st);
    if (rc != RT_OK) return rc;
    if (!r.cls.empty()) {
        const uint32_t* list = (const uint32_t*)s.cls_list.p;
        rc = f32 ? launch_classes<float>(c, s, r.cls, list, d_rgb8, d_linear, true, st)
                 : launch_classes<double>(c, s, r.cls, list, d_rgb8, d_linear, true, st);
        if (rc != RT_OK) return rc;
    }
    if (r.n_cand) {
        const std::vector<CountClass> last{CountClass{r.n_k, 0u, r.n_cand}};
        const uint32_t* list = (const uint32_t*)s.act[r.cur].p;
        rc = f32 ? launch_classes<float>(c, s, last, list, d_rgb8, d_linear, r.cls.empty(), st)
                 : launch_classes<double>(c, s, last, list, d_rgb8, d_linear, r.cls.empty(), st);
        if (rc != RT_OK) return rc;
    }
    s.stream = st;
    s.have_stream = true;
    return end_launch(c, st, (uint64_t)s.rg.row_count * s.rg.col_count, 0u);
}

extern "C" int rt_progressive_refine(rt_context* c, double tolerance, uint32_t spp_max, void* stream,
                                     uint64_t* n_active, uint64_t* n_samples) {
    const std::string who = "rt_progressive_refine";
    if (!c || !n_active || !n_samples) return fail(RT_ERR_INVALID, who + ": NULL argument");
    *n_active = 0;
    *n_samples = 0;
    if (!c->prog.open) return fail(RT_ERR_INVALID, who + ": no session open on this context");
    if (tolerance != tolerance) return fail(RT_ERR_INVALID, who + ": tolerance is NaN");
    rt_context::Session& s = c->prog;
    rt_context::Session::Refine& r = s.run;
    if (r.started) {
        if (tolerance != r.tol || spp_max != r.spp_max)
            return fail(RT_ERR_INVALID, who + ": tolerance or spp_max differs from the run's first call");
        if (r.broken)
            return fail(RT_ERR_UNSUPPORTED, who + ": another call has traced into the session since the run's last "
                                                  "step (rt_progressive_extend_map_async takes any map)");
    } else {
        if (spp_max > s.cap) return fail(RT_ERR_INVALID, who + ": spp_max above the session's spp_capacity");
        if (spp_max < s.done_max) return fail(RT_ERR_INVALID, who + ": spp_max below the samples a pixel already holds");
        if (s.done_min != s.done_max)
            return fail(RT_ERR_UNSUPPORTED, who + ": a run starts on a uniform session (rt_progressive_extend_map_async "
                                                  "takes any map)");
        if (s.done_min == 0u) return fail(RT_ERR_INVALID, who + ": the session holds no sample yet");
    }
    const bool first = !r.started, f32 = (s.flags & RT_FLAG_F32) != 0;
    const uint32_t n_pix = s.rg.row_count * s.rg.col_count;
    const uint32_t n_k = first ? s.done_min : r.n_k, n_cand = first ? n_pix : r.n_cand;
    if (!first && (n_cand == 0u || n_k >= spp_max)) {   // converged, or every candidate is at the cap
        r.S = 0u;
        r.n_items = 0u;   // this step built no table
        return RT_OK;
    }
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(c->device));
    int rc = RT_OK;
    if (first) {
        const size_t words = (size_t)n_pix * sizeof(uint32_t), lin_bytes = (size_t)n_pix * 3u * sizeof(double);
        const size_t blocks = ((size_t)n_pix + kRefineBlock - 1u) / kRefineBlock;
        for (DeviceBuffer* b : {&s.counts, &s.act[0], &s.act[1], &s.cls_list})
            if ((rc = reserve(*b, words)) != RT_OK) return rc;
        if ((rc = reserve(s.sel, n_pix)) != RT_OK) return rc;
        if ((rc = reserve(s.blk, blocks * sizeof(uint32_t))) != RT_OK) return rc;
        if ((rc = reserve(s.ret, 4u * sizeof(uint32_t))) != RT_OK) return rc;
        if ((rc = reserve(s.lin_cur, lin_bytes)) != RT_OK) return rc;
        if ((rc = reserve(s.lin_new, lin_bytes)) != RT_OK) return rc;
    }
    if ((rc = stage_reserve(s.stage, 4u * sizeof(uint32_t))) != RT_OK) return rc;
    if ((rc = begin_launch(c, st)) != RT_OK) return rc;   // the session shares the counter, scratch and camera tables
    // the estimate's reductions: the whole frame at n0 / 2 and n0 at first, later the candidates alone at n_k,
    // whose values at n_k / 2 (the count they held a step ago) are still in lin_cur
    const uint32_t* const list = first ? nullptr : (const uint32_t*)s.act[r.cur].p;
    if (first) {
        if (n_k >= 2u) {
            rc = f32 ? reduce_uniform<float>(c, s, n_k / 2u, s.lin_cur.p, st) : reduce_uniform<double>(c, s, n_k / 2u, s.lin_cur.p, st);
            if (rc != RT_OK) return rc;
        }
        rc = f32 ? reduce_uniform<float>(c, s, n_k, s.lin_new.p, st) : reduce_uniform<double>(c, s, n_k, s.lin_new.p, st);
    } else {
        const std::vector<CountClass> cand{CountClass{n_k, 0u, n_cand}};
        rc = f32 ? launch_classes<float>(c, s, cand, list, nullptr, s.lin_new.p, true, st)
                 : launch_classes<double>(c, s, cand, list, nullptr, s.lin_new.p, true, st);
    }
    if (rc != RT_OK) return rc;
    // select, scan, scatter: the next active list into the other act buffer, the rest behind the earlier classes
    const uint32_t nb = (n_cand + kRefineBlock - 1u) / kRefineBlock;
    const int nxt = first ? 0 : 1 - r.cur;
    uint32_t* const d_blk = (uint32_t*)s.blk.p;
    hipLaunchKernelGGL(refine_select, dim3(nb), dim3(kRefineBlock), 0, st, list, n_cand, n_k, tolerance,
                       n_k < spp_max ? 1u : 0u, (double*)s.lin_cur.p, (const double*)s.lin_new.p, (uint32_t*)s.counts.p,
                       (uint8_t*)s.sel.p, d_blk);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(refine_scan, dim3(1), dim3(kRefineBlock), 0, st, d_blk, nb, (uint32_t*)s.ret.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(refine_scatter, dim3(nb), dim3(kRefineBlock), 0, st, list, n_cand, (const uint8_t*)s.sel.p,
                       (const uint32_t*)d_blk, (uint32_t*)s.act[nxt].p, (uint32_t*)s.cls_list.p + r.cls_used);
    HIPCHK(hipGetLastError());
    // the step's one readback, and its one wait: how many pixels go on
    HIPCHK(hipMemcpyAsync(s.stage.p, s.ret.p, 4u * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint32_t A = *(const volatile uint32_t*)s.stage.p;
    if (A > n_cand) return fail(RT_ERR_HIP, who + ": internal: more active pixels than candidates");
    if (n_cand - A) r.cls.push_back(CountClass{n_k, r.cls_used, n_cand - A});
    r.cls_used += n_cand - A;
    r.started = true;
    r.tol = tolerance;
    r.spp_max = spp_max;
    r.cur = nxt;
    r.n_cand = A;
    r.n_k = n_k;
    r.S = 0u;
    r.n_items = 0u;
    s.done_stale = true;
    s.stream = st;
    s.have_stream = true;
    if (A == 0u) return end_launch(c, st, n_pix, 0u);
    // the plan: rt_progressive_map_plan's for A pixels that all go from n_k to t (its mean is exact)
    const uint32_t t = (uint32_t)std::min<uint64_t>(2ull * n_k, spp_max);
    const uint32_t waves = (uint32_t)c->n_cu * 4u * (uint32_t)(f32 ? kWavesSplit<float> : kWavesSplit<double>);
    uint32_t S = 0;
    uint64_t planned = 0;
    const int prc = split_plan(A, t - n_k, waves, &S, &planned);
    const bool grid = prc == kPlanOk && S % kSplitGrain == 0u;
    const uint32_t base = grid ? n_k - n_k % kSplitGrain : n_k;
    const uint32_t nsub = grid ? split_nsub(t - base, S) : 1u;
    const uint64_t n_items = (uint64_t)A * nsub;
    if (prc != kPlanOk || n_items > kSplitMaxItems) {
        r.broken = true;   // the active pixels stay at n_k, as the device counts say
        return fail(prc != kPlanOk ? prc : RT_ERR_UNSUPPORTED, who + ": no plan for this step (more than 0x7FFFFFFF work items)");
    }
    if ((rc = ensure_bytes(s.items, (size_t)n_items * sizeof(MapItem), st)) != RT_OK) return rc;
    hipLaunchKernelGGL(refine_expand, dim3((A + kRefineBlock - 1u) / kRefineBlock), dim3(kRefineBlock), 0, st,
                       (const uint32_t*)s.act[nxt].p, A, (uint32_t*)s.counts.p, n_k, t, base, grid ? S : t - n_k, nsub,
                       (MapItem*)s.items.p);
    HIPCHK(hipGetLastError());
    const uint64_t traced = (uint64_t)A * (t - n_k);
    const uint32_t item_spp = (uint32_t)std::max<uint64_t>(1u, traced / n_items);   // the mean item, as run_map
    rc = f32 ? launch_items<float>(c, s, (const MapItem*)s.items.p, (uint32_t)n_items, item_spp, st)
             : launch_items<double>(c, s, (const MapItem*)s.items.p, (uint32_t)n_items, item_spp, st);
    if (rc != RT_OK) return rc;
    r.n_k = t;
    r.S = S;
    r.n_items = n_items;
    *n_active = A;
    *n_samples = traced;
    return end_launch(c, st, n_pix, traced);
}

extern "C" int rt_progressive_refine_items(rt_context* c, uint32_t* samples_per_item, uint64_t* n_items, uint32_t* items,
                                           uint64_t items_capacity) {
    const std::string who = "rt_progressive_refine_items";
    if (!c || !samples_per_item || !n_items) return fail(RT_ERR_INVALID, who + ": NULL argument");
    *samples_per_item = 0;
    *n_items = 0;
    if (!c->prog.open) return fail(RT_ERR_INVALID, who + ": no session open on this context");
    rt_context::Session& s = c->prog;
    *samples_per_item = s.run.n_items ? s.run.S : 0u;
    *n_items = s.run.n_items;
    if (!items || s.run.n_items == 0u) return RT_OK;
    if (items_capacity < s.run.n_items) return fail(RT_ERR_INVALID, who + ": items_capacity below the item count");
    HIPCHK(hipSetDevice(c->device));
    if (s.have_stream) HIPCHK(hipStreamSynchronize(s.stream));
    HIPCHK(hipMemcpy(items, s.items.p, (size_t)s.run.n_items * sizeof(MapItem), hipMemcpyDeviceToHost));
    return RT_OK;
}

extern "C" int rt_progressive_extend_async(rt_context* c, uint32_t spp_total, void* d_rgb8, void* d_linear, void* stream) {
    const std::string who = "rt_progressive_extend_async";
    int rc = open_session(c, who);
    if (rc != RT_OK) return rc;
    if ((rc = sync_done(c)) != RT_OK) return rc;
    rt_context::Session& s = c->prog;
    if (s.done_min == s.done_max) return extend_uniform(c, who, spp_total, d_rgb8, d_linear, stream);
    // after a non-uniform map: every pixel goes from its own count to spp_total
    if (spp_total < s.done_max) return fail(RT_ERR_INVALID, who + ": spp_total below the samples a pixel already holds");
    if (spp_total > s.cap) return fail(RT_ERR_INVALID, who + ": spp_total above the session's spp_capacity");
    const std::vector<uint32_t> target(s.done.size(), spp_total);
    const MapReduce red{target.data(), d_rgb8, d_linear};
    bool enqueued = false;
    return run_map(c, who, target.data(), &red, d_rgb8 || d_linear ? 1u : 0u, nullptr, 0u, nullptr, (hipStream_t)stream,
                   &enqueued);
}

extern "C" int rt_progressive_extend_map_async(rt_context* c, const uint32_t* spp_target, void* d_rgb8, void* d_linear,
                                               void* stream) {
    const std::string who = "rt_progressive_extend_map_async";
    int rc = open_session(c, who);
    if (rc != RT_OK) return rc;
    rt_context::Session& s = c->prog;
    if (!spp_target) return fail(RT_ERR_INVALID, who + ": spp_target is NULL");
    if ((rc = sync_done(c)) != RT_OK) return rc;
    const bool out = d_rgb8 != nullptr || d_linear != nullptr;
    bool same = s.done_min == s.done_max;
    for (size_t p = 0; p < s.done.size(); ++p) {
        const uint32_t t = spp_target[p];
        if (t < s.done[p]) return fail(RT_ERR_INVALID, who + ": a target below the samples its pixel already holds");
        if (t > s.cap) return fail(RT_ERR_INVALID, who + ": a target above the session's spp_capacity");
        if (t == 0u && out) return fail(RT_ERR_INVALID, who + ": a target of 0 with an output (no image of 0 samples)");
        same = same && t == spp_target[0];
    }
    if (same)   // a uniform map is rt_progressive_extend_async: same kernels, same stats
        return spp_target[0] == 0u ? RT_OK : extend_uniform(c, who, spp_target[0], d_rgb8, d_linear, stream);
    const MapReduce red{spp_target, d_rgb8, d_linear};
    bool enqueued = false;
    return run_map(c, who, spp_target, &red, out ? 1u : 0u, nullptr, 0u, nullptr, (hipStream_t)stream, &enqueued);
}

extern "C" int rt_progressive_snapshot_map_async(rt_context* c, const uint32_t* spp_count, void* d_rgb8, void* d_linear,
                                                 void* stream) {
    const std::string who = "rt_progressive_snapshot_map_async";
    int rc = open_session(c, who);
    if (rc != RT_OK) return rc;
    rt_context::Session& s = c->prog;
    if (!d_rgb8 && !d_linear) return fail(RT_ERR_INVALID, who + ": both outputs are NULL");
    // every pixel at its own count, during or after a refinement run: the classes are already on the device
    if (!spp_count && s.run.started && !s.run.broken) return snapshot_run(c, d_rgb8, d_linear, (hipStream_t)stream);
    if ((rc = sync_done(c)) != RT_OK) return rc;
    const uint32_t* counts = spp_count ? spp_count : s.done.data();
    for (size_t p = 0; p < s.done.size(); ++p)
        if (counts[p] == 0u || counts[p] > s.done[p])
            return fail(RT_ERR_INVALID, who + ": a count of 0 or above the samples its pixel holds");
    const MapReduce red{counts, d_rgb8, d_linear};
    bool enqueued = false;
    return run_map(c, who, nullptr, &red, 1u, nullptr, 0u, nullptr, (hipStream_t)stream, &enqueued);
}

extern "C" int rt_progressive_counts(rt_context* c, uint32_t* out) {
    const std::string who = "rt_progressive_counts";
    int rc = open_session(c, who);
    if (rc != RT_OK) return rc;
    if (!out) return fail(RT_ERR_INVALID, who + ": out is NULL");
    if ((rc = sync_done(c)) != RT_OK) return rc;
    std::copy(c->prog.done.begin(), c->prog.done.end(), out);
    return RT_OK;
}

extern "C" int rt_progressive_error_async(rt_context* c, void* d_error, void* stream) {
    const std::string who = "rt_progressive_error_async";
    int rc = open_session(c, who);
    if (rc != RT_OK) return rc;
    rt_context::Session& s = c->prog;
    if (!d_error) return fail(RT_ERR_INVALID, who + ": d_error is NULL");
    if ((rc = sync_done(c)) != RT_OK) return rc;
    const uint32_t n_pix = (uint32_t)s.done.size();
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(c->device));
    const size_t lin_bytes = (size_t)n_pix * 3u * sizeof(double);
    if ((rc = ensure_bytes(s.lin_full, lin_bytes, st)) != RT_OK) return rc;
    if ((rc = ensure_bytes(s.lin_half, lin_bytes, st)) != RT_OK) return rc;
    // the snapshot at half the count, then at the count; a pixel below 2 samples has no half (0: left out) and
    // reads +inf, whatever its buffers hold
    std::vector<uint32_t> half(s.done);
    for (uint32_t& n : half) n /= 2u;
    const MapReduce red[2] = {{half.data(), nullptr, s.lin_half.p}, {s.done.data(), nullptr, s.lin_full.p}};
    const uint32_t* d_counts = nullptr;
    bool enqueued = false;
    if ((rc = run_map(c, who, nullptr, red, 2u, s.done.data(), n_pix, &d_counts, st, &enqueued)) != RT_OK) return rc;
    if (!enqueued) {   // no pixel holds a sample: every estimate is +inf, and the counts have not gone up
        if ((rc = begin_launch(c, st)) != RT_OK) return rc;
        if ((rc = stage_reserve(s.stage, (size_t)n_pix * sizeof(uint32_t))) != RT_OK) return rc;
        memcpy(s.stage.p, s.done.data(), (size_t)n_pix * sizeof(uint32_t));
        if ((rc = send_tables(s, (size_t)n_pix * sizeof(uint32_t), st)) != RT_OK) return rc;
        d_counts = (const uint32_t*)s.tables.p;
        s.stream = st;
        s.have_stream = true;
    }
    hipLaunchKernelGGL(progressive_error, dim3((n_pix + 255u) / 256u), dim3(256), 0, st, (const double*)s.lin_full.p,
                       (const double*)s.lin_half.p, d_counts, (double*)d_error, n_pix);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev_last, st));   // kernel_ms covers the estimate's kernel as well
    return RT_OK;
}

extern "C" int rt_progressive_map_plan(uint64_t n_pixels, const uint32_t* done, const uint32_t* target,
                                       uint32_t resident_waves, uint32_t* samples_per_item, uint64_t* n_items,
                                       uint32_t* items, uint64_t items_capacity) {
    const int rc = progressive_map_plan(n_pixels, done, target, resident_waves, samples_per_item, n_items, items,
                                        items_capacity);
    if (rc != kPlanOk)
        return fail(rc, "rt_progressive_map_plan: a NULL array or output, no pixels, a target below done, too small an "
                        "item capacity (invalid); a target above 2^20, more than 0x7FFFFFFF pixels or items (unsupported)");
    return RT_OK;
}

extern "C" int rt_progressive_end(rt_context* c) {
    if (!c) return fail(RT_ERR_INVALID, "rt_progressive_end: NULL context");
    rt_context::Session& s = c->prog;
    if (!s.open) return fail(RT_ERR_INVALID, "rt_progressive_end: no session open on this context");
    HIPCHK(hipSetDevice(c->device));
    if (s.have_stream) HIPCHK(hipStreamSynchronize(s.stream));
    HIPCHK(hipFree(s.rec));
    s = rt_context::Session{};
    return RT_OK;
}

extern "C" int rt_context_collect(rt_context* c, void* stream, rt_stats* out) {
    if (!c) return fail(RT_ERR_INVALID, "rt_context_collect: NULL context");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;   // NULL = the HIP null stream
    HIPCHK(hipStreamSynchronize(st));
    std::vector<unsigned long long> segs(kSegShards * kSegStride);
    uint32_t err = 0;
    HIPCHK(hipMemcpy(segs.data(), c->segs.p, segs.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&err, c->err.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
    float ms = 0.f;
    if (c->have_first) HIPCHK(hipEventElapsedTime(&ms, c->ev_first, c->ev_last));
    HIPCHK(hipMemset(c->segs.p, 0, segs.size() * sizeof(unsigned long long)));
    HIPCHK(hipMemset(c->err.p, 0, 16));
    uint64_t total = 0, slots = 0, iters = 0, dsky = 0, qrays = 0, kst[kNKstat] = {}, work[kNWork] = {};
    for (int i = 0; i < kSegShards; ++i)
        for (int j = 0; j < kNKstat; ++j) kst[j] += segs[(size_t)i * kSegStride + kstat_slot(j)];
    if (kst[0] | kst[1] | kst[2] | kst[3]) {   // instrumented build (make kstats) only
        fprintf(stderr, "rt_kstats: general taken_groups %llu sweeps %llu clusters %llu top_groups %llu  camera "
                "candidates %llu sweeps %llu  finish_pixel %llu  filter_lanes_passing %llu\n",
                (unsigned long long)kst[0], (unsigned long long)kst[1], (unsigned long long)kst[4],
                (unsigned long long)kst[5], (unsigned long long)kst[2], (unsigned long long)kst[3],
                (unsigned long long)kst[6], (unsigned long long)kst[7]);
        // ... and the flush scope of the fp32 scene-frame sweeps (counters 8..12)
        fprintf(stderr, "rt_kstats: flush steps_per_super_max %llu steps_per_sweep_max %llu lanes_two_supers %llu "
                "lanes_any %llu lanes_two_pairs %llu\n", (unsigned long long)kst[8], (unsigned long long)kst[9],
                (unsigned long long)kst[10], (unsigned long long)kst[11], (unsigned long long)kst[12]);
    }
    for (int i = 0; i < kSegShards; ++i) {
        total += segs[(size_t)i * kSegStride];
        slots += segs[(size_t)i * kSegStride + 1];
        iters += segs[(size_t)i * kSegStride + 2];
        dsky += segs[(size_t)i * kSegStride + kDirectSkySlot];
        qrays += segs[(size_t)i * kSegStride + kQuerySlot];   // the valid rays of the queries
        for (uint32_t j = 0; j < kNWork; ++j) work[j] += segs[(size_t)i * kSegStride + kWorkSlot + j];
    }
    if (out) {
        memset(out, 0, sizeof(*out));
        out->kernel_ms = ms;
        out->pixels = c->pixels;
        out->samples = c->samples + qrays;
        out->ray_segments = total;
        out->lane_slots = slots;
        out->bounce_iters = iters;
        out->pixels_per_second = ms > 0.f ? (double)c->pixels / ((double)ms * 1e-3) : 0.0;
        out->box_groups = work[kWBox];
        out->filter_groups = work[kWFilt];
        out->exact_tests = work[kWExact];
        out->cone_tests = work[kWCone];
        out->camera_exact_tests = work[kWCExact];
        out->direct_sky_samples = dsky;
        out->kernel_id = c->last_kernel_id;
        out->kernel_wg_per_cu = c->last_wg_per_cu;
    }
    c->have_first = false;
    c->pixels = c->samples = 0;
    c->last_kernel_id = c->last_wg_per_cu = 0;
    if (err) return fail(RT_ERR_RANGE, "a pixel channel exceeded 2.0 (Color::to_u8_array would panic, color.rs:55-57)");
    return RT_OK;
}

extern "C" int rt_device_alloc(rt_context* c, size_t bytes, void** out) {
    if (!c || !out) return fail(RT_ERR_INVALID, "rt_device_alloc: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMalloc(out, bytes ? bytes : 1));
    return RT_OK;
}
extern "C" int rt_device_free(rt_context* c, void* ptr) {
    if (!c) return fail(RT_ERR_INVALID, "rt_device_free: NULL context");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipFree(ptr));
    return RT_OK;
}
extern "C" int rt_memcpy_d2h(rt_context* c, void* dst, const void* src, size_t bytes) {
    if (!c || !dst || !src) return fail(RT_ERR_INVALID, "rt_memcpy_d2h: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
}

extern "C" int rt_memcpy_h2d(rt_context* c, void* dst, const void* src, size_t bytes) {
    if (!c || !dst || !src) return fail(RT_ERR_INVALID, "rt_memcpy_h2d: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return RT_OK;
}

extern "C" int rt_render(const rt_scene* scene, const rt_camera* cam, uint32_t max_bounces, uint32_t spp, uint64_t seed,
                         uint32_t flags, const rt_tile_range* range, uint8_t* rgb8, double* linear, rt_stats* stats) {
    if (!scene || !cam) return fail(RT_ERR_INVALID, "rt_render: NULL argument");
    const auto t0 = std::chrono::steady_clock::now();
    rt_context* c = nullptr;
    int rc = rt_context_create(0, &c);
    if (rc != RT_OK) return rc;
    struct Guard { rt_context* c; void* a = nullptr; void* b = nullptr;
        ~Guard() { if (a) rt_device_free(c, a); if (b) rt_device_free(c, b); rt_context_destroy(c); } } g{c};
    rc = rt_context_set_scene(c, scene);
    if (rc != RT_OK) return rc;
    const rt_tile_range rg = range ? *range : rt_tile_range{0, 1, cam->image_height, 0, cam->image_width};
    const size_t npx = (size_t)rg.row_count * rg.col_count;
    if (rgb8 && (rc = rt_device_alloc(c, npx * 3, &g.a)) != RT_OK) return rc;
    if (linear && (rc = rt_device_alloc(c, npx * 3 * sizeof(double), &g.b)) != RT_OK) return rc;
    rc = rt_render_async(c, cam, max_bounces, spp, seed, flags, &rg, g.a, g.b, nullptr);
    if (rc != RT_OK) return rc;
    rt_stats st;
    const int crc = rt_context_collect(c, nullptr, &st);
    if (crc != RT_OK && crc != RT_ERR_RANGE) return crc;
    if (rgb8 && (rc = rt_memcpy_d2h(c, rgb8, g.a, npx * 3)) != RT_OK) return rc;
    if (linear && (rc = rt_memcpy_d2h(c, linear, g.b, npx * 3 * sizeof(double))) != RT_OK) return rc;
    st.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    st.pixels_per_second = st.seconds > 0 ? (double)st.pixels / st.seconds : 0.0;
    if (stats) *stats = st;
    if (crc == RT_ERR_RANGE) return fail(RT_ERR_RANGE, "a pixel channel exceeded 2.0 (Color::to_u8_array would panic, color.rs:55-57)");
    return RT_OK;
}
