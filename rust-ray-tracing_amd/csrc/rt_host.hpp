// rt_host.hpp — the base of the C ABI's host code: the error state, owned device and pinned memory, a scene's
// device tables, and the two steps that turn them into kernel arguments (scene_params, cam_table_params) with the
// build_cam_table launch that fills the camera tables.  Host only.  It knows nothing of rt_context: the library
// (rt_launch.hpp) and the test-only device library (tests/device/rt_devunit.hip) both build their KParams here.
#pragma once
#include "rt_camera.hpp"
#include "rt_layout.hpp"

#include <string>
#include <type_traits>

namespace rt {

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

// ---- run-time values as template arguments ----
// f(T()) with T the precision of a launch: float (f32) or double.  The one place a precision flag picks a type.
template <typename F> static auto with_precision(bool f32, F&& f) { return f32 ? f(float()) : f(double()); }
// f(std::bool_constant<b>()...) for the bools that follow f: camera batches, the mega level, a query's root2 / shared.
template <bool... Bs, typename F> static auto with_bools(F&& f) { return f(std::bool_constant<Bs>()...); }
template <bool... Bs, typename F, typename... Rest> static auto with_bools(F&& f, bool b, Rest... rest) {
    return b ? with_bools<Bs..., true>(f, rest...) : with_bools<Bs..., false>(f, rest...);
}

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
    DeviceBuffer cen, rsph, rfsph, rflat, top, sup, lfs, lbx[4], clus, mats;
    DeviceBuffer camx, cull, cullc;   // per slot: camera-origin, cone-cull; cone-cull per cluster
    TableConsts k;
    struct CamKey { bool valid = false; double center[3] = {0, 0, 0}; uint32_t scalar = 0, off = 0; } camkey;
    void reset() { *this = DeviceScene(); }
};
template <typename T> static int upload_scene(DeviceScene<T>& d, const SceneTables<T>& t) {
    int rc = RT_OK;
    auto up = [&](DeviceBuffer& dst, const auto& v) { if (rc == RT_OK) rc = upload(dst, v); };
    auto room = [&](DeviceBuffer& dst, size_t bytes) { if (rc == RT_OK) rc = reserve(dst, bytes); };
    up(d.cen, t.cen);
    up(d.rsph, t.rsph); up(d.rfsph, t.rfsph); up(d.rflat, t.rflat);
    up(d.top, t.top); up(d.sup, t.sup);   // t.meg stays on the host: the mega kernels read the local levels (lbx)
    up(d.lfs, t.lfs);
    for (int lv = 0; lv < 4; ++lv) up(d.lbx[lv], t.lbx[lv]);
    up(d.clus, t.clus); up(d.mats, t.mats);
    room(d.camx, t.cam_bytes.camx); room(d.cull, t.cam_bytes.cull); room(d.cullc, t.cam_bytes.cullc);
    d.k = t.k;
    return rc;
}

// The scene half of the kernel arguments: the tables of this precision, the two tables both precisions share
// (ridx: slot -> scene index; mtiers: the mega walk's order table), the constants and the counts.  filter_off
// (RT_FILTER_OFF, diagnostics): every general-sweep and camera-sweep group goes through the exact test.  The
// owner's counters (segs, err, counter) are the caller's to set.
template <typename T>
static void scene_params(const DeviceScene<T>& d, const SceneCounts& n, const DeviceBuffer& ridx, const DeviceBuffer& mtiers,
                         bool filter_off, KParams<T>& p) {
    p.cen = (const T*)d.cen.p;
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
    p.mtiers = (const uint64_t*)mtiers.p;
    for (int a = 0; a < 3; ++a) { p.mt_lo[a] = n.mt_lo[a]; p.mt_n[a] = n.mt_n[a]; }
    p.mt_inv = n.mt_inv;
    p.l_r2max = d.k.l_r2max;
    p.l_hir2 = d.k.l_hir2;
    p.l_isr = d.k.l_isr;
    p.ridx = (const uint32_t*)ridx.p;
    p.n_top = n.n_top;
    p.n_xg = n.n_xg;
    p.n_xs = n.n_xs;
    p.f_cmax = filter_off ? std::numeric_limits<float>::infinity() : d.k.f_cmax;
    p.f_r2max = d.k.f_r2max;
    p.f_ir2 = d.k.f_ir2;
    p.f_hir2 = d.k.f_hir2;
    p.f_isr = d.k.f_isr;
    p.mats = (const MatT<T>*)d.mats.p;
    p.n_spheres = n.n_spheres;
}

// Camera batches + camera-origin tables (every primary ray starts at the centre): point p at the camera tables
// of this precision.  What they hold is launch_cam_table's.
template <typename T>
static void cam_table_params(const DeviceScene<T>& d, const SceneCounts& n, KParams<T>& p) {
    p.camx = (const T*)d.camx.p;
    p.cull = (const float*)d.cull.p;
    p.cullc = (const float*)d.cullc.p;
    p.n_clp = n.n_clp;
    p.n_supc = n.n_supc;
}

// build_cam_table on st: the scene's camera tables for primary rays that start at `center`.
template <typename T>
static int launch_cam_table(const DeviceScene<T>& d, const SceneCounts& n, const DeviceBuffer& ridx, const T center[3],
                            bool scalar, bool filter_off, hipStream_t st) {
    const uint32_t n_thr = std::max(n.n_cslots, n.n_clp + n.n_supc);
    auto build = scalar ? build_cam_table<T, true> : build_cam_table<T, false>;
    hipLaunchKernelGGL(build, dim3((n_thr + 255) / 256), dim3(256), 0, st, (const T*)d.cen.p, center[0], center[1],
                       center[2], (uint32_t)filter_off, (T*)d.camx.p, (float*)d.cull.p, (const uint32_t*)ridx.p,
                       n.n_cslots, (const double*)d.clus.p, (float*)d.cullc.p, n.n_clp + n.n_supc);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

}  // namespace rt
