// rt_devunit.hip — TEST INFRASTRUCTURE ONLY: the kernel's device math (csrc/rt_device.hpp, rt_common.hpp,
// rt_sweep.hpp), one function per map kernel, out[i] = f(in[i]), behind a C ABI (tests/devunit_bind.py,
// tests/test_gpu_device_math.py), and two probes of whole stages on chosen lanes: the sweeps (the ray probe,
// tests/test_gpu_cull_probe.py) and next_ray (the next-ray probe, tests/test_gpu_scatter.py).  Built by `make devunit` with the product's flags into
// lib/librt_devunit.so; the product library never links it and it is not part of the source hash.
//
// Launch shape: 256-thread blocks, n a multiple of 256 (the binding pads with in-contract values), no
// early return: every lane of every wave holds an input the test chose, so the wave ballots inside
// dvs / sqrt_len see nothing else.  Vectors are component-major: x at [i], y at [n + i], z at [2n + i].
// Every entry point takes host pointers, allocates, copies, launches, synchronises, copies back, frees,
// and returns the HIP error as an int (-1: n is no multiple of 256).
#include "rt_sweep.hpp"
#include "rt_camera.hpp"
#include "rt_layout.hpp"
#include "rt_host.hpp"   // the product's device tables and kernel arguments, for the ray probe
#include "rt_launch.hpp" // frame_params: the frame half of the kernel arguments, for the next-ray probe

using namespace rt;

namespace {

constexpr unsigned kBlock = 256;

// Device buffers of one call: freed on scope exit, the first HIP error kept.
struct Dev {
    std::vector<void*> ptrs;
    hipError_t err = hipSuccess;
    void note(hipError_t e) { if (err == hipSuccess && e != hipSuccess) err = e; }
    template <typename T> T* out(size_t n) {
        void* d = nullptr;
        if (err != hipSuccess) return nullptr;
        note(hipMalloc(&d, (n ? n : 1) * sizeof(T)));
        if (d) ptrs.push_back(d);
        return (T*)d;
    }
    template <typename T> T* in(const T* h, size_t n) {
        T* d = out<T>(n);
        if (d && n) note(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice));
        return d;
    }
    template <typename T> void back(T* h, const T* d, size_t n) {
        if (err == hipSuccess && n) note(hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost));
    }
    void sync() {
        if (err != hipSuccess) return;
        note(hipGetLastError());
        note(hipDeviceSynchronize());
    }
    bool ok() const { return err == hipSuccess; }
    ~Dev() { for (void* p : ptrs) (void)hipFree(p); }
};

__device__ __forceinline__ size_t gid() { return (size_t)blockIdx.x * kBlock + threadIdx.x; }
template <typename T> __device__ __forceinline__ V3<T> ld3(const T* v, size_t n, size_t i) { return mk(v[i], v[n + i], v[2 * n + i]); }
template <typename T> __device__ __forceinline__ void st3(T* o, size_t n, size_t i, V3<T> r) { o[i] = r.x; o[n + i] = r.y; o[2 * n + i] = r.z; }

template <typename T> __global__ void k_unit(const T* v, T* o, size_t n) { const size_t i = gid(); st3(o, n, i, unit(ld3(v, n, i))); }
template <typename T> __global__ void k_dvs(const T* v, const T* s, T* o, size_t n) { const size_t i = gid(); st3(o, n, i, dvs(ld3(v, n, i), s[i])); }
template <typename T> __global__ void k_sqrt_nd(const T* x, T* o, size_t) { const size_t i = gid(); o[i] = sqrt_nd(x[i]); }
template <typename T> __global__ void k_sqrt_len(const T* x, T* o, size_t) { const size_t i = gid(); o[i] = sqrt_len(x[i]); }
template <typename T> __global__ void k_sincos(const T* u, T* so, T* co, size_t) {
    const size_t i = gid();
    T s, c;
    sincos2pi(u[i], s, c);
    so[i] = s; co[i] = c;
}
template <typename T> __global__ void k_unit_vec(const T* u1, const T* u2, T* o, size_t n) { const size_t i = gid(); st3(o, n, i, unit_vec(u1[i], u2[i])); }
template <typename T> __global__ void k_refract(const T* v, const T* nn, const T* ratio, T* o, size_t n) {
    const size_t i = gid();
    st3(o, n, i, refract(ld3(v, n, i), ld3(nn, n, i), ratio[i]));
}
template <typename T> __global__ void k_q8(const T* v, uint8_t* o, size_t) { const size_t i = gid(); o[i] = q8(v[i]); }
template <typename T> __global__ void k_div_dim(const T* x, uint32_t W, double r, T* o, size_t) { const size_t i = gid(); o[i] = div_dim(x[i], W, r); }
template <typename T>
__global__ void k_rng(const uint32_t* sid, const uint32_t* pix, const uint32_t* k, const uint32_t* stream, uint32_t k0,
                      uint32_t k1, uint32_t* r, T* ua, T* ub, size_t n) {
    const size_t i = gid();
    const U4 b = rng<T>(sid[i], pix[i], k[i], stream[i], k0, k1);
    r[i] = b.a; r[n + i] = b.b; r[2 * n + i] = b.c; r[3 * n + i] = b.d;
    ua[i] = u01a(b, T(0)); ub[i] = u01b(b, T(0));
}
__global__ void k_philox(const uint32_t* c, const uint32_t* key, uint32_t* r, size_t n) {
    const size_t i = gid();
    const U4 b = philox(c[i], c[n + i], c[2 * n + i], c[3 * n + i], key[i], key[n + i]);
    r[i] = b.a; r[n + i] = b.b; r[2 * n + i] = b.c; r[3 * n + i] = b.d;
}
__global__ void k_philox2(const uint32_t* c, const uint32_t* key, uint32_t* r, size_t n) {
    const size_t i = gid();
    const U4 b = philox2(c[i], c[n + i], key[i]);
    r[i] = b.a; r[n + i] = b.b;
}
// hit_update folded over the lane's first cnt[i] (<= 8) candidates, slot-major: hb[c * n + i].
constexpr uint32_t kHitSlots = 8;
template <typename T, bool root2, bool SCALAR>
__global__ void k_hit(const T* hb, const T* disc, const uint32_t* idx, const uint32_t* cnt, const T* a, T* ot, int32_t* oi,
                      size_t n) {
    const size_t i = gid();
    const T aa = a[i];
    const T inv_a = SCALAR ? T(0) : T(1.0) / aa;   // nearest_hit
    const uint32_t m = cnt[i];
    HitBest<T> bh;
    for (uint32_t c = 0; c < kHitSlots; ++c)
        if (c < m) hit_update<T, root2, SCALAR>(hb[c * n + i], disc[c * n + i], idx[c * n + i], aa, inv_a, bh);
    ot[i] = bh.bt(); oi[i] = bh.bi();
}

// sqrt over consecutive fp32 bit patterns, compared on the device with (float)sqrt((double)x) (the f64 sqrt is
// correctly rounded and 53 >= 2 * 24 + 2, so the double rounding is harmless).  A wave holds 64 consecutive
// patterns.  mode 0: sqrt_len; mode 1: sqrt_len with lane 7 of every odd wave replaced by a tiny positive
// argument (below 2^-96), so the other 63 lanes take the ballot's library path; mode 2: sqrt_nd (the caller
// keeps the range inside its contract).
constexpr uint32_t kFirst = 16;
__global__ void k_sqrt_sweep(uint32_t start, uint32_t iters, int mode, unsigned long long* count, uint32_t* first) {
#pragma unroll 1
    for (uint32_t it = 0; it < iters; ++it) {
        const uint32_t off = (it * gridDim.x + blockIdx.x) * kBlock + threadIdx.x;
        uint32_t bits = start + off;
        if (mode == 1 && (off & 127u) == 71u) bits = (bits >> 5) | 1u;   // in (0, 2^-96): below 0x08000000
        const float x = __uint_as_float(bits);
        const float got = mode == 2 ? sqrt_nd(x) : sqrt_len(x);
        const float want = (float)sqrt((double)x);
        const bool same = (got != got && want != want) || __float_as_uint(got) == __float_as_uint(want);
        if (!same) {
            const unsigned long long slot = atomicAdd(count, 1ull);
            if (slot < kFirst) first[slot] = bits;
        }
    }
}

// ---- the ray probe: the product's sweeps on the caller's rays ----
// nearest_hit and camera_sweep read their tables through cold_args<T>(), the start of the kernarg segment, so the
// probe kernels take KParams<T> by value as their first argument, as the product's kernels do.  Lane i holds ray i
// and writes idx[i] / t[i] only when active[i] is set: an inactive lane's outputs stay as the caller left them.
// General probe: inactive lanes do not enter nearest_hit (its ballots and box masks see the active lanes only).
// Camera probe: the whole wave calls camera_sweep with v = active (a wave without any active lane is skipped:
// camera_sweep takes its cone's axis from the first valid lane).
template <typename T, bool ROOT2, bool SC, bool MEGA>
__global__ void __launch_bounds__(kBlock) k_probe_general(KParams<T> p, const T* o, const T* d, const uint8_t* active,
                                                          int32_t* idx, T* t, size_t n) {
    const size_t i = gid();
    if (active[i]) {
        const V3<T> ro = ld3(o, n, i), rd = ld3(d, n, i);
        T th;
        const int h = nearest_hit<T, ROOT2, SC, MEGA>(ro, rd, th);
        idx[i] = h;
        t[i] = th;
    }
}
template <typename T, bool ROOT2, bool SC, bool MEGA>
__global__ void __launch_bounds__(kBlock) k_probe_camera(KParams<T> p, const T* d, const uint8_t* active, int32_t* idx,
                                                         T* t, size_t n) {
    const size_t i = gid();
    const bool v = active[i] != 0;
    if (__ballot(v) == 0ull) return;   // wave-uniform
    const V3<T> rd = ld3(d, n, i);
    T th;
    const int h = camera_sweep<T, ROOT2, SC, MEGA>(v, rd, th);
    if (v) {
        idx[i] = h;
        t[i] = th;
    }
}

// The device tables of one scene image at precision T and the kernel arguments over them, both by the product's own
// steps (rt_host.hpp): upload_scene and scene_params for the scene half (a table the scene does not have stays
// NULL, unread), cam_table_params and launch_cam_table for the camera tables.  The frame half of p stays zero.
template <typename T> struct ProbeScene {
    DeviceScene<T> d;
    DeviceBuffer ridx, mtiers;
    KParams<T> p;
    int setup(const SceneImage& im, bool filter_off) {
        int rc = upload_scene(d, im.tables<T>());
        if (rc == RT_OK) rc = upload(ridx, im.ridx);
        if (rc == RT_OK) rc = upload(mtiers, im.mtiers);
        memset(&p, 0, sizeof(p));
        scene_params(d, im.n, ridx, mtiers, filter_off, p);
        return rc;
    }
    // The camera tables of centre c, built on the null stream; returns once they are there.
    int cam_tables(const SceneImage& im, const T* c, bool scalar, bool filter_off) {
        for (int a = 0; a < 3; ++a) p.center[a] = c[a];
        cam_table_params(d, im.n, p);
        const int rc = launch_cam_table(d, im.n, ridx, p.center, scalar, filter_off, 0);
        if (rc != RT_OK) return rc;
        return hipDeviceSynchronize() == hipSuccess ? RT_OK : RT_ERR_HIP;
    }
};

// mode 0: the live path <T, false, false>, 1: root2 <T, true, false>, 2: scalar <T, false, true>; MEGA as the
// launchers pick it (n_mg > 0).  centre == nullptr: the general probe.  Returns 0, a HIP error of the probe's own
// calls, or the product's error code (RT_ERR_HIP) where its steps failed.
template <typename T>
int probe(const rt_scene* s, int mode, int filter_off, const T* centre, const T* o, const T* d, const uint8_t* active,
          int32_t* idx, T* t, size_t n) {
    if (!s || mode < 0 || mode > 2 || n % kBlock != 0 || n > (1u << 24)) return -1;
    const SceneImage im = build_scene_image(s);
    ProbeScene<T> ps;
    int rc = ps.setup(im, filter_off != 0);
    if (rc == RT_OK && centre) rc = ps.cam_tables(im, centre, mode == 2, filter_off != 0);
    if (rc != RT_OK) return rc;
    const KParams<T>& p = ps.p;
    Dev dv;
    const T* dor = centre ? nullptr : dv.in(o, 3 * n);
    const T* dd = dv.in(d, 3 * n);
    const uint8_t* da = dv.in(active, n);
    int32_t* di = dv.in(idx, n);
    T* dt = dv.in(t, n);
    if (dv.ok() && n) {
        const dim3 g((unsigned)(n / kBlock)), b(kBlock);
        const bool mega = im.n.n_mg > 0;
#define PROBE_LAUNCH(R2, SC, MG)                                                                            \
    do {                                                                                                    \
        if (centre) hipLaunchKernelGGL((k_probe_camera<T, R2, SC, MG>), g, b, 0, 0, p, dd, da, di, dt, n);  \
        else hipLaunchKernelGGL((k_probe_general<T, R2, SC, MG>), g, b, 0, 0, p, dor, dd, da, di, dt, n);   \
    } while (0)
        if (mode == 0) { if (mega) PROBE_LAUNCH(false, false, true); else PROBE_LAUNCH(false, false, false); }
        else if (mode == 1) { if (mega) PROBE_LAUNCH(true, false, true); else PROBE_LAUNCH(true, false, false); }
        else { if (mega) PROBE_LAUNCH(false, true, true); else PROBE_LAUNCH(false, true, false); }
#undef PROBE_LAUNCH
        dv.sync();
    }
    dv.back(idx, di, n);
    dv.back(t, dt, n);
    return (int)dv.err;
}

// ---- the next-ray probe: the product's next_ray<T, SCALAR> and nothing else ----
// Lane i: role 0 idle (the lane does not enter next_ray; its o, d, c stay as the caller left them), 1 camera
// (cam = true: colx, rowy, pix, sid), 2 scatter (cam = false: o, d, c, hit_i, hit_t, k, pix, sid).  o, d, c are read
// and written in place.  next_ray reads the camera, the key and the scene's centre and material tables through
// cold_args<T>(), so the kernel takes KParams<T> by value as its first argument.
template <typename T, bool SCALAR>
__global__ void __launch_bounds__(kBlock) k_probe_next_ray(KParams<T> p, const uint8_t* role, const uint32_t* colx,
                                                           const uint32_t* rowy, const uint32_t* pix, const uint32_t* sid,
                                                           const uint32_t* k, const int32_t* hit_i, const T* hit_t, T* o,
                                                           T* d, T* c, size_t n) {
    const size_t i = gid();
    const uint32_t r = role[i];
    if (r != 0u) {
        V3<T> ro = ld3(o, n, i), rd = ld3(d, n, i), rc = ld3(c, n, i);
        next_ray<T, SCALAR>(r == 1u, colx[i], rowy[i], pix[i], sid[i], k[i], hit_i[i], hit_t[i], ro, rd, rc);
        st3(o, n, i, ro);
        st3(d, n, i, rd);
        st3(c, n, i, rc);
    }
}

// The kernel arguments by the product's own host steps: ProbeScene::setup for the scene half (the centre and
// material tables of build_scene_image), frame_params for the frame half (the camera in T, rW / rH, the pinhole
// flag, the RNG key with the fp32 fold).  mode 0: <T, false> (the packed modes), 1: <T, true> (scalar).  A scatter
// lane's hit index must be a sphere of the scene (-1 otherwise: the kernel gathers its tables with it).
template <typename T>
int probe_next_ray(const rt_scene* s, const rt_camera* cam, uint64_t seed, int mode, const uint8_t* role,
                   const uint32_t* colx, const uint32_t* rowy, const uint32_t* pix, const uint32_t* sid, const uint32_t* k,
                   const int32_t* hit_i, const T* hit_t, T* o, T* d, T* c, size_t n) {
    if (!s || !cam || mode < 0 || mode > 1 || n % kBlock != 0 || n > (1u << 24)) return -1;
    if (cam->image_width == 0 || cam->image_height == 0 || s->n_spheres == 0) return -1;
    for (size_t i = 0; i < n; ++i) {
        if (role[i] > 2u) return -1;
        if (role[i] == 2u && (hit_i[i] < 0 || (uint32_t)hit_i[i] >= s->n_spheres)) return -1;
    }
    const SceneImage im = build_scene_image(s);
    ProbeScene<T> ps;
    const int rc = ps.setup(im, false);
    if (rc != RT_OK) return rc;
    FrameArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.cam = cam;
    fa.depth = 50u;
    fa.spp = 16u;
    fa.seed = seed;
    fa.flags = mode == 1 ? RT_FLAG_MODE_SCALAR : 0u;
    fa.rg.row_count = cam->image_height; fa.rg.row_step = 1u; fa.rg.col_count = cam->image_width;
    frame_params(fa, ps.p);
    const KParams<T>& p = ps.p;
    Dev dv;
    const uint8_t* dr = dv.in(role, n);
    const uint32_t* dx = dv.in(colx, n);
    const uint32_t* dy = dv.in(rowy, n);
    const uint32_t* dp = dv.in(pix, n);
    const uint32_t* ds = dv.in(sid, n);
    const uint32_t* dk = dv.in(k, n);
    const int32_t* dh = dv.in(hit_i, n);
    const T* dt = dv.in(hit_t, n);
    T* dor = dv.in(o, 3 * n);
    T* dd = dv.in(d, 3 * n);
    T* dc = dv.in(c, 3 * n);
    if (dv.ok() && n) {
        const dim3 g((unsigned)(n / kBlock)), b(kBlock);
        if (mode == 0) hipLaunchKernelGGL((k_probe_next_ray<T, false>), g, b, 0, 0, p, dr, dx, dy, dp, ds, dk, dh, dt, dor, dd, dc, n);
        else hipLaunchKernelGGL((k_probe_next_ray<T, true>), g, b, 0, 0, p, dr, dx, dy, dp, ds, dk, dh, dt, dor, dd, dc, n);
        dv.sync();
    }
    dv.back(o, dor, 3 * n);
    dv.back(d, dd, 3 * n);
    dv.back(c, dc, 3 * n);
    return (int)dv.err;
}

template <typename F> int run(size_t n, F&& body) {
    if (n % kBlock != 0) return -1;
    Dev d;
    body(d, dim3((unsigned)(n / kBlock)), dim3(kBlock));
    return (int)d.err;
}

}  // namespace

#define LAUNCH(kern, ...) do { if (d.ok() && n) { hipLaunchKernelGGL(kern, g, b, 0, 0, __VA_ARGS__); d.sync(); } } while (0)

#define DEVUNIT_FOR(T, sfx)                                                                                            \
    int du_unit_##sfx(const T* v, T* out, size_t n) {                                                                  \
        return run(n, [&](Dev& d, dim3 g, dim3 b) {                                                                    \
            const T* dv = d.in(v, 3 * n); T* o = d.out<T>(3 * n);                                                      \
            LAUNCH(k_unit<T>, dv, o, n); d.back(out, o, 3 * n); });                                                    \
    }                                                                                                                  \
    int du_dvs_##sfx(const T* v, const T* s, T* out, size_t n) {                                                       \
        return run(n, [&](Dev& d, dim3 g, dim3 b) {                                                                    \
            const T* dv = d.in(v, 3 * n); const T* ds = d.in(s, n); T* o = d.out<T>(3 * n);                            \
            LAUNCH(k_dvs<T>, dv, ds, o, n); d.back(out, o, 3 * n); });                                                 \
    }                                                                                                                  \
    int du_sqrt_nd_##sfx(const T* x, T* out, size_t n) {                                                               \
        return run(n, [&](Dev& d, dim3 g, dim3 b) {                                                                    \
            const T* dx = d.in(x, n); T* o = d.out<T>(n);                                                              \
            LAUNCH(k_sqrt_nd<T>, dx, o, n); d.back(out, o, n); });                                                     \
    }                                                                                                                  \
    int du_sqrt_len_##sfx(const T* x, T* out, size_t n) {                                                              \
        return run(n, [&](Dev& d, dim3 g, dim3 b) {                                                                    \
            const T* dx = d.in(x, n); T* o = d.out<T>(n);                                                              \
            LAUNCH(k_sqrt_len<T>, dx, o, n); d.back(out, o, n); });                                                    \
    }                                                                                                                  \
    int du_sincos2pi_##sfx(const T* u, T* s, T* c, size_t n) {                                                         \
        return run(n, [&](Dev& d, dim3 g, dim3 b) {                                                                    \
            const T* du = d.in(u, n); T* ds = d.out<T>(n); T* dc = d.out<T>(n);                                        \
            LAUNCH(k_sincos<T>, du, ds, dc, n); d.back(s, ds, n); d.back(c, dc, n); });                                \
    }                                                                                                                  \
    int du_unit_vec_##sfx(const T* u1, const T* u2, T* out, size_t n) {                                                \
        return run(n, [&](Dev& d, dim3 g, dim3 b) {                                                                    \
            const T* d1 = d.in(u1, n); const T* d2 = d.in(u2, n); T* o = d.out<T>(3 * n);                              \
            LAUNCH(k_unit_vec<T>, d1, d2, o, n); d.back(out, o, 3 * n); });                                            \
    }                                                                                                                  \
    int du_refract_##sfx(const T* v, const T* nn, const T* ratio, T* out, size_t n) {                                  \
        return run(n, [&](Dev& d, dim3 g, dim3 b) {                                                                    \
            const T* dv = d.in(v, 3 * n); const T* dn = d.in(nn, 3 * n); const T* dr = d.in(ratio, n);                 \
            T* o = d.out<T>(3 * n);                                                                                    \
            LAUNCH(k_refract<T>, dv, dn, dr, o, n); d.back(out, o, 3 * n); });                                         \
    }                                                                                                                  \
    int du_q8_##sfx(const T* v, uint8_t* out, size_t n) {                                                              \
        return run(n, [&](Dev& d, dim3 g, dim3 b) {                                                                    \
            const T* dv = d.in(v, n); uint8_t* o = d.out<uint8_t>(n);                                                  \
            LAUNCH(k_q8<T>, dv, o, n); d.back(out, o, n); });                                                          \
    }                                                                                                                  \
    int du_div_dim_##sfx(const T* x, uint32_t W, double r, T* out, size_t n) {                                         \
        return run(n, [&](Dev& d, dim3 g, dim3 b) {                                                                    \
            const T* dx = d.in(x, n); T* o = d.out<T>(n);                                                              \
            LAUNCH(k_div_dim<T>, dx, W, r, o, n); d.back(out, o, n); });                                               \
    }                                                                                                                  \
    int du_rng_##sfx(const uint32_t* sid, const uint32_t* pix, const uint32_t* k, const uint32_t* stream, uint32_t k0, \
                     uint32_t k1, uint32_t* r, T* ua, T* ub, size_t n) {                                               \
        return run(n, [&](Dev& d, dim3 g, dim3 b) {                                                                    \
            const uint32_t* d0 = d.in(sid, n); const uint32_t* d1 = d.in(pix, n); const uint32_t* d2 = d.in(k, n);     \
            const uint32_t* d3 = d.in(stream, n);                                                                      \
            uint32_t* dr = d.out<uint32_t>(4 * n); T* da = d.out<T>(n); T* db = d.out<T>(n);                           \
            LAUNCH(k_rng<T>, d0, d1, d2, d3, k0, k1, dr, da, db, n);                                                   \
            d.back(r, dr, 4 * n); d.back(ua, da, n); d.back(ub, db, n); });                                            \
    }                                                                                                                  \
    /* mode 0: <T,false,false>, 1: <T,true,false>, 2: <T,*,true> (the scalar mode ignores root2) */                    \
    int du_hit_##sfx(const T* hb, const T* disc, const uint32_t* idx, const uint32_t* cnt, const T* a, int mode,       \
                     T* t_out, int32_t* i_out, size_t n) {                                                             \
        if (mode < 0 || mode > 2) return -1;                                                                           \
        return run(n, [&](Dev& d, dim3 g, dim3 b) {                                                                    \
            const T* dh = d.in(hb, kHitSlots * n); const T* dd = d.in(disc, kHitSlots * n);                                  \
            const uint32_t* di = d.in(idx, kHitSlots * n); const uint32_t* dc = d.in(cnt, n); const T* da = d.in(a, n);   \
            T* ot = d.out<T>(n); int32_t* oi = d.out<int32_t>(n);                                                      \
            if (mode == 0) LAUNCH((k_hit<T, false, false>), dh, dd, di, dc, da, ot, oi, n);                            \
            else if (mode == 1) LAUNCH((k_hit<T, true, false>), dh, dd, di, dc, da, ot, oi, n);                        \
            else LAUNCH((k_hit<T, false, true>), dh, dd, di, dc, da, ot, oi, n);                                       \
            d.back(t_out, ot, n); d.back(i_out, oi, n); });                                                            \
    }

extern "C" {

DEVUNIT_FOR(float, f32)
DEVUNIT_FOR(double, f64)

int du_philox4x32_10(const uint32_t* ctr, const uint32_t* key, uint32_t* out, size_t n) {
    return run(n, [&](Dev& d, dim3 g, dim3 b) {
        const uint32_t* dc = d.in(ctr, 4 * n); const uint32_t* dk = d.in(key, 2 * n); uint32_t* o = d.out<uint32_t>(4 * n);
        LAUNCH(k_philox, dc, dk, o, n); d.back(out, o, 4 * n); });
}
int du_philox2x32_10(const uint32_t* ctr, const uint32_t* key, uint32_t* out, size_t n) {
    return run(n, [&](Dev& d, dim3 g, dim3 b) {
        const uint32_t* dc = d.in(ctr, 2 * n); const uint32_t* dk = d.in(key, n); uint32_t* o = d.out<uint32_t>(2 * n);
        LAUNCH(k_philox2, dc, dk, o, n); d.back(out, o, 2 * n); });
}
// The host's fp32 key fold (rt_launch.hpp frame_params): seed lo ^ fmix32(seed hi), with rt_device.hpp's fmix32.
uint32_t du_fold_key_f32(uint64_t seed) { return (uint32_t)seed ^ fmix32((uint32_t)(seed >> 32)); }

// sqrt over the `count` bit patterns from `start` (wrapping mod 2^32); count a multiple of 256, and of 2^22 when
// above 2^22.  *mismatches: how many differ from (float)sqrt((double)x); first[16]: the first offenders.
int du_sqrt_sweep_f32(uint32_t start, uint64_t count, int mode, uint64_t* mismatches, uint32_t* first) {
    constexpr uint64_t kGrid = 1u << 14;
    if (count == 0 || count > (1ull << 32) || count % kBlock != 0 || mode < 0 || mode > 2) return -1;
    const uint64_t blocks = count / kBlock;
    if (blocks > kGrid && blocks % kGrid != 0) return -1;
    const unsigned grid = (unsigned)(blocks > kGrid ? kGrid : blocks);
    const uint32_t iters = (uint32_t)(blocks / grid);
    Dev d;
    unsigned long long zero = 0;
    uint32_t none[kFirst] = {0};
    unsigned long long* dc = d.in(&zero, 1);
    uint32_t* df = d.in(none, kFirst);
    if (d.ok()) { hipLaunchKernelGGL(k_sqrt_sweep, dim3(grid), dim3(kBlock), 0, 0, start, iters, mode, dc, df); d.sync(); }
    d.back(&zero, dc, 1);
    d.back(first, df, kFirst);
    *mismatches = zero;
    return (int)d.err;
}

// The ray probe (above).  o, d: n rays, component-major; active: one byte per lane; idx, t: in and out (a lane that
// is not active keeps the caller's values); idx -1 and t +inf: no hit.  The camera probe's rays all start at centre.
int du_probe_general_f32(const rt_scene* s, int mode, int filter_off, const float* o, const float* d,
                         const uint8_t* active, int32_t* idx, float* t, size_t n) {
    return o ? probe<float>(s, mode, filter_off, nullptr, o, d, active, idx, t, n) : -1;
}
int du_probe_general_f64(const rt_scene* s, int mode, int filter_off, const double* o, const double* d,
                         const uint8_t* active, int32_t* idx, double* t, size_t n) {
    return o ? probe<double>(s, mode, filter_off, nullptr, o, d, active, idx, t, n) : -1;
}
int du_probe_camera_f32(const rt_scene* s, int mode, int filter_off, const float* centre, const float* d,
                        const uint8_t* active, int32_t* idx, float* t, size_t n) {
    return centre ? probe<float>(s, mode, filter_off, centre, nullptr, d, active, idx, t, n) : -1;
}
int du_probe_camera_f64(const rt_scene* s, int mode, int filter_off, const double* centre, const double* d,
                        const uint8_t* active, int32_t* idx, double* t, size_t n) {
    return centre ? probe<double>(s, mode, filter_off, centre, nullptr, d, active, idx, t, n) : -1;
}
// The next-ray probe (above): role, colx, rowy, pix, sid, k, hit_i, hit_t: n lanes; o, d, c: [3, n] component-major, in
// and out (an idle lane keeps the caller's values).
int du_next_ray_f32(const rt_scene* s, const rt_camera* cam, uint64_t seed, int mode, const uint8_t* role,
                    const uint32_t* colx, const uint32_t* rowy, const uint32_t* pix, const uint32_t* sid, const uint32_t* k,
                    const int32_t* hit_i, const float* hit_t, float* o, float* d, float* c, size_t n) {
    return probe_next_ray<float>(s, cam, seed, mode, role, colx, rowy, pix, sid, k, hit_i, hit_t, o, d, c, n);
}
int du_next_ray_f64(const rt_scene* s, const rt_camera* cam, uint64_t seed, int mode, const uint8_t* role,
                    const uint32_t* colx, const uint32_t* rowy, const uint32_t* pix, const uint32_t* sid, const uint32_t* k,
                    const int32_t* hit_i, const double* hit_t, double* o, double* d, double* c, size_t n) {
    return probe_next_ray<double>(s, cam, seed, mode, role, colx, rowy, pix, sid, k, hit_i, hit_t, o, d, c, n);
}
// What build_scene_image makes of the scene, for the case generators (host only, no GPU): counts[8] = {n_xg, n_xs,
// n_top, n_mg, n_gg, n_supc, n_cslots, 0}, and the first min(cap, n_cslots) words of the slot -> scene index table
// (0xFFFFFFFF: a dummy slot; the always-exact slots first, then cluster k at 4 n_xg + 16 k).
int du_scene_layout(const rt_scene* s, uint32_t* counts, uint32_t* ridx, size_t cap) {
    if (!s || !counts) return -1;
    const SceneImage im = build_scene_image(s);
    const uint32_t c[8] = {im.n.n_xg, im.n.n_xs, im.n.n_top, im.n.n_mg, im.n.n_gg, im.n.n_supc, im.n.n_cslots, 0u};
    memcpy(counts, c, sizeof(c));
    for (size_t i = 0; ridx && i < cap && i < im.ridx.size(); ++i) ridx[i] = im.ridx[i];
    return 0;
}

}  // extern "C"
