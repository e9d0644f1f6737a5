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
// rt_sweep.hpp (general sweep), rt_camera.hpp (primary rays, scatter), rt_finish.hpp (the record view, replay + reduction),
// rt_trace.hpp + rt_trace_body.hpp (the persistent kernel), rt_guides.hpp (guide buffers: first hits only),
// rt_query.hpp (ray queries: the closest hit of the caller's rays, and occlusion before a t_max),
// rt_step.hpp (path steps: the material stage alone, and closest hit + scatter in one kernel), rt_list.hpp (ray lists:
// the step over the live rays only, and the stable compaction that leaves the next list), rt_rays.hpp (full paths for the caller's
// primary rays); rt_projection.hpp (host only: the rays of camera models the reference lacks);
// host only, without HIP: rt_layout.hpp (the scene image: every device table of a scene, build_scene_image),
// rt_split_plan.hpp (the sample-parallel plan), rt_progressive_plan.hpp (a progressive session's record buffer,
// sample windows and count classes);
// and the host code, each header knowing only the ones before it: rt_host.hpp (errors, owned device and pinned
// memory, a scene's device tables and their half of the kernel arguments: scene_params, cam_table_params,
// launch_cam_table; it knows no context, and the test-only device library builds its arguments with it),
// rt_launch.hpp (what a context's launches share, kernel selection and kernel_id, the launch steps frame_params,
// ensure_cam_tables, frame_setup, plan_grid, and the launchers launch_plain, launch_split, launch_window,
// launch_guides, launch_query, launch_occlusion, launch_scatter, launch_step, launch_rays), rt_session.hpp (a progressive session: its state, launch_items and launch_classes
// for per-pixel counts, extend_uniform, run_map, snapshot_run and the steps of refine_step).  This file holds the
// C ABI: rt_context, the entry points (their argument checks, then one call) and the small device helpers.
#include "rt_session.hpp"
#include "rt_projection.hpp"

#include <chrono>

// ============================== host side ==============================
using namespace rt;

// A context: what its launches share (rt_launch.hpp) and its progressive session (rt_session.hpp).
struct rt_context : LaunchContext {
    Session prog;
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

// A context without a scene: no table, every count zero.
static void free_scene(rt_context* c) {
    c->d32.reset();
    c->d64.reset();
    c->ridx.reset();
    c->mtiers.reset();
    c->n = SceneCounts{};
    c->has_scene = false;
}

// Everything a context made, and the context: what init_context did not get to is still NULL.
static void free_context(rt_context* c) {
    free_scene(c);
    c->segs.reset(); c->err.reset(); c->counter.reset(); c->scratch.reset(); c->records.reset(); c->rayskip.reset();
    c->ballots.reset(); c->tiles.reset();
    if (c->ev_first) (void)hipEventDestroy(c->ev_first);
    if (c->ev_last) (void)hipEventDestroy(c->ev_last);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

static int init_context(rt_context* c, int device) {
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
    return RT_OK;
}

extern "C" int rt_context_create(int device, rt_context** out) {
    if (!out) return fail(RT_ERR_INVALID, "rt_context_create: out is NULL");
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(RT_ERR_INVALID, "rt_context_create: no such device");
    HIPCHK(hipSetDevice(device));
    rt_context* c = new rt_context();
    const int rc = init_context(c, device);
    if (rc != RT_OK) {
        free_context(c);   // the error text stays init_context's
        return rc;
    }
    *out = c;
    return RT_OK;
}

extern "C" int rt_context_destroy(rt_context* c) {
    if (!c) return RT_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->prog.open) (void)rt_progressive_end(c);
    free_context(c);
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
        const uint32_t P = prog_positions(spp);
        const uint64_t rec_bytes = n_pix * paths_sbytes(P, f32 ? 4u : 8u, paths_wide(P, max_bounces));
        if (split_mode == 0) {
            uint64_t n_items = 0;
            const int prc = split_plan(n_pix, spp, split_waves(c, f32), &S, &n_items);
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
    rc = with_precision(f32, [&](auto t) {
        using T = decltype(t);
        return split ? launch_split<T>(c, a, S, nsub, st) : launch_plain<T>(c, a, st);
    });
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
    rc = with_precision((flags & RT_FLAG_F32) != 0, [&](auto t) {
        return launch_guides<decltype(t)>(c, a, (float*)d_albedo, (float*)d_normal, (float*)d_depth, (float*)d_coverage, st);
    });
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
    rc = with_precision((flags & RT_FLAG_F32) != 0, [&](auto t) { return launch_query<decltype(t)>(c, a, st); });
    if (rc != RT_OK) return rc;
    return end_launch(c, st, n_rays, 0u);   // samples: the valid rays, counted on the device (kQuerySlot)
}

extern "C" int rt_query_occluded_async(rt_context* c, uint64_t n_rays, const void* d_origins, const double* origin,
                                       const void* d_directions, const void* d_t_max, double t_max, uint32_t flags,
                                       void* d_occluded, void* stream) {
    const std::string who = "rt_query_occluded_async";
    if (!c || !d_directions || !d_occluded) return fail(RT_ERR_INVALID, who + ": NULL argument (ctx, d_directions or d_occluded)");
    if ((d_origins != nullptr) == (origin != nullptr))
        return fail(RT_ERR_INVALID, who + ": exactly one of d_origins (per ray) and origin (shared) must be given");
    if (!d_t_max && t_max != t_max) return fail(RT_ERR_INVALID, who + ": d_t_max is NULL and t_max is NaN");
    if (flags & ~RT_FLAG_ALL) return fail(RT_ERR_INVALID, who + ": unknown flag bits");
    if (flags & ~(RT_FLAG_F32 | RT_FLAG_ROOT2))
        return fail(RT_ERR_UNSUPPORTED, who + ": the live path's hit rule only (RT_FLAG_F32, RT_FLAG_ROOT2; no RT_FLAG_MODE_*)");
    if (n_rays > 0x7FFFFFFFull) return fail(RT_ERR_UNSUPPORTED, who + ": too many rays in one call");
    if (!c->has_scene) return fail(RT_ERR_INVALID, who + ": no scene set (rt_context_set_scene first)");
    if (n_rays == 0) return RT_OK;
    const OcclusionArgs a{n_rays, d_origins, origin, d_directions, d_t_max, t_max, flags, d_occluded};
    hipStream_t st = (hipStream_t)stream;
    int rc = begin_launch(c, st);
    if (rc != RT_OK) return rc;
    rc = with_precision((flags & RT_FLAG_F32) != 0, [&](auto t) { return launch_occlusion<decltype(t)>(c, a, st); });
    if (rc != RT_OK) return rc;
    return end_launch(c, st, n_rays, 0u);   // samples: the valid rays, counted on the device (kQuerySlot)
}

// The checks rt_scatter_async and rt_path_step_async share, after their own of the pointers.
static int check_step(const rt_context* c, const std::string& who, uint64_t n_rays, uint32_t bounce, uint32_t flags) {
    if (flags & ~RT_FLAG_ALL) return fail(RT_ERR_INVALID, who + ": unknown flag bits");
    if (flags & ~(RT_FLAG_F32 | RT_FLAG_ROOT2))
        return fail(RT_ERR_UNSUPPORTED, who + ": the live path only (RT_FLAG_F32, RT_FLAG_ROOT2; no RT_FLAG_MODE_*)");
    if ((flags & RT_FLAG_F32) && bounce > RT_MAX_BOUNCES_F32)   // rng<float>'s counter (rt_device.hpp)
        return fail(RT_ERR_UNSUPPORTED, who + ": fp32 with bounce > RT_MAX_BOUNCES_F32 (3839)");
    if (n_rays > 0x7FFFFFFFull) return fail(RT_ERR_UNSUPPORTED, who + ": too many rays in one call");
    if (!c->has_scene) return fail(RT_ERR_INVALID, who + ": no scene set (rt_context_set_scene first)");
    return RT_OK;
}

extern "C" int rt_scatter_async(rt_context* c, uint64_t n_rays, const void* d_origins, const double* origin,
                                const void* d_directions, const void* d_index, const void* d_t, const void* d_pixel,
                                const void* d_sample, uint32_t bounce, uint64_t seed, uint32_t flags, void* d_colour,
                                void* d_out_origins, void* d_out_directions, void* stream) {
    const std::string who = "rt_scatter_async";
    if (!c || !d_directions || !d_index || !d_t || !d_pixel || !d_sample)
        return fail(RT_ERR_INVALID, who + ": NULL argument (ctx, d_directions, d_index, d_t, d_pixel or d_sample)");
    if (!d_out_origins && !d_out_directions) return fail(RT_ERR_INVALID, who + ": both output arrays are NULL");
    if ((d_origins != nullptr) == (origin != nullptr))
        return fail(RT_ERR_INVALID, who + ": exactly one of d_origins (per ray) and origin (shared) must be given");
    int rc = check_step(c, who, n_rays, bounce, flags);
    if (rc != RT_OK) return rc;
    if (n_rays == 0) return RT_OK;
    const ScatterArgs a{n_rays, d_origins, origin, d_directions, d_index, d_t, d_pixel, d_sample, bounce, seed, flags,
                        d_colour, d_out_origins, d_out_directions};
    hipStream_t st = (hipStream_t)stream;
    if ((rc = begin_launch(c, st)) != RT_OK) return rc;
    rc = with_precision((flags & RT_FLAG_F32) != 0, [&](auto t) { return launch_scatter<decltype(t)>(c, a, st); });
    if (rc != RT_OK) return rc;
    return end_launch(c, st, n_rays, 0u);   // samples: the scattered rays, counted on the device (kQuerySlot)
}

extern "C" int rt_path_step_async(rt_context* c, uint64_t n_rays, void* d_origins, void* d_directions, void* d_colour,
                                  const void* d_pixel, const void* d_sample, uint32_t bounce, uint64_t seed,
                                  uint32_t flags, void* d_status, void* d_index, void* d_t, void* d_normal, void* d_front,
                                  void* stream) {
    const std::string who = "rt_path_step_async";
    if (!c || !d_origins || !d_directions || !d_pixel || !d_sample)
        return fail(RT_ERR_INVALID, who + ": NULL argument (ctx, d_origins, d_directions, d_pixel or d_sample)");
    int rc = check_step(c, who, n_rays, bounce, flags);
    if (rc != RT_OK) return rc;
    if (n_rays == 0) return RT_OK;
    const StepArgs a{n_rays, d_origins, d_directions, d_colour, d_pixel, d_sample, bounce, seed, flags,
                     d_status, d_index, d_t, d_normal, d_front};
    hipStream_t st = (hipStream_t)stream;
    if ((rc = begin_launch(c, st)) != RT_OK) return rc;
    rc = with_precision((flags & RT_FLAG_F32) != 0, [&](auto t) { return launch_step<decltype(t)>(c, a, st); });
    if (rc != RT_OK) return rc;
    return end_launch(c, st, n_rays, 0u);   // samples: the valid rays, counted on the device (kQuerySlot)
}

// The list checks rt_path_step_list_async and rt_ray_list_compact_async share: the output pair and the ping-pong rule.
static int check_lists(const std::string& who, const ListArgs& l) {
    if ((l.list_out != nullptr) != (l.count_out != nullptr))
        return fail(RT_ERR_INVALID, who + ": d_list_out and d_count_out must be given together (or both NULL)");
    if (l.list_out && l.list_out == l.list_in)
        return fail(RT_ERR_INVALID, who + ": d_list_out is d_list_in (ping-pong two lists)");
    if (l.count_out && l.count_out == l.count_in)
        return fail(RT_ERR_INVALID, who + ": d_count_out is d_count_in (ping-pong two counts)");
    return RT_OK;
}

extern "C" int rt_path_step_list_async(rt_context* c, uint64_t n_rays, const void* d_list_in, const void* d_count_in,
                                       void* d_origins, void* d_directions, void* d_colour, const void* d_pixel,
                                       const void* d_sample, uint32_t bounce, uint64_t seed, uint32_t flags,
                                       void* d_status, void* d_index, void* d_t, void* d_normal, void* d_front,
                                       void* d_list_out, void* d_count_out, void* stream) {
    const std::string who = "rt_path_step_list_async";
    if (!c || !d_origins || !d_directions || !d_pixel || !d_sample)
        return fail(RT_ERR_INVALID, who + ": NULL argument (ctx, d_origins, d_directions, d_pixel or d_sample)");
    const ListArgs l{d_list_in, d_count_in, d_list_out, d_count_out, nullptr};
    int rc = check_lists(who, l);
    if (rc != RT_OK) return rc;
    if ((rc = check_step(c, who, n_rays, bounce, flags)) != RT_OK) return rc;
    if (n_rays == 0) return RT_OK;
    const StepArgs a{n_rays, d_origins, d_directions, d_colour, d_pixel, d_sample, bounce, seed, flags,
                     d_status, d_index, d_t, d_normal, d_front};
    hipStream_t st = (hipStream_t)stream;
    if ((rc = begin_launch(c, st)) != RT_OK) return rc;
    rc = with_precision((flags & RT_FLAG_F32) != 0, [&](auto t) { return launch_step_list<decltype(t)>(c, a, l, st); });
    if (rc != RT_OK) return rc;
    return end_launch(c, st, n_rays, 0u);   // samples: the valid listed rays, counted on the device (kQuerySlot)
}

extern "C" int rt_ray_list_compact_async(rt_context* c, uint64_t n_rays, const void* d_list_in, const void* d_count_in,
                                         const void* d_keep, void* d_list_out, void* d_count_out, void* stream) {
    const std::string who = "rt_ray_list_compact_async";
    if (!c || !d_keep) return fail(RT_ERR_INVALID, who + ": NULL argument (ctx or d_keep)");
    if (!d_list_out && !d_count_out) return fail(RT_ERR_INVALID, who + ": no output list (d_list_out and d_count_out are NULL)");
    const ListArgs l{d_list_in, d_count_in, d_list_out, d_count_out, d_keep};
    int rc = check_lists(who, l);
    if (rc != RT_OK) return rc;
    if (n_rays > 0x7FFFFFFFull) return fail(RT_ERR_UNSUPPORTED, who + ": too many rays in one call");
    if (n_rays == 0) return RT_OK;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = begin_launch(c, st)) != RT_OK) return rc;
    if ((rc = launch_compact(c, n_rays, l, st)) != RT_OK) return rc;
    return end_launch(c, st, n_rays, 0u);   // no samples, no segments: a compaction counts nothing else
}

extern "C" int rt_render_rays_async(rt_context* c, uint64_t n_pixels, uint32_t spp, uint32_t rays_per_pixel,
                                    const void* d_origins, const double* origin, const void* d_directions,
                                    uint32_t max_bounces, uint64_t seed, uint32_t pixel_base, uint32_t flags,
                                    void* d_rgb8, void* d_linear, void* stream) {
    const std::string who = "rt_render_rays_async";
    if (!c || !d_directions) return fail(RT_ERR_INVALID, who + ": NULL argument (ctx or d_directions)");
    if ((d_origins != nullptr) == (origin != nullptr))
        return fail(RT_ERR_INVALID, who + ": exactly one of d_origins (per ray) and origin (shared) must be given");
    if (!d_rgb8 && !d_linear) return fail(RT_ERR_INVALID, who + ": both outputs are NULL");
    if (spp == 0) return fail(RT_ERR_INVALID, who + ": spp == 0 (the reference panics: 0/0 in to_u8_array)");
    if (rays_per_pixel == 0 || rays_per_pixel > spp)
        return fail(RT_ERR_INVALID, who + ": rays_per_pixel outside 1..spp");
    if (flags & ~RT_FLAG_ALL) return fail(RT_ERR_INVALID, who + ": unknown flag bits");
    if (flags & ~(RT_FLAG_F32 | RT_FLAG_ROOT2))
        return fail(RT_ERR_UNSUPPORTED, who + ": the live path only (RT_FLAG_F32, RT_FLAG_ROOT2; no RT_FLAG_MODE_*)");
    if (spp > (1u << 20)) return fail(RT_ERR_UNSUPPORTED, who + ": spp > 2^20");
    if ((flags & RT_FLAG_F32) && max_bounces > RT_MAX_BOUNCES_F32)
        return fail(RT_ERR_UNSUPPORTED, who + ": fp32 with max_bounces > RT_MAX_BOUNCES_F32 (3839)");
    if (n_pixels > 0x7FFFFFFFull) return fail(RT_ERR_UNSUPPORTED, who + ": too many pixels in one call");
    if ((uint64_t)pixel_base + n_pixels > (1ull << 32))
        return fail(RT_ERR_INVALID, who + ": pixel_base + n_pixels above 2^32 (the RNG's pixel is 32 bits)");
    if (!c->has_scene) return fail(RT_ERR_INVALID, who + ": no scene set (rt_context_set_scene first)");
    if (n_pixels == 0) return RT_OK;
    const RayArgs a{n_pixels, spp, rays_per_pixel, d_origins, origin, d_directions, max_bounces, seed, pixel_base, flags,
                    d_rgb8, d_linear};
    hipStream_t st = (hipStream_t)stream;
    int rc = begin_launch(c, st);
    if (rc != RT_OK) return rc;
    rc = with_precision((flags & RT_FLAG_F32) != 0, [&](auto t) { return launch_rays<decltype(t)>(c, a, st); });
    if (rc != RT_OK) return rc;
    return end_launch(c, st, n_pixels, 0u);   // samples: valid pixels x spp, counted on the device (rays_validate)
}

extern "C" int rt_camera_rays(const rt_projection* proj, uint32_t grid, uint32_t flags, void* origins, void* directions) {
    const int rc = camera_rays(proj, grid, flags, origins, directions);
    if (rc != kProjOk)
        return fail(rc, "rt_camera_rays: a NULL argument, an empty image, grid == 0, an unknown model or flag, a frame that "
                        "cannot be built (look_at == center, up along the view axis), angle_deg outside (0, 360] or "
                        "extent <= 0 (invalid); more than 2^31 - 1 pixels or grid > 1024 (unsupported)");
    return RT_OK;
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
    DeviceBuffer rec;
    HIPCHK(rec.alloc((size_t)bytes));
    Session& s = c->prog;
    s = Session{};
    s.open = true;
    s.cam = *cam;
    s.rg = rg;
    s.depth = max_bounces;
    s.cap = spp_capacity;
    s.flags = flags;
    s.seed = seed;
    s.rec = std::move(rec);
    s.done.assign((size_t)n_pix, 0u);
    return RT_OK;
}

static int open_session(rt_context* c, const std::string& who) {
    if (!c) return fail(RT_ERR_INVALID, who + ": NULL context");
    if (!c->prog.open) return fail(RT_ERR_INVALID, who + ": no session open on this context");
    return RT_OK;
}

extern "C" int rt_progressive_refine(rt_context* c, double tolerance, uint32_t spp_max, void* stream,
                                     uint64_t* n_active, uint64_t* n_samples) {
    const std::string who = "rt_progressive_refine";
    if (!c || !n_active || !n_samples) return fail(RT_ERR_INVALID, who + ": NULL argument");
    *n_active = 0;
    *n_samples = 0;
    if (!c->prog.open) return fail(RT_ERR_INVALID, who + ": no session open on this context");
    if (tolerance != tolerance) return fail(RT_ERR_INVALID, who + ": tolerance is NaN");
    return refine_step(c, c->prog, who, tolerance, spp_max, (hipStream_t)stream, n_active, n_samples);
}

extern "C" int rt_progressive_refine_items(rt_context* c, uint32_t* samples_per_item, uint64_t* n_items, uint32_t* items,
                                           uint64_t items_capacity) {
    const std::string who = "rt_progressive_refine_items";
    if (!c || !samples_per_item || !n_items) return fail(RT_ERR_INVALID, who + ": NULL argument");
    *samples_per_item = 0;
    *n_items = 0;
    if (!c->prog.open) return fail(RT_ERR_INVALID, who + ": no session open on this context");
    Session& s = c->prog;
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
    Session& s = c->prog;
    if ((rc = sync_done(c, s)) != RT_OK) return rc;
    if (s.done_min == s.done_max) return extend_uniform(c, s, who, spp_total, d_rgb8, d_linear, stream);
    // after a non-uniform map: every pixel goes from its own count to spp_total
    if (spp_total < s.done_max) return fail(RT_ERR_INVALID, who + ": spp_total below the samples a pixel already holds");
    if (spp_total > s.cap) return fail(RT_ERR_INVALID, who + ": spp_total above the session's spp_capacity");
    const std::vector<uint32_t> target(s.done.size(), spp_total);
    const MapReduce red{target.data(), d_rgb8, d_linear};
    bool enqueued = false;
    return run_map(c, s, who, target.data(), &red, d_rgb8 || d_linear ? 1u : 0u, nullptr, 0u, nullptr, (hipStream_t)stream,
                   &enqueued);
}

extern "C" int rt_progressive_extend_map_async(rt_context* c, const uint32_t* spp_target, void* d_rgb8, void* d_linear,
                                               void* stream) {
    const std::string who = "rt_progressive_extend_map_async";
    int rc = open_session(c, who);
    if (rc != RT_OK) return rc;
    Session& s = c->prog;
    if (!spp_target) return fail(RT_ERR_INVALID, who + ": spp_target is NULL");
    if ((rc = sync_done(c, s)) != RT_OK) return rc;
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
        return spp_target[0] == 0u ? RT_OK : extend_uniform(c, s, who, spp_target[0], d_rgb8, d_linear, stream);
    const MapReduce red{spp_target, d_rgb8, d_linear};
    bool enqueued = false;
    return run_map(c, s, who, spp_target, &red, out ? 1u : 0u, nullptr, 0u, nullptr, (hipStream_t)stream, &enqueued);
}

extern "C" int rt_progressive_snapshot_map_async(rt_context* c, const uint32_t* spp_count, void* d_rgb8, void* d_linear,
                                                 void* stream) {
    const std::string who = "rt_progressive_snapshot_map_async";
    int rc = open_session(c, who);
    if (rc != RT_OK) return rc;
    Session& s = c->prog;
    if (!d_rgb8 && !d_linear) return fail(RT_ERR_INVALID, who + ": both outputs are NULL");
    // every pixel at its own count, during or after a refinement run: the classes are already on the device
    if (!spp_count && s.run.started && !s.run.broken) return snapshot_run(c, s, d_rgb8, d_linear, (hipStream_t)stream);
    if ((rc = sync_done(c, s)) != RT_OK) return rc;
    const uint32_t* counts = spp_count ? spp_count : s.done.data();
    for (size_t p = 0; p < s.done.size(); ++p)
        if (counts[p] == 0u || counts[p] > s.done[p])
            return fail(RT_ERR_INVALID, who + ": a count of 0 or above the samples its pixel holds");
    const MapReduce red{counts, d_rgb8, d_linear};
    bool enqueued = false;
    return run_map(c, s, who, nullptr, &red, 1u, nullptr, 0u, nullptr, (hipStream_t)stream, &enqueued);
}

extern "C" int rt_progressive_counts(rt_context* c, uint32_t* out) {
    const std::string who = "rt_progressive_counts";
    int rc = open_session(c, who);
    if (rc != RT_OK) return rc;
    if (!out) return fail(RT_ERR_INVALID, who + ": out is NULL");
    if ((rc = sync_done(c, c->prog)) != RT_OK) return rc;
    std::copy(c->prog.done.begin(), c->prog.done.end(), out);
    return RT_OK;
}

extern "C" int rt_progressive_error_async(rt_context* c, void* d_error, void* stream) {
    const std::string who = "rt_progressive_error_async";
    int rc = open_session(c, who);
    if (rc != RT_OK) return rc;
    Session& s = c->prog;
    if (!d_error) return fail(RT_ERR_INVALID, who + ": d_error is NULL");
    if ((rc = sync_done(c, s)) != RT_OK) return rc;
    return estimate_error(c, s, who, d_error, (hipStream_t)stream);
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
    Session& s = c->prog;
    if (!s.open) return fail(RT_ERR_INVALID, "rt_progressive_end: no session open on this context");
    HIPCHK(hipSetDevice(c->device));
    if (s.have_stream) HIPCHK(hipStreamSynchronize(s.stream));
    const hipError_t e = s.rec.release();   // reported under the call it makes
    if (e != hipSuccess) return fail(RT_ERR_HIP, std::string("hipFree(s.rec): ") + hipGetErrorString(e));
    s = Session{};
    return RT_OK;
}

extern "C" int rt_context_collect(rt_context* c, void* stream, rt_stats* out) {
    if (!c) return fail(RT_ERR_INVALID, "rt_context_collect: NULL context");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;   // NULL = the HIP null stream
    HIPCHK(hipStreamSynchronize(st));
    std::vector<unsigned long long> segs(kSegShards * kSegStride);
    uint32_t errs[2] = {0u, 0u};   // word 0: a pixel channel above 2.0 (finish); word 1: a path step's ray outside its contract
    HIPCHK(hipMemcpy(segs.data(), c->segs.p, segs.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(errs, c->err.p, sizeof(errs), hipMemcpyDeviceToHost));
    const uint32_t err = errs[0];
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
        qrays += segs[(size_t)i * kSegStride + kQuerySlot];   // the valid rays of the queries, the samples of the ray renders' valid pixels
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
    if (errs[1])
        return fail(RT_ERR_INVALID, "rt_scatter_async / rt_path_step_async: a ray with index >= n_spheres or sample >= 2^20 "
                                    "(not scattered; the other rays are as they would be without it); or a ray list with "
                                    "an entry >= n_rays (skipped) or a count > n_rays (clamped)");
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
