/*
 * rt_mi355x.h — C ABI of the MI355X-native Monte-Carlo sample loop.
 *
 * Drop-in boundary for semicolonTransistor/rust-ray-tracing's hot path:
 *   trait Renderer { fn render(&self, max_bounces, samples_per_pixel, &Arc<Scene>, &Arc<Camera>)
 *                    -> (RgbImage, RenderStat) }                     (src/renderer.rs:38-40)
 * whose live implementation is TileRenderer::render (src/renderer.rs:243-387) driving
 * TileRenderTask::render_vectorized2 (src/renderer.rs:141-176) ->
 * Scene::trace_vectorized2 (src/ray_tracing.rs:375-505).  A GPU renderer is a new
 * `impl Renderer` that flattens Scene/Camera into the structs below and calls rt_render
 * (or the device-resident rt_context_* API); the Rust-side binding is in INTEGRATION.md.
 *
 * Everything is plain C: pointers + sizes, caller-owned buffers, int status codes.
 * Thread-safety: rt_render may be called from any thread; one rt_context must not be
 * used concurrently from two threads.
 */
#ifndef RT_MI355X_H
#define RT_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (the reference panics instead; see rt_last_error) ---- */
#define RT_OK 0
#define RT_ERR_INVALID 1     /* bad argument: NULL pointer, spp == 0, material index out of range ...
                                (reference: unwrap()/panic!, e.g. objects.rs:296, materials.rs:31) */
#define RT_ERR_HIP 2         /* HIP runtime failure (no device, launch failure, OOM) */
#define RT_ERR_RANGE 3       /* a pixel channel exceeded 2.0 after /spp: the reference panics in
                                Color::to_u8_array (color.rs:55-57); the image is still written */
#define RT_ERR_UNSUPPORTED 4 /* configuration this build cannot run (e.g. spp > 2^20) */

/* Largest max_bounces an RT_FLAG_F32 render accepts (RT_ERR_UNSUPPORTED above): fp32 draws Philox2x32-10
 * with the counter (pixel, sample | code << 20), code 257 + bounce for the scatter, which must stay below
 * 2^12.  fp64 (Philox4x32-10, the bounce in its own counter word) has no such limit. */
#define RT_MAX_BOUNCES_F32 3839u

/* ---- materials (src/materials.rs:41-155) ---- */
#define RT_LAMBERTIAN 0u
#define RT_METAL 1u
#define RT_DIELECTRIC 2u

typedef struct rt_material {
    uint32_t kind;       /* RT_LAMBERTIAN / RT_METAL / RT_DIELECTRIC */
    uint32_t hollow;     /* Dielectric::hollow (materials.rs:111-114) */
    double albedo[3];    /* Lambertian::albedo / Metal::albedo */
    double fuzz;         /* Metal::fuzzy_factor, already clamped by Metal::new (materials.rs:79-88) */
    double ior;          /* Dielectric::index_of_refraction */
} rt_material;           /* 48 bytes */

/* ---- scene: spheres in scene order (closest-hit ties resolve to the later sphere,
 *      objects.rs:141), Scene::objects (ray_tracing.rs:102-104) flattened SoA ---- */
typedef struct rt_scene {
    uint32_t n_spheres;
    uint32_t n_materials;
    const double* center;         /* [n_spheres][3] */
    const double* radius;         /* [n_spheres] */
    const uint32_t* material;     /* [n_spheres], index into materials */
    const rt_material* materials; /* [n_materials] */
} rt_scene;

/* ---- camera: the precomputed fields of Camera (ray_tracing.rs:15-24) ---- */
typedef struct rt_camera {
    uint32_t image_width, image_height;
    double center[3];   /* Camera::center */
    double ulc[3];      /* Camera::viewport_upper_left_corner */
    double vu[3];       /* Camera::viewport_u */
    double vv[3];       /* Camera::viewport_v */
    double du[3];       /* Camera::defocus_u */
    double dv[3];       /* Camera::defocus_v */
} rt_camera;

/* Pixel set to render: rows row_begin + i*row_step (i < row_count), columns
 * [col_begin, col_begin + col_count).  Outputs are compact over the set:
 * element (i, c) at index i*col_count + c.  NULL = whole image (== RgbImage layout). */
typedef struct rt_tile_range {
    uint32_t row_begin, row_step, row_count;
    uint32_t col_begin, col_count;
} rt_tile_range;

/* RenderStat (renderer.rs:11-34) plus the work counters the roofline needs. */
typedef struct rt_stats {
    double seconds;          /* wall time of the call (host clock) */
    double kernel_ms;        /* device time of the trace kernel(s), HIP events */
    double pixels_per_second;
    uint64_t pixels;
    uint64_t samples;        /* pixels * spp */
    uint64_t ray_segments;   /* enabled rays traced, summed over bounces (ray_tracing.rs:396-401) */
    uint64_t lane_slots;     /* SIMD lanes issued for those traces (64 per wave-bounce);
                                (ray_segments - direct_sky_samples) / lane_slots = lane utilisation */
    uint64_t bounce_iters;   /* bounce-loop iterations executed, summed over pixels */
    /* Executed work of the culls and exact tests, in wave-level tests (each runs all 64 lanes of a
     * wave); DESIGN.md §5 turns them into executed FLOP for the roofline:
     *   box_groups          general sweep, 4 boxes each: 18 v_pk_fma_f32 = 72 fp32 FLOP per lane
     *   filter_groups       general sweep, 4 spheres each: 14 v_pk_fma_f32 = 56 fp32 FLOP per lane
     *   exact_tests         general sweep, one sphere each through Sphere::hit_packed's test
     *                       (objects.rs:252-257): 17 FLOP per lane in the render's precision.  Behind
     *                       the sphere filter the fp32 non-mega kernels count one per step in which
     *                       each lane tests one of its own candidates (a different sphere per lane)
     *   cone_tests          camera sweep, 64 cone records each: 23 fp32 FLOP per lane
     *   camera_exact_tests  camera sweep, one sphere each from the camera-origin table: 8 FLOP per
     *                       lane in the render's precision */
    uint64_t box_groups, filter_groups, exact_tests, cone_tests, camera_exact_tests;
    /* Samples of pixels finished when they are claimed, without tracing: a pinhole camera's pixel
     * whose camera candidate list is empty (no primary ray of the pixel can hit a sphere, so every
     * sample escapes at bounce 0).  Their primary segments are in ray_segments (the reference traces
     * them, ray_tracing.rs:396-401) but occupy no SIMD lane, so they are not in lane_slots. */
    uint64_t direct_sky_samples;
    /* The kernel the last collected render ran (RT_KERNEL_* fields below; 0 = none) and how many of
     * its 4-wave workgroups were resident per CU (hipOccupancyMaxActiveBlocksPerMultiprocessor): equal
     * to the kernel's waves-per-SIMD target unless LDS or registers cut its occupancy. */
    uint32_t kernel_id;
    uint32_t kernel_wg_per_cu;
} rt_stats;

/* rt_stats.kernel_id: trace_paths<T, W, ROOT2, MODE, CAMQ, MEGA> of rt_kernel.hip, one bit field each.
 * Bit 15 is set for any kernel, so 0 means "no render collected". */
#define RT_KERNEL_F64(id) ((id) & 1u)            /* T = double (else float) */
#define RT_KERNEL_WAVES(id) (((id) >> 1) & 7u)   /* W: waves per SIMD the register allocation targets */
#define RT_KERNEL_ROOT2(id) (((id) >> 4) & 1u)   /* quirk Q1 off */
#define RT_KERNEL_MODE(id) (((id) >> 5) & 3u)    /* 0 live path, 1 vectorized, 2 scalar, 3 vectorized3 */
#define RT_KERNEL_CAMQ(id) (((id) >> 7) & 1u)    /* pinhole camera batches */
#define RT_KERNEL_MEGA(id) (((id) >> 8) & 1u)    /* four-level sweep (mega boxes; scenes of > 8 super groups) */
/* Set: the sample-parallel kernels ran, trace_paths_split<T, W, CAMQ, MEGA> followed by finish_records<T>
 * (rt_render_split_async); ROOT2 and MODE are 0 there. */
#define RT_KERNEL_SPLIT(id) (((id) >> 9) & 1u)
/* Set (with RT_KERNEL_SPLIT): a session's item-table kernel ran, trace_paths_items<T, W, CAMQ, MEGA>
 * (rt_progressive_extend_map_async with a non-uniform map). */
#define RT_KERNEL_ITEMS(id) (((id) >> 10) & 1u)
/* Set: the guide-buffer kernel ran, guide_pixels<T, CAMQ, MEGA> (rt_render_guides_async); F64, WAVES, CAMQ and
 * MEGA mean what they mean above, ROOT2, MODE, SPLIT and ITEMS are 0. */
#define RT_KERNEL_GUIDES(id) (((id) >> 11) & 1u)
/* Set: the ray-query kernel ran, query_rays<T, ROOT2, SHARED, MEGA> (rt_query_hits_async); F64, WAVES, ROOT2 and
 * MEGA mean what they mean above, CAMQ is SHARED (the shared-origin path: the camera sweep over the origin's camera
 * tables), MODE, SPLIT, ITEMS and GUIDES are 0. */
#define RT_KERNEL_QUERY(id) (((id) >> 12) & 1u)
/* Set: the caller-ray kernel ran, trace_paths_rays<T, W, ROOT2, MEGA> (rt_render_rays_async; rays_validate<T> runs
 * ahead of it); F64, WAVES, ROOT2 and MEGA mean what they mean above, CAMQ, MODE, SPLIT, ITEMS, GUIDES and QUERY are 0. */
#define RT_KERNEL_RAYS(id) (((id) >> 13) & 1u)
/* Set: the occlusion kernel ran, occlusion_rays<T, ROOT2, MEGA> (rt_query_occluded_async); F64, WAVES, ROOT2 and MEGA
 * mean what they mean above, CAMQ, MODE, SPLIT, ITEMS, GUIDES, QUERY and RAYS are 0. */
#define RT_KERNEL_OCCLUSION(id) (((id) >> 14) & 1u)
/* Above bit 15.  Set: the scatter kernel ran, scatter_rays<T> (rt_scatter_async): F64 means what it means above, every
 * other field is 0 (a map kernel without an occupancy target: WAVES is 0). */
#define RT_KERNEL_SCATTER(id) (((id) >> 16) & 1u)
/* Set: the fused path-step kernel ran, path_step_rays<T, ROOT2, MEGA> (rt_path_step_async); F64, WAVES, ROOT2 and MEGA
 * mean what they mean above, every other field is 0. */
#define RT_KERNEL_STEP(id) (((id) >> 17) & 1u)
/* Set together with RT_KERNEL_STEP: the list step ran, path_step_list<T, ROOT2, MEGA> (rt_path_step_list_async; the
 * compaction kernels follow it where an output list was asked for); F64, WAVES, ROOT2 and MEGA are the step's.  Set
 * alone: a list compaction ran (rt_ray_list_compact_async: keep_ballots, list_tile_sums, list_scan_tiles,
 * list_scatter), kernels without a precision or an occupancy target: F64 and WAVES are 0. */
#define RT_KERNEL_LIST(id) (((id) >> 18) & 1u)

/* ---- flags ---- */
#define RT_FLAG_F32 0x1u     /* compute in fp32 (default: fp64, the reference's arithmetic) */
#define RT_FLAG_ROOT2 0x2u   /* quirk Q1 off: accept the far root like scalar Sphere::hit
                                (objects.rs:228-234) instead of testing root1 twice (objects.rs:273) */
/* Semantics modes (at most one; default = the live path, TileRenderTask::render_vectorized2 ->
 * Scene::trace_vectorized2, renderer.rs:141-176, quirks Q1-Q3 as the reference has them):
 *   RT_FLAG_MODE_VECTORIZED: render_vectorized -> Scene::trace_vectorized (renderer.rs:102-139,
 *     ray_tracing.rs:312-373): each sample keeps its own value and the sky uses its own final
 *     direction (Q2, Q3 off); hit_packed is shared, so Q1 still applies unless RT_FLAG_ROOT2.
 *   RT_FLAG_MODE_VECTORIZED3: render_vectorized3 -> Scene::trace_vectorized3 (renderer.rs:178-213,
 *     ray_tracing.rs:508-628): each sample's own value as in _VECTORIZED, summed in the order an
 *     in-place swap partition (CombinedIndex, :113-214, :561-607) leaves the slots in; the missing
 *     lanes of a partial chunk add sky(0) (white at depth 0).
 *   RT_FLAG_MODE_SCALAR: TileRenderTask::render -> Scene::trace_rays (renderer.rs:68-100,
 *     ray_tracing.rs:264-306): scalar Sphere::hit (objects.rs:216-247; no FMA, both roots, normal
 *     divided by the signed radius), the first of equal hits wins (min_by_key), Color::average. */
#define RT_FLAG_MODE_VECTORIZED 0x4u
#define RT_FLAG_MODE_SCALAR 0x8u
#define RT_FLAG_MODE_VECTORIZED3 0x10u
#define RT_FLAG_ALL 0x1Fu     /* any other bit, or two mode bits, is RT_ERR_INVALID */

/* Camera::new (ray_tracing.rs:27-62).  view_angle and defocus_angle in degrees. */
int rt_camera_new(rt_camera* out, uint32_t image_width, uint32_t image_height, double focal_length,
                  double view_angle_deg, const double center[3], const double look_at[3],
                  const double up[3], double defocus_angle_deg);

/* Metal::new's clamp (materials.rs:79-88): fuzz < 1 ? fuzz : 1. */
double rt_metal_clamp_fuzz(double fuzz);

/* One-shot render, host buffers in/out (replaces TileRenderer::render, renderer.rs:243-387,
 * on the device; scene upload and PCIe copies included).
 *   rgb8:   [pixels][3] RGB8, Color::to_u8_array of (sum / spp)   (may be NULL)
 *   linear: [pixels][3] f64 pixel colour after /spp, before gamma (may be NULL)
 *   stats:  may be NULL
 *   seed:   keys the counter-based draws that replace thread_rng() (ray_tracing.rs:78-79).  fp64
 *           keys Philox4x32-10 with the whole 64-bit seed.  fp32 (RT_FLAG_F32) keys Philox2x32-10,
 *           whose key is 32 bits: seed lo ^ fmix32(seed hi) (murmur3's finaliser; fmix32(0) = 0), so
 *           2^32 seed pairs share each fp32 key, but no structured pattern such as hi == lo does.
 * Returns RT_OK, RT_ERR_RANGE (image written; reference would have panicked) or an error. */
int rt_render(const rt_scene* scene, const rt_camera* camera, uint32_t max_bounces, uint32_t spp,
              uint64_t seed, uint32_t flags, const rt_tile_range* range, uint8_t* rgb8,
              double* linear, rt_stats* stats);

/* ---- device-resident API: scene kept in HBM across calls, outputs in device memory ---- */
typedef struct rt_context rt_context;

/* The renderer object: TileRenderer::new (renderer.rs:232-241) and its drop; one per GPU. */
int rt_context_create(int device, rt_context** out);
int rt_context_destroy(rt_context* ctx);
/* Upload (replace) the scene, the Arc<Scene> handed to Renderer::render (main.rs:43,
 * renderer.rs:38-40); copies fp64 and fp32 SoA images into HBM. */
int rt_context_set_scene(rt_context* ctx, const rt_scene* scene);
/* Enqueue one render on `stream` (a hipStream_t; NULL = the HIP null stream, as in every HIP
 * API): the pixels of `range` through TileRenderTask::render_vectorized2 (renderer.rs:141-176),
 * i.e. one share of TileRenderer::render's tile loop (renderer.rs:248-296).  d_rgb8 / d_linear are device pointers (either may be NULL).  Asynchronous.  Renders on
 * one context share its work counter, scratch and camera table: a render on a different stream
 * than the previous one first synchronises the previous stream, so they never overlap.  Use one
 * context per concurrent stream for overlap. */
int rt_render_async(rt_context* ctx, const rt_camera* camera, uint32_t max_bounces, uint32_t spp,
                    uint64_t seed, uint32_t flags, const rt_tile_range* range, void* d_rgb8,
                    void* d_linear, void* stream);
/* rt_render_async with a pixel's samples dealt to several waves, for launches with fewer pixels than the
 * chip has resident waves (previews, crops, thin shards, one pixel at a very high spp).  A work item is a
 * (pixel, sample sub-range); a tracing kernel writes every sample's record into a context-owned record
 * buffer and a second kernel, enqueued right behind it on `stream`, reduces each pixel in the reference's
 * order.  The image is bit-identical to rt_render_async's.
 * samples_per_item:
 *   0  = the library plans from the launch shape (rt_split_plan).  When the plan is one item per pixel, or
 *        the record buffer would exceed the scratch budget (24 GB), the call IS rt_render_async (same
 *        kernel, same stats).
 *   >0 = forced, any value in 1..2^20 (larger: RT_ERR_INVALID); a value >= spp runs one item per pixel
 *        through the split kernels.
 * Flags: RT_FLAG_F32 only.  RT_FLAG_ROOT2 or any RT_FLAG_MODE_* is RT_ERR_UNSUPPORTED; otherwise the
 * argument checks are rt_render_async's.  More than 0x7FFFFFFF work items, or (forced) a record buffer over
 * the scratch budget, is RT_ERR_UNSUPPORTED.
 * rt_context_collect after it: RT_KERNEL_SPLIT(kernel_id) is set when the split kernels ran, kernel_ms
 * covers both kernels, and samples, pixels, ray_segments and bounce_iters equal the unsplit render's.
 * lane_slots, direct_sky_samples (0 here: sky pixels are traced like any other) and the executed-work
 * counters may differ. */
int rt_render_split_async(rt_context* ctx, const rt_camera* camera, uint32_t max_bounces, uint32_t spp,
                          uint64_t seed, uint32_t flags, const rt_tile_range* range, void* d_rgb8,
                          void* d_linear, void* stream, uint32_t samples_per_item);
/* ---- guide buffers: what a denoiser or an edge-aware filter needs beside a noisy preview ----
 * Per pixel the mean first-hit albedo, normal, depth and coverage over the primary rays of the image that
 * rt_render_async makes with the same camera, spp, seed and precision (flags).  Draws are keyed by (pixel,
 * sample, bounce), so the guides at n samples come from exactly the primary rays of the image at n samples:
 * their edges lie where the image's lie.  Nothing is scattered and no colour is computed.
 * Definition, for a pixel with n = spp samples and sample s in [0, n), in the render's precision T (fp64, or
 * fp32 under RT_FLAG_F32):
 *   primary ray  Camera::get_ray for (col, row, s, pix = row * W + col, seed): bit for bit the ray
 *                rt_render_async traces at bounce 0 (the same draws, the same fp32 key fold).
 *   hit          the live path's closest hit at bounce 0: Sphere::hit_packed with quirk Q1 as the reference has
 *                it (a ray whose near root is invalid has no hit), the later sphere wins ties, t in [0.001, inf);
 *                then PackedHitRecords::finalize: loc = o + d t, normal = unit(loc - centre) with the packed
 *                length, front = pk_dot(d, normal) < 0, the normal negated when not front.
 *   per sample   albedo_s: the attenuation the render's path takes at bounce 0, i.e. the material's albedo
 *                rounded to T for Lambertian and Metal, (1, 1, 1) for Dielectric, (1, 1, 1) on a miss;
 *                normal_s: the finalized normal (against the ray), (0, 0, 0) on a miss;
 *                depth_s: t (directions are unit: a distance), 0 on a miss;
 *                coverage_s: 1 on a hit, 0 on a miss.
 *   reduction    fixed, so that a value is a function of the samples alone, never of the launch; each channel on
 *                its own.  Every per-sample value is converted to double; partial j (j in 0..63, starting at
 *                +0.0) adds the samples with s % 64 == j in ascending s; the 64 partials are folded
 *                for h in 32, 16, 8, 4, 2, 1: p[i] += p[i + h] for i < h; the output is (float)(p[0] / (double)n).
 * Every output is float32.  The means are over all n samples, so they are premultiplied by coverage: a consumer
 * that wants the mean over the hits divides by coverage.
 * Outputs: device pointers, compact over the range like d_rgb8; d_albedo and d_normal [pixels][3] float,
 * d_depth and d_coverage [pixels] float.  Any may be NULL; a value does not depend on which others were asked for.
 * Asynchronous on `stream` under rt_render_async's cross-stream rule.  It uses the context's scene and camera
 * tables with a render's rebuild rule, is allowed while a progressive session is open and touches neither the
 * session's records nor its counts.
 * flags: RT_FLAG_F32 or 0.  RT_ERR_UNSUPPORTED: RT_FLAG_ROOT2 or any RT_FLAG_MODE_*, spp > 2^20, more than
 * 0x7FFFFFFF pixels.  RT_ERR_INVALID: unknown flag bits, ctx or camera NULL, spp == 0, all four outputs NULL, a
 * bad range.  Never RT_ERR_RANGE: nothing is quantised.
 * rt_context_collect after it: pixels is the pixel count, samples = ray_segments = pixels * spp, bounce_iters = 0,
 * kernel_ms covers the kernel, RT_KERNEL_GUIDES(kernel_id) is set; the executed-work counters hold what the
 * reused camera sweep counts. */
int rt_render_guides_async(rt_context* ctx, const rt_camera* camera, uint32_t spp, uint64_t seed, uint32_t flags,
                           const rt_tile_range* range, void* d_albedo, void* d_normal, void* d_depth,
                           void* d_coverage, void* stream);
/* ---- ray queries: the closest hit of caller-supplied rays ----
 * What is under a pixel of a preview, rays of a camera model the reference lacks (orthographic, fisheye, panorama),
 * occlusion passes over first hits, an integrator driven from the host's own device tensors: n_rays rays through the
 * sweeps the renders run, one result per ray.  T is float under RT_FLAG_F32 and double otherwise.
 * Rays:
 *   d_directions  device [n_rays][3] of T (the natural (n, 3) tensor).  Directions are NOT normalised.
 *   origins       exactly one of the two forms (both or neither: RT_ERR_INVALID):
 *                 per ray: d_origins is device [n_rays][3] of T and origin is NULL;
 *                 shared:  d_origins is NULL and origin is 3 HOST doubles, rounded to T the way a camera centre is
 *                          ((T)origin[i]).  The call then runs the camera sweep over the camera tables of that origin,
 *                          which it builds under rt_render_async's rule (a later render with another centre rebuilds
 *                          them).  Both forms give the same values for the same rays.
 * Definition, per ray (o, d), in T:
 *   hit      the closest hit of the live path over all spheres in scene order: Sphere::hit_packed
 *            (objects.rs:249-290) plus PackedHitRecords::update (objects.rs:140-155).  t in [0.001, inf); ties go to
 *            the later sphere; quirk Q1 applies (the near root is tested twice, so a ray whose near root is invalid,
 *            e.g. one that starts inside a sphere, misses that sphere) unless RT_FLAG_ROOT2, which accepts the far
 *            root like scalar Sphere::hit.  Picking wants RT_FLAG_ROOT2.
 *   t        the ray parameter of the hit: the hit point is o + d t, a distance only when |d| = 1.
 *   then PackedHitRecords::finalize (objects.rs:157-162), as the guide buffers have it:
 *   point    o + d t (a multiply, then an add: no FMA)
 *   normal   (point - centre) / sqrt(|point - centre|^2) with the packed (mul_add) length, negated when not front
 *   front    pk_dot(d, normal) < 0, taken before the negation
 *   index    the sphere's scene index.
 *   A miss:  index -1, t +inf, normal and point 0, front 0.
 * Precondition, enforced per ray: a ray is invalid when a component of its origin or direction is not finite, or
 * when |d|^2 (PackedVec3::length_squared, in T) is outside [1e-6, 1e6], the constants rounded to T: the range of
 * direction lengths the culls are proven for; it also excludes a zero direction.  The bounds themselves are valid.
 * An invalid ray is not traced: index -2 (RT_QUERY_INVALID), t NaN, normal and point 0, front 0, and the results of
 * the other rays do not depend on it.
 * Outputs: device pointers, any may be NULL, all of them NULL is RT_ERR_INVALID.  d_t: T [n_rays]; d_index: int32
 * [n_rays]; d_normal, d_point: T [n_rays][3]; d_front: uint8 [n_rays].  A value does not depend on which other outputs
 * were asked for.
 * flags: RT_FLAG_F32 and RT_FLAG_ROOT2.  Any RT_FLAG_MODE_* is RT_ERR_UNSUPPORTED; unknown bits are RT_ERR_INVALID.
 * n_rays == 0: RT_OK, nothing is enqueued.  n_rays > 0x7FFFFFFF: RT_ERR_UNSUPPORTED.  RT_ERR_INVALID, checked before
 * any HIP call: ctx or d_directions NULL, no scene set.
 * Asynchronous on `stream` under rt_render_async's cross-stream rule.  Allowed while a progressive session is open;
 * touches neither its records nor its counts.
 * rt_context_collect after it: pixels = n_rays, samples = ray_segments = the valid rays, bounce_iters = 0, lane_slots
 * 64 per batch of 64 consecutive rays with a valid ray in it, RT_KERNEL_QUERY(kernel_id) is set; the executed-work
 * counters hold what the reused sweeps count.
 * Out of scope: sorting or binning incoherent rays, the scalar mode, radiance (a per-ray t_max and the any-hit exit:
 * rt_query_occluded_async below). */
#define RT_QUERY_MISS (-1)
#define RT_QUERY_INVALID (-2)
int rt_query_hits_async(rt_context* ctx, uint64_t n_rays, const void* d_origins, const double* origin,
                        const void* d_directions, uint32_t flags, void* d_t, void* d_index, void* d_normal,
                        void* d_point, void* d_front, void* stream);
/* ---- occlusion queries: is anything in the way before t_max ----
 * Shadow rays towards a light, ambient occlusion, visibility between two points, line of sight: n_rays rays, each with
 * a bound t_max of its own, one byte per ray.  T is float under RT_FLAG_F32 and double otherwise.  The sweep stops
 * working for a ray at its first accepted hit and never enters a box that lies wholly past the ray's t_max.
 * Definition, per ray (o, d, t_max), in T:
 *   occluded  some sphere's accepted root r satisfies r < t_max, strictly.  The accepted root is exactly
 *             rt_query_hits_async's hit rule: Sphere::hit_packed's near root when it lies in [0.001, inf); quirk Q1
 *             applies unless RT_FLAG_ROOT2, which accepts the far root when the near one is not valid.  Equivalently:
 *             rt_query_hits_async's closest hit of (o, d) exists and its t < t_max.  Strict, so a shadow ray whose
 *             t_max is the t of a known hit does not report that hit.  Directions are NOT normalised, so d = light - p
 *             with t_max = 1 asks about the open segment up to the light.
 *   valid     a ray is valid when it meets rt_query_hits_async's precondition (finite components, |d|^2 in T within
 *             [1e-6, 1e6], the bounds themselves valid) and its t_max is not NaN.  t_max may be +inf (unbounded),
 *             negative, zero or -inf.  A valid ray with t_max <= T(0.001) is never occluded and is not traced.
 * Output: d_occluded, device uint8 [n_rays]: 0 (RT_OCCLUDED_NO) not occluded, 1 (RT_OCCLUDED_YES) occluded, 255
 * (RT_OCCLUDED_INVALID) an invalid ray, not traced.  No ray's value depends on any other ray.
 * Rays: d_directions and the two origin forms are rt_query_hits_async's (exactly one form; a shared origin is rounded
 * as (T)origin[i] and broadcast).  Both forms run the general sweep, as rt_render_rays_async does (no camera tables),
 * and give identical bytes.
 * t_max: d_t_max is device [n_rays] of T, or NULL; when NULL every ray uses (T)t_max, when given the host t_max is
 * not read.
 * flags: RT_FLAG_F32 and RT_FLAG_ROOT2.  Any RT_FLAG_MODE_* is RT_ERR_UNSUPPORTED; unknown bits are RT_ERR_INVALID.
 * n_rays == 0: RT_OK, nothing is enqueued.  n_rays > 0x7FFFFFFF: RT_ERR_UNSUPPORTED.  RT_ERR_INVALID, checked before
 * any HIP call: ctx, d_directions or d_occluded NULL, both or neither origin form, d_t_max NULL and the host t_max NaN,
 * no scene set.
 * Asynchronous on `stream` under rt_render_async's cross-stream rule.  Allowed while a progressive session is open;
 * touches neither its records nor its counts.
 * rt_context_collect after it: pixels = n_rays, samples = ray_segments = the valid rays, bounce_iters = 0, lane_slots
 * 64 per batch of 64 consecutive rays of which at least one entered the sweep (valid, t_max > 0.001),
 * RT_KERNEL_OCCLUSION(kernel_id) is set; the executed-work counters hold what the sweep counted before it stopped.
 * Out of scope: a shared-origin path over the camera tables, sorting or binning incoherent rays, which sphere
 * occludes, a t_min other than 0.001, the scalar and vectorized* modes. */
#define RT_OCCLUDED_NO 0
#define RT_OCCLUDED_YES 1
#define RT_OCCLUDED_INVALID 255
int rt_query_occluded_async(rt_context* ctx, uint64_t n_rays, const void* d_origins, const double* origin,
                            const void* d_directions, const void* d_t_max, double t_max, uint32_t flags,
                            void* d_occluded, void* stream);
/* ---- path steps: the material stage, for integrators the caller drives ----
 * rt_query_hits_async says what a ray hits; these two produce the next ray and the attenuation, so that query ->
 * scatter -> query is a path tracer whose loop, lights, outputs and termination rule belong to the caller (next-event
 * estimation with rt_query_occluded_async, per-bounce outputs, ...).  T is float under RT_FLAG_F32, else double.
 *
 * rt_scatter_async: the material stage alone.  Per ray i with d_index[i] >= 0 it is exactly what a render does to a
 * ray that hit sphere d_index[i] at parameter d_t[i] on bounce `bounce`:
 *   PackedHitRecords::finalize (objects.rs:157-162): point o + d t, the normal with the packed length, front taken
 *     before the negation; then Material::get_hit_result (materials.rs:54-147) with its one draw from stream 2 at
 *     counter (d_sample[i], d_pixel[i], bounce), the keys derived from `seed` as rt_render_async derives them (the
 *     fp32 fold included).
 *   out origin: the hit point; out direction: the scattered direction, NOT normalised, as a render leaves it;
 *   d_colour[i] *= attenuation, in place, component by component as the render multiplies (the albedo rounded to T
 *     for Lambertian and Metal, 1 for Dielectric).
 * A ray with d_index[i] < 0 (RT_QUERY_MISS, RT_QUERY_INVALID) is not scattered: its outputs are its inputs bit for
 * bit and its colour is untouched.  No ray's values depend on another ray.
 * Arguments: d_directions T [n][3]; the origins in rt_query_hits_async's two forms (exactly one); d_index int32 [n]
 * and d_t T [n] as rt_query_hits_async writes them; d_pixel, d_sample uint32 [n]; d_colour T [n][3] or NULL (no
 * colour is tracked); d_out_origins, d_out_directions T [n][3], one of them may be NULL; they may be the input arrays
 * (in place) or separate ones, with identical values.
 * d_index[i] >= n_spheres or d_sample[i] >= 2^20 (on a ray with d_index[i] >= 0): the ray is left as a miss is and
 * rt_context_collect returns RT_ERR_INVALID; the other rays are untouched by it.
 * flags: RT_FLAG_F32 and RT_FLAG_ROOT2 (the scatter does not depend on ROOT2).  Any RT_FLAG_MODE_* is
 * RT_ERR_UNSUPPORTED; unknown bits are RT_ERR_INVALID.  RT_ERR_UNSUPPORTED: fp32 with bounce > RT_MAX_BOUNCES_F32
 * (a render's own bounces end one below it; at RT_MAX_BOUNCES_F32 itself the fp32 counter's code wraps and the draw is
 * stream 0's block of that sample), n_rays > 0x7FFFFFFF.  n_rays == 0: RT_OK, nothing is enqueued.  RT_ERR_INVALID, checked before any HIP call: ctx,
 * d_directions, d_index, d_t, d_pixel or d_sample NULL, both output arrays NULL, both or neither origin form, no scene.
 * rt_context_collect after it: pixels = n_rays, samples = the scattered rays, ray_segments = bounce_iters = 0,
 * RT_KERNEL_SCATTER(kernel_id) is set.
 *
 * rt_path_step_async: closest hit and scatter in one kernel.  Per ray, bit for bit, what rt_query_hits_async followed
 * by rt_scatter_async does on the same arrays in place, without the trip through memory between them:
 *   a hit becomes the scattered ray (d_origins, d_directions and d_colour are updated);
 *   a miss, and a ray outside the query's precondition (not traced), keep their origin, direction and colour: a
 *   caller retires a ray by zeroing its direction.
 * d_status uint8 [n]: RT_STEP_SCATTERED, RT_STEP_MISSED (not scattered) or RT_STEP_INVALID.  d_index, d_t, d_normal
 * and d_front are rt_query_hits_async's outputs for the hit that was scattered (the hit point is the new origin; the
 * normal is what a shadow ray or a BSDF weight needs).  Any of the five may be NULL and no value depends on which
 * were asked for.  Origins are per ray only (the call writes them back); d_colour may be NULL.
 * Flags, limits and the sample check are rt_scatter_async's.  RT_ERR_INVALID before any HIP call: ctx, d_origins,
 * d_directions, d_pixel or d_sample NULL, no scene.
 * rt_context_collect after it: pixels = n_rays, samples = ray_segments = the valid rays, bounce_iters = 0, lane_slots
 * and the work counters as rt_query_hits_async counts them, RT_KERNEL_STEP(kernel_id) is set.
 *
 * The loop "colour = 1; for k < max_bounces: step; a miss multiplies by the sky of its own direction and retires; a
 * ray alive at the end is 0" over a camera's primary rays (pixel = row W + col, sample = s), reduced as
 * ((((0 + a0) + a1) + a2) + a3) / spp with a_l the sum over chunks j of sample 4 j + l, is bit for bit
 * rt_render_async's linear output under RT_FLAG_MODE_VECTORIZED, as long as no scattered direction leaves the query's
 * |d|^2 range (a render traces those too).
 * Both calls are asynchronous on `stream` under rt_render_async's cross-stream rule and allowed while a progressive
 * session is open.  Out of scope: sorting live rays between steps (compacting them: the ray lists below), a shared
 * origin in the fused call, the scalar and vectorized* semantics. */
#define RT_STEP_MISSED 0
#define RT_STEP_SCATTERED 1
#define RT_STEP_INVALID 255
int rt_scatter_async(rt_context* ctx, uint64_t n_rays, const void* d_origins, const double* origin,
                     const void* d_directions, const void* d_index, const void* d_t,
                     const void* d_pixel, const void* d_sample, uint32_t bounce, uint64_t seed, uint32_t flags,
                     void* d_colour, void* d_out_origins, void* d_out_directions, void* stream);
int rt_path_step_async(rt_context* ctx, uint64_t n_rays, void* d_origins, void* d_directions, void* d_colour,
                       const void* d_pixel, const void* d_sample, uint32_t bounce, uint64_t seed, uint32_t flags,
                       void* d_status, void* d_index, void* d_t, void* d_normal, void* d_front, void* stream);
/* ---- ray lists: path steps over the live rays only, compacted on the device ----
 * A ray list is a device array uint32_t list[n_rays] of ray ids plus a device word uint32_t count: the first count
 * entries are the list, entries past count are never read.  The ray arrays (d_origins, d_directions, d_colour, d_pixel,
 * d_sample and every output) stay where they are and are indexed by ray id; only the list shrinks.
 *
 * rt_path_step_list_async: for each listed ray r = list_in[i], i < count, exactly what rt_path_step_async does to ray
 * r, bit for bit: the ray, the colour, d_status[r] and the optional d_index[r], d_t[r], d_normal[r], d_front[r].
 * No byte of any array is written at a ray that is not listed: a retired ray keeps its final direction, colour and last
 * status (RT_STEP_MISSED, RT_STEP_SCATTERED, RT_STEP_INVALID) for the caller to read once at the end.
 * d_list_in NULL: the identity list 0 .. n_rays - 1.  d_count_in NULL: count = n_rays (both NULL: a first step needs
 * no list).  d_list_out and d_count_out, given together or both NULL (no output list): list_out receives list_in[i]
 * for every i whose ray reported RT_STEP_SCATTERED, in increasing i (stable order: an increasing list stays increasing,
 * and the list is reproducible byte for byte), and *count_out how many.  Words of list_out past *count_out are not
 * written.
 *
 * rt_ray_list_compact_async: the same selection under the caller's own rule: entry i is kept iff
 * d_keep[list_in[i]] != 0 (d_keep uint8 [n_rays], by ray id): Russian roulette, a throughput cut-off, or a list built
 * from a status array (d_list_in NULL, d_keep = d_status).
 *
 * Lists: a list entry >= n_rays is skipped (no ray is touched for it, it is never in list_out), a count > n_rays is
 * clamped to n_rays; either sets the error word rt_scatter_async's sample check sets, so rt_context_collect returns
 * RT_ERR_INVALID.  The kernels check these bounds and never fault on a bad list.  A ray id listed twice is undefined
 * for that ray only.
 * RT_ERR_INVALID before any HIP call: d_list_out == d_list_in or d_count_out == d_count_in when both are non-NULL
 * (callers ping-pong two lists and two counts); exactly one of d_list_out and d_count_out given; d_keep NULL; a
 * compaction with no output list; and for the step rt_path_step_async's own (ctx, d_origins, d_directions, d_pixel or
 * d_sample NULL, no scene).  Flags, limits and the sample check are rt_path_step_async's: n_rays == 0: RT_OK, nothing
 * is enqueued; n_rays > 0x7FFFFFFF: RT_ERR_UNSUPPORTED; any RT_FLAG_MODE_*: RT_ERR_UNSUPPORTED.
 * Both calls are asynchronous on `stream` under rt_render_async's cross-stream rule and allowed while a progressive
 * session is open; several may be enqueued and collected once, and no call reads the count on the host.  The
 * compaction's scratch (a 64-bit word per 64 list positions, a word per tile) belongs to the context and only grows.
 * Environment RT_LIST_TILE (64 .. 65536, a power of two; read at every call, any other value ignored): the rays per
 * tile of the compaction's scan, default 65536.  It changes no result.
 * rt_context_collect after them: pixels = n_rays per call; a step's samples = ray_segments = the valid listed rays,
 * lane_slots and the work counters as rt_path_step_async counts them; a compaction counts nothing.
 * RT_KERNEL_LIST(kernel_id) is set, together with RT_KERNEL_STEP by a step.
 * Out of scope: occlusion queries and rt_scatter_async over a list, sorting or binning a list, moving the ray arrays. */
int rt_path_step_list_async(rt_context* ctx, uint64_t n_rays, const void* d_list_in, const void* d_count_in,
                            void* d_origins, void* d_directions, void* d_colour, const void* d_pixel, const void* d_sample,
                            uint32_t bounce, uint64_t seed, uint32_t flags,
                            void* d_status, void* d_index, void* d_t, void* d_normal, void* d_front,
                            void* d_list_out, void* d_count_out, void* stream);
int rt_ray_list_compact_async(rt_context* ctx, uint64_t n_rays, const void* d_list_in, const void* d_count_in,
                              const void* d_keep /* uint8 [n_rays], by ray id */,
                              void* d_list_out, void* d_count_out, void* stream);
/* ---- rendering caller-supplied primary rays: any camera model, full paths ----
 * rt_render_async with the primary rays taken from the caller's arrays instead of Camera::get_ray: an orthographic
 * view, a fisheye, a 360 degree panorama (rt_camera_rays below makes their rays) or the rays of the caller's own
 * tensors, path-traced to an image.  T is float under RT_FLAG_F32 and double otherwise; R = rays_per_pixel, 1 <= R <= spp.
 * Definition:
 *   pixel p   in [0, n_pixels) is the live path's pixel (render_vectorized2 -> trace_vectorized2, quirks Q1-Q3 as
 *             rt_render_async has them): spp samples in chunks of 4.
 *   sample s  starts as ray p R + (s mod R) of the caller's arrays, taken as given: directions are NOT normalised, and
 *             quirk Q2's sky reads the primary direction's y as supplied.
 *   draws     every later draw is the render's: stream 2, counter (s, pix, bounce) with pix = pixel_base + p.  Streams
 *             0 and 1 (the camera's jitter and defocus disk) are never drawn.  pixel_base + n_pixels above 2^32 is
 *             RT_ERR_INVALID; shards of one frame pass their first pixel as pixel_base to keep their streams apart.
 * Rays: d_directions is device [n_pixels R][3] of T; the origins come in exactly the two forms of rt_query_hits_async
 * (per ray: d_origins device [n_pixels R][3] of T; shared: 3 HOST doubles rounded as (T)origin[i]).  Both forms give
 * identical values, and both run every bounce through the general sweep (no camera batches over a shared origin).
 * Precondition, per ray: the query's (finite components, |d|^2 in T within [1e-6, 1e6], the bounds included).  A pixel
 * with an invalid ray among its R is not traced: its linear output is NaN x 3, its rgb8 is 0, 0, 0, it raises no
 * RT_ERR_RANGE and the other pixels do not depend on it.  (A fisheye pixel outside the image circle is such a pixel.)
 * Outputs: rt_render_async's, d_rgb8 [n_pixels][3] u8 and d_linear [n_pixels][3] double, device pointers, one of them
 * may be NULL.  RT_ERR_RANGE is reported at rt_context_collect as for a render.
 * flags: RT_FLAG_F32 and RT_FLAG_ROOT2.  Any RT_FLAG_MODE_* is RT_ERR_UNSUPPORTED; unknown bits are RT_ERR_INVALID.
 * n_pixels == 0: RT_OK, nothing is enqueued.  RT_ERR_UNSUPPORTED: spp > 2^20, fp32 with max_bounces >
 * RT_MAX_BOUNCES_F32, n_pixels > 0x7FFFFFFF.  RT_ERR_INVALID, checked before any HIP call: ctx or d_directions NULL,
 * both or neither origin form, both outputs NULL, spp == 0, R == 0 or R > spp, no scene set.
 * Asynchronous on `stream` under rt_render_async's cross-stream rule.  Allowed while a progressive session is open;
 * touches neither its records nor its counts.
 * rt_context_collect after it: pixels = n_pixels, samples = valid pixels x spp, ray_segments and bounce_iters as a
 * render counts them (over the valid pixels), RT_KERNEL_RAYS(kernel_id) is set.
 * Out of scope: sample-parallel splitting, progressive sessions and guides over caller rays, the other semantics
 * modes, sorting or binning incoherent rays. */
int rt_render_rays_async(rt_context* ctx, uint64_t n_pixels, uint32_t spp, uint32_t rays_per_pixel,
                         const void* d_origins, const double* origin, const void* d_directions,
                         uint32_t max_bounces, uint64_t seed, uint32_t pixel_base, uint32_t flags,
                         void* d_rgb8, void* d_linear, void* stream);
/* Host only, needs no GPU: the primary rays of three camera models the reference lacks, for rt_render_rays_async
 * (rays_per_pixel = grid^2) or rt_query_hits_async.  origins and directions are HOST arrays
 * [image_width image_height grid^2][3] of T (float under RT_FLAG_F32, else double), pixels row-major from the top
 * left, and within a pixel ray r = j grid + i goes through the sub-pixel position ((i + 0.5) / grid, (j + 0.5) / grid).
 * The frame is Camera::new's (ray_tracing.rs:34-37): dir = unit(look_at - center), w = -dir, u = unit(up x w) (right),
 * v = w x u (up).  Everything is computed in double; directions are unit in double; values are rounded to T last.
 * A fisheye pixel outside the image circle gets the direction 0, 0, 0: an invalid ray, so rt_render_rays_async
 * renders that pixel black (linear NaN) and rt_query_hits_async reports RT_QUERY_INVALID.
 * RT_ERR_INVALID: a NULL argument, an empty image, grid == 0, an unknown model, a flag other than RT_FLAG_F32, a frame
 * that cannot be built (non-finite, look_at == center, up along the view axis), a fisheye angle_deg outside
 * (0, 360], an orthographic extent that is not a positive number.  RT_ERR_UNSUPPORTED: more than 0x7FFFFFFF pixels,
 * grid > 1024. */
#define RT_PROJ_ORTHOGRAPHIC 0u   /* parallel rays along the view axis; origins on a plane through center,
                                     `extent` world units high, width by the aspect ratio */
#define RT_PROJ_EQUIRECT 1u       /* 360 x 180 degrees: longitude over columns, latitude over rows, one origin */
#define RT_PROJ_FISHEYE 2u        /* equidistant: angle from the axis = r * angle_deg / 2, r = distance from the
                                     image centre in units of half the shorter side; r > 1: a zero direction */
typedef struct rt_projection {
    uint32_t model, image_width, image_height;
    double center[3], look_at[3], up[3];
    double angle_deg, extent;   /* fisheye: the full field of view in degrees; orthographic: the view's height */
} rt_projection;
int rt_camera_rays(const rt_projection* proj, uint32_t grid, uint32_t flags, void* origins, void* directions);
/* The plan rt_render_split_async makes for samples_per_item = 0; host only, needs no GPU.
 * resident_waves: the waves the split kernels keep resident (CUs x 4 SIMDs x 5 waves in fp32, x 4 in fp64).
 * Returns the samples per item (a multiple of 128, or spp when the plan is one item per pixel) and the
 * item count.  The plan aims at about 8 items per resident wave and splits only launches with fewer pixels
 * than resident waves.  RT_ERR_INVALID: NULL output, no pixels or spp == 0; RT_ERR_UNSUPPORTED: spp > 2^20 or more
 * than 0x7FFFFFFF items. */
int rt_split_plan(uint64_t n_pixels, uint32_t spp, uint32_t resident_waves, uint32_t* samples_per_item,
                  uint64_t* n_items);
/* ---- progressive sessions: add samples to a frame, take an image at any count ----
 * A session keeps every sample's record (primary y, colour, termination bounce) in a record buffer of its own,
 * laid out for spp_capacity samples per pixel: 17 bytes per sample of capacity in fp32, 33 in fp64 (36 / 68
 * when max_bounces > 254), per pixel rounded up to 256 bytes.  1920x1080 at 512 spp is 18.0 GB in fp32 and
 * 35.0 GB in fp64.  The RNG is keyed by (pixel, sample, bounce), so a sample's record does not depend on how
 * many samples its pixel will have, and the image after n samples is bit for bit rt_render_async's at spp = n
 * with the same arguments, for every n; going from n to m traces only the m - n new samples.
 * The live path only (flags: RT_FLAG_F32 or 0).  One session per context; rt_render_async and
 * rt_render_split_async may be interleaved with it on the same context (they share the counter, scratch and
 * camera tables under rt_render_async's cross-stream rule and never touch the session's records). */

/* Host only, needs no GPU: the bytes of record buffer a session needs, n_pixels regions of
 * spp_capacity rounded up to 4 samples.  RT_ERR_INVALID: NULL output, no pixels, spp_capacity == 0, unknown
 * flag bits; RT_ERR_UNSUPPORTED: spp_capacity > 2^20, more than 0x7FFFFFFF pixels, RT_FLAG_ROOT2 or a
 * RT_FLAG_MODE_*. */
int rt_progressive_bytes(uint64_t n_pixels, uint32_t spp_capacity, uint32_t max_bounces, uint32_t flags,
                         uint64_t* bytes);
/* Open a session on ctx: fixes the camera, max_bounces, seed, flags, range (NULL = whole image) and
 * spp_capacity and allocates the record buffer.  max_bytes: the most it may allocate; 0 = the library's
 * scratch budget (24 GB).  Synchronous.
 * RT_ERR_INVALID: a session is already open, spp_capacity == 0, unknown flag bits, a bad range;
 * RT_ERR_UNSUPPORTED: a flag other than RT_FLAG_F32, spp_capacity > 2^20, fp32 with max_bounces >
 * RT_MAX_BOUNCES_F32, more than 0x7FFFFFFF pixels (an extend has one work item per pixel at least), a record
 * buffer over max_bytes.  While a session is open rt_context_set_scene is RT_ERR_INVALID (the records belong
 * to the scene they were traced in). */
int rt_progressive_begin(rt_context* ctx, const rt_camera* camera, uint32_t max_bounces, uint32_t spp_capacity,
                         uint64_t seed, uint32_t flags, const rt_tile_range* range, uint64_t max_bytes);
/* Trace samples [done, spp_total) of every pixel (done: the spp_total of the previous extend, 0 at first),
 * then, if d_rgb8 or d_linear is non-NULL, reduce samples [0, spp_total) into them.  Asynchronous on `stream`,
 * same cross-stream rule as rt_render_async.  The window is planned like rt_split_plan(pixels, spp_total -
 * done, resident waves) and always runs the sample-parallel kernels.
 *   spp_total == done with an output: a snapshot (the reduction only).
 *   spp_total > done with both outputs NULL: tracing only.
 *   spp_total == done with both outputs NULL: RT_OK, nothing is enqueued.
 * RT_ERR_INVALID: no session open, spp_total == 0, below done or above spp_capacity.
 * rt_context_collect after it: the outputs and the return code (RT_ERR_RANGE included) are those of
 * rt_render_async at spp = spp_total.  samples and ray_segments count the samples traced since the last
 * collect, so their sums over a session's collects up to n equal the unsplit render's at spp = n;
 * bounce_iters gets every pixel's K once per reduction, pixels the pixel count once per extend that enqueued
 * work; RT_KERNEL_SPLIT(kernel_id) is set and kernel_ms covers the trace and reduction kernels. */
int rt_progressive_extend_async(rt_context* ctx, uint32_t spp_total, void* d_rgb8, void* d_linear, void* stream);

/* ---- per-pixel sample counts: stop spending samples on pixels that are converged ----
 * A session holds done_p samples of pixel p.  "Pixel" is an index in the range's compact order, the order of the
 * outputs; every array below has one element per pixel of the session's range.  Pixel p's value at n_p samples
 * is rt_render_async's at spp = n_p for that pixel, bit for bit, whatever the other pixels hold.
 * A region is still laid out for spp_capacity samples (rt_progressive_bytes): pixels that stop early save
 * tracing time, not memory. */

/* Trace samples [done_p, spp_target[p]) of every pixel, then, if an output is given, reduce [0, spp_target[p]).
 * spp_target: HOST array, read before the call returns.  The call may block on copying its own tables (the item
 * table and the index lists go through a pinned buffer the session owns); the kernels are asynchronous on
 * `stream`, under the cross-stream rule of rt_render_async.
 * A map in which every pixel has the same done_p and the same target IS rt_progressive_extend_async (same
 * kernels, same stats).  Any other map runs one launch of the item-table kernel over the items of
 * rt_progressive_map_plan, then one reduction launch per distinct target (at most 256 distinct targets when an
 * output is given: more is RT_ERR_UNSUPPORTED; a trace-only call has no such limit).
 * RT_ERR_INVALID: no session open, spp_target NULL, a target below done_p or above spp_capacity, a target of 0 with
 * an output.  With both outputs NULL a target of 0 leaves that pixel untouched.
 * After a non-uniform map, rt_progressive_extend_async(ctx, n) is RT_ERR_INVALID for n < max done_p and otherwise
 * traces [done_p, n) of each pixel.
 * rt_context_collect after it: output pixel p and the return code (RT_ERR_RANGE included) are those of
 * rt_render_async at spp = spp_target[p].  samples and ray_segments count what was traced since the last collect
 * (over a session they sum to the unsplit renders' at each pixel's count), bounce_iters gets a pixel's K once per
 * reduction of that pixel, pixels the pixel count once per call that enqueued work; RT_KERNEL_SPLIT is set, and
 * RT_KERNEL_ITEMS when the item-table kernel ran. */
int rt_progressive_extend_map_async(rt_context* ctx, const uint32_t* spp_target, void* d_rgb8, void* d_linear,
                                    void* stream);
/* The reduction alone, at any earlier counts: 1 <= spp_count[p] <= done_p (HOST array; NULL = every pixel's
 * done_p).  Traces nothing: samples and ray_segments are 0 at the collect.
 * RT_ERR_INVALID: no session open, both outputs NULL, a count of 0 or above done_p; RT_ERR_UNSUPPORTED: more than
 * 256 distinct counts. */
int rt_progressive_snapshot_map_async(rt_context* ctx, const uint32_t* spp_count, void* d_rgb8, void* d_linear,
                                      void* stream);
/* done_p of every pixel into `out` (host).  Synchronous, no GPU work.  RT_ERR_INVALID: no session, out NULL. */
int rt_progressive_counts(rt_context* ctx, uint32_t* out);
/* The half-buffer error estimate, one double per pixel into d_error (device):
 *   err_p = max over channels of |linear_c at done_p samples - linear_c at done_p / 2 samples| (integer division),
 * both the session's own linear snapshots, subtracted in double; +inf where done_p < 2.  Runs the two snapshots
 * into buffers the session owns (48 bytes per pixel), then an element-wise kernel.  Its two reductions count in
 * bounce_iters like any other (a pixel's K at done_p / 2 and at done_p), and `pixels` gets the pixel count once.
 * RT_ERR_INVALID: no session open, d_error NULL; RT_ERR_UNSUPPORTED: more than 256 distinct counts. */
int rt_progressive_error_async(rt_context* ctx, void* d_error, void* stream);
/* Host only, needs no GPU: the item list rt_progressive_extend_map_async makes for a map.  With A the pixels that
 * have target > done and mean = ceil(sum (target - done) / A), samples_per_item is rt_split_plan(A, mean,
 * resident_waves)'s S (0 when A == 0).  Where S is a multiple of 128, pixel p's items are
 * [max(done_p, base_p + j S), min(target_p, base_p + (j + 1) S)) with base_p = done_p rounded down to 128, so no two
 * items share a 128-byte line of a pixel's termination-bounce array; any other S makes each active pixel one item
 * [done_p, target_p).  Items are in pixel order, a pixel's items adjacent.
 * items: NULL (count only), or room for items_capacity records of 4 words {pixel, first, end, 0}.
 * RT_ERR_INVALID: a NULL array or output, no pixels, a target below done, items given with items_capacity below
 * *n_items (which is set); RT_ERR_UNSUPPORTED: a target above 2^20, more than 0x7FFFFFFF pixels or items. */
int rt_progressive_map_plan(uint64_t n_pixels, const uint32_t* done, const uint32_t* target, uint32_t resident_waves,
                            uint32_t* samples_per_item, uint64_t* n_items, uint32_t* items, uint64_t items_capacity);

/* ---- refinement planned on the device: the doubling policy without per-pixel host work ----
 * One step of the policy "double the pixels whose estimate is above the tolerance": with err_p the estimate of
 * rt_progressive_error_async, active = (err_p > tolerance) and (done_p < spp_max), and the active pixels go to
 * min(2 done_p, spp_max).  A run is the calls from the first one until it returns *n_active == 0; a session
 * carries one run.  The counts, the linear values the estimate compares, the selection, the lists and the item
 * table stay on the device; no step uploads a per-pixel or per-item table.  The counts and the image of a run are
 * exactly those of the same policy driven from the host with rt_progressive_error_async and
 * rt_progressive_extend_map_async.
 *   First call: the session must be uniform at n0 >= 1 samples.  The whole frame is reduced at n0 and, if
 *     n0 >= 2, at n0 / 2, into buffers the session owns (2 x 24 bytes per pixel; the lists and counts take
 *     another 17).
 *   Later calls: the candidates are the pixels the previous call traced, all at one count n_k.  At n_k == spp_max
 *     they are finished (*n_active = 0, nothing runs).  Otherwise they alone are reduced once, at n_k; their value
 *     at n_k / 2 is the one kept from the step before.
 * The selection runs in kernels (estimate and flag, block counts, a scan of the block counts, a scatter, each a
 * launch of its own), then the call copies ONE 16-byte record down through the session's pinned buffer and waits
 * for it: the number of active pixels.  That wait is the only host synchronisation of a step, and the reason
 * the call has no _async suffix.  From that number the host plans as rt_progressive_map_plan does (its mean is
 * exact here), a kernel expands the active list into the item table, and the item-table kernel traces
 * [n_k, min(2 n_k, spp_max)) of the active pixels asynchronously on `stream`, under the cross-stream rule of
 * rt_render_async.  *n_active: the pixels selected; *n_samples: the samples enqueued; *n_active == 0: converged,
 * nothing traced.  A NaN estimate is not active.
 * rt_context_collect after it: samples and ray_segments count what was traced (over a run they sum to the counts'
 * total above n0), pixels gets the pixel count once per call that enqueued work, RT_KERNEL_SPLIT and
 * RT_KERNEL_ITEMS are set by a step that traced.  bounce_iters gets a pixel's K once per reduction of that pixel:
 * far fewer than on the host-driven path, which reduces every pixel twice per estimate.  kernel_ms spans the
 * readback's wait.
 * With the other calls: during a run the device counts are the session's; rt_progressive_counts and every map,
 * extend or error call first copy them down (4 bytes per pixel), then do what they always do.
 * rt_progressive_snapshot_map_async(ctx, NULL, ...) during or after a run reduces each class the run built from
 * its device list (one launch per count, no host pass, no upload), with the outputs and the return code of the
 * host path.  A call that traces into the session (an extend or a map with new samples) ends the run's claim on
 * the counts: a later rt_progressive_refine is RT_ERR_UNSUPPORTED.
 * RT_ERR_INVALID: no session open, a NULL output, a NaN tolerance, spp_max above spp_capacity or below the current
 * count, a session without samples, tolerance or spp_max differing from the run's first call;
 * RT_ERR_UNSUPPORTED: a run started on a non-uniform session, a call after another call has traced into the
 * session (see above), more than 0x7FFFFFFF work items in a step.  Out of scope: any policy but doubling and any
 * non-uniform start; rt_progressive_extend_map_async takes every map. */
int rt_progressive_refine(rt_context* ctx, double tolerance, uint32_t spp_max, void* stream, uint64_t* n_active,
                          uint64_t* n_samples);
/* Diagnostic: the item table the last rt_progressive_refine step built on the device ({pixel, first, end, 0}
 * records), copied to the host; items, items_capacity and n_items as in rt_progressive_map_plan.  A step that
 * selected nothing (or no step yet) has no items and samples_per_item 0.  Synchronises the session's stream.
 * RT_ERR_INVALID: no session open, a NULL output, items given with items_capacity below *n_items (which is set). */
int rt_progressive_refine_items(rt_context* ctx, uint32_t* samples_per_item, uint64_t* n_items, uint32_t* items,
                                uint64_t items_capacity);

/* Close the session: synchronises the stream of its last extend and frees the record buffer.
 * RT_ERR_INVALID: no session open.  rt_context_destroy ends an open session. */
int rt_progressive_end(rt_context* ctx);

/* RenderStat (renderer.rs:11-34) for the renders since the last call.
 * Synchronise `stream` (NULL = null stream), then report and reset the counters accumulated by the renders
 * enqueued since the last call (ray_segments, work counters, error flag).  kernel_ms = device time
 * between the first and last enqueued render (HIP events on that stream); pixels_per_second =
 * pixels / kernel_ms (the per-shard px/s the reference prints per tile, renderer.rs:339);
 * seconds = 0 (rt_render fills in its wall time). */
int rt_context_collect(rt_context* ctx, void* stream, rt_stats* stats);
/* Device memory helpers (so hosts without a HIP toolchain can drive the async API); no reference
 * counterpart (the reference has no device memory). */
int rt_device_alloc(rt_context* ctx, size_t bytes, void** out);
int rt_device_free(rt_context* ctx, void* ptr);
int rt_memcpy_d2h(rt_context* ctx, void* dst, const void* src, size_t bytes);   /* synchronises the device */
int rt_memcpy_h2d(rt_context* ctx, void* dst, const void* src, size_t bytes);   /* host to device (a query's rays);
                                                                                    returns when the copy is done */

/* Last error message of the calling thread ("" if none). */
const char* rt_last_error(void);
/* Build/version string: "rt_mi355x <version> gfx950 <product|experiment> src=<source hash>". */
const char* rt_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RT_MI355X_H */
