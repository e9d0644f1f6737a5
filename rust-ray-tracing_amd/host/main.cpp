// rt-render — the reference's binary (src/main.rs:27-74) on the MI355X sample loop.
//
//   rt-render [--scene scene.toml] [--width 3840] [--height 2160] [--spp 100] [--bounces 50]
//             [--seed 0x5EED0001] [--f32] [--root2] [--mode vectorized2|vectorized|vectorized3|scalar]
//             [--out output.png|.ppm] [--block-size B] [--sample-parallel] [--progressive n1,n2,...]
//             [--adaptive TOL --spp-min N [--count-map counts.png|.ppm] [--device-plan]] [--guides] [--dump-scene]
//             [--pick COL,ROW]... [--look-from X,Y,Z] [--look-at X,Y,Z] [--up X,Y,Z]
//             [--projection ortho|equirect|fisheye [--proj-angle DEG] [--proj-extent E] [--aa G]]
//
// --mode picks which of the reference's renderers is reproduced (include/rt_mi355x.h): the live
// render_vectorized2 (default), render_vectorized, or the scalar render.
// --sample-parallel deals each pixel's samples to several waves where a launch has fewer pixels than the chip
// has waves (rt_render_split_async's own plan; small frames at a high spp; the live path only, same image).
// --progressive n1,n2,... renders in one progressive session (rt_progressive_*): after each count (strictly
// increasing, all below --spp) it writes <out stem>_spp<count, 7 digits><ext> and prints one line with the
// count, the kernel time so far and the sample rate; only the new samples of a step are traced.  At --spp it
// writes --out, byte for byte the file the same command writes without --progressive.  The live path only.
// --adaptive TOL --spp-min N samples adaptively in one progressive session (rt_progressive_extend_map_async):
// every pixel gets N samples, then the pixels whose error estimate (the largest channel difference between the
// pixel at its count and at half its count) is above TOL double their count, up to --spp, until none is left.
// It prints per step the active pixels and the samples traced, and at the end the total and its share of
// pixels x spp.  --count-map PATH writes each pixel's count as grey RGB8, 255 * count / spp.  The live path only.
// --device-plan (with --adaptive) keeps the estimate, the selection and the item table on the GPU
// (rt_progressive_refine): the same lines, the same files, a few words between host and device per step.
// --guides also writes the guide buffers a denoiser wants beside the image (rt_render_guides_async): <out stem>_albedo.pfm,
// _normal.pfm, _depth.pfm and _coverage.pfm next to --out, the exact float32 values (PFM: "PF" three channels, "Pf"
// one, scale -1.0, little-endian, rows bottom to top).  They are always the uniform guides at --spp, from the
// primary rays of the image at --spp, whatever way the image itself was sampled; --out is the file the command
// writes without --guides.  One line gives the guide pass's kernel time and sample rate.  The live path only.
//
// --pick COL,ROW (repeatable) renders nothing and writes no file: it asks what lies under the centre of each of those
// pixels of the --width x --height frame (rt_query_hits_async: the ray from the camera centre through the pixel
// centre, quirk Q1 off so that a camera inside a sphere picks it, in fp64 or with --f32 in fp32) and prints one line
// per pick: "Pick (COL, ROW): sphere I KIND t T point [X, Y, Z] normal [X, Y, Z] front F" or "Pick (COL, ROW): miss",
// the numbers with enough digits to round-trip.  --mode vectorized2 only, and not with an option that says how or
// where an image is rendered (--out, --block-size, --sample-parallel, --progressive, --adaptive, --guides): each is
// refused.  --root2 is what a pick does anyway and is accepted; --spp, --bounces and --seed have no effect.
//
// --projection ortho|equirect|fisheye renders the frame through a camera model the reference lacks: the rays come
// from rt_camera_rays (orthographic: parallel rays over a plane --proj-extent world units high, default 10; equirect:
// a 360 x 180 degree panorama; fisheye: equidistant, --proj-angle degrees across the shorter side, default 180, black
// outside the image circle), G x G of them per pixel on a regular sub-pixel grid (--aa G, default 1; needs --spp >=
// G^2), are uploaded and path-traced in full by rt_render_rays_async; --out is written as ever.  --f32 and --root2
// are allowed.  Refused, each with a message, together with --mode, --block-size, --sample-parallel, --progressive,
// --adaptive, --guides or --pick.  --look-from, --look-at and --up (each X,Y,Z) place the camera, the perspective
// one too; their defaults are main.rs's.
//
// Defaults are main.rs's hard-coded values (scene.toml in the working directory, 3840x2160, 50
// bounces, 100 spp, camera from (16,2,18.5) looking at the origin, vfov 30, focal 10, no defocus,
// output.png).  --dump-scene prints the flattened scene as JSON and exits (no GPU needed).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "image.hpp"
#include "scene.hpp"

using namespace rt_host;

// Rust's `{}` for f64: the shortest representation that round-trips.
static std::string rs(double v) {
    if (v == std::floor(v) && std::fabs(v) < 1e15) {
        std::ostringstream o;
        o << (long long)v;
        if (v == 0 && std::signbit(v)) return "-0";
        return o.str();
    }
    for (int p = 1; p <= 17; ++p) {
        char buf[64];
        std::snprintf(buf, sizeof buf, "%.*g", p, v);
        if (std::strtod(buf, nullptr) == v) {
            std::string s(buf);
            if (s.find('e') == std::string::npos) return s;
            std::snprintf(buf, sizeof buf, "%.17f", v);   // Rust never prints exponents for {}
            s = buf;
            while (!s.empty() && s.back() == '0') s.pop_back();
            return s;
        }
    }
    return std::to_string(v);
}
static std::string rs3(const double* v) { return "[" + rs(v[0]) + ", " + rs(v[1]) + ", " + rs(v[2]) + "]"; }

static void dump_scene(const Scene& sc) {
    FlatScene f = sc.flatten();
    std::printf("{\"n_spheres\": %zu, \"center\": [", f.radius.size());
    for (size_t i = 0; i < f.center.size(); ++i) std::printf("%s%.17g", i ? ", " : "", f.center[i]);
    std::printf("], \"radius\": [");
    for (size_t i = 0; i < f.radius.size(); ++i) std::printf("%s%.17g", i ? ", " : "", f.radius[i]);
    std::printf("], \"material\": [");
    for (size_t i = 0; i < f.material.size(); ++i) std::printf("%s%u", i ? ", " : "", f.material[i]);
    std::printf("], \"materials\": [");
    for (size_t i = 0; i < f.materials.size(); ++i) {
        const rt_material& m = f.materials[i];
        std::printf("%s{\"kind\": %u, \"hollow\": %u, \"albedo\": [%.17g, %.17g, %.17g], \"fuzz\": %.17g, \"ior\": %.17g}",
                    i ? ", " : "", m.kind, m.hollow, m.albedo[0], m.albedo[1], m.albedo[2], m.fuzz, m.ior);
    }
    std::printf("]}\n");
}

int main(int argc, char** argv) {
    std::string scene_path = "scene.toml", out = "output.png";
    uint32_t width = 3840, height = 2160, spp = 100, bounces = 50, flags = 0, block_size = 0;
    uint64_t seed = 0x5EED0001ull;
    bool dump = false, sample_parallel = false, guides = false, out_given = false;
    std::vector<std::pair<uint32_t, uint32_t>> picks;   // --pick: (col, row)
    std::string progressive_arg, count_map;
    bool progressive = false, adaptive = false, device_plan = false;
    double tolerance = 0.0;
    uint32_t spp_min = 0;
    std::string projection;   // --projection: "", ortho, equirect or fisheye
    double proj_angle = 180.0, proj_extent = 10.0;
    uint32_t aa = 1;
    bool proj_opts = false, mode_given = false;
    double look_from[3] = {16.0, 2.0, 18.5}, look_at[3] = {0.0, 0.0, 0.0}, up[3] = {0.0, 1.0, 0.0};   // main.rs:51-58
    auto vec3_arg = [](const std::string& name, const std::string& v, double out[3]) {
        std::stringstream vs(v);
        std::string tok;
        int k = 0;
        while (std::getline(vs, tok, ',')) {
            char* end = nullptr;
            const double x = std::strtod(tok.c_str(), &end);
            if (tok.empty() || *end != '\0' || k == 3) { k = -1; break; }
            out[k++] = x;
        }
        if (k != 3 || v.back() == ',') { std::fprintf(stderr, "%s: '%s' is not X,Y,Z\n", name.c_str(), v.c_str()); std::exit(2); }
    };
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> std::string {
            if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", a.c_str()); std::exit(2); }
            return argv[++i];
        };
        if (a == "--scene") scene_path = next();
        else if (a == "--width") width = (uint32_t)std::stoul(next());
        else if (a == "--height") height = (uint32_t)std::stoul(next());
        else if (a == "--spp") spp = (uint32_t)std::stoul(next());
        else if (a == "--bounces") bounces = (uint32_t)std::stoul(next());
        else if (a == "--seed") seed = std::stoull(next(), nullptr, 0);
        else if (a == "--f32") flags |= RT_FLAG_F32;
        else if (a == "--root2") flags |= RT_FLAG_ROOT2;
        else if (a == "--mode") {
            const std::string m = next();
            flags &= ~(RT_FLAG_MODE_VECTORIZED | RT_FLAG_MODE_SCALAR | RT_FLAG_MODE_VECTORIZED3);
            if (m == "vectorized") flags |= RT_FLAG_MODE_VECTORIZED;
            else if (m == "vectorized3") flags |= RT_FLAG_MODE_VECTORIZED3;
            else if (m == "scalar") flags |= RT_FLAG_MODE_SCALAR;
            else if (m != "vectorized2") { std::fprintf(stderr, "unknown mode %s\n", m.c_str()); return 2; }
            mode_given = true;
        }
        else if (a == "--look-from") vec3_arg(a, next(), look_from);
        else if (a == "--look-at") vec3_arg(a, next(), look_at);
        else if (a == "--up") vec3_arg(a, next(), up);
        else if (a == "--projection") projection = next();
        else if (a == "--proj-angle") { proj_angle = std::stod(next()); proj_opts = true; }
        else if (a == "--proj-extent") { proj_extent = std::stod(next()); proj_opts = true; }
        else if (a == "--aa") { aa = (uint32_t)std::stoul(next()); proj_opts = true; }
        else if (a == "--out") { out = next(); out_given = true; }
        else if (a == "--block-size") block_size = (uint32_t)std::stoul(next());
        else if (a == "--sample-parallel") sample_parallel = true;
        else if (a == "--progressive") { progressive_arg = next(); progressive = true; }
        else if (a == "--adaptive") { tolerance = std::stod(next()); adaptive = true; }
        else if (a == "--spp-min") spp_min = (uint32_t)std::stoul(next());
        else if (a == "--count-map") count_map = next();
        else if (a == "--device-plan") device_plan = true;
        else if (a == "--guides") guides = true;
        else if (a == "--pick") {
            const std::string v = next();
            const size_t comma = v.find(',');
            auto digits = [](const std::string& t) {
                return !t.empty() && t.size() <= 9 && t.find_first_not_of("0123456789") == std::string::npos;
            };
            if (comma == std::string::npos || !digits(v.substr(0, comma)) || !digits(v.substr(comma + 1))) {
                std::fprintf(stderr, "--pick: '%s' is not COL,ROW\n", v.c_str());
                return 2;
            }
            picks.emplace_back((uint32_t)std::stoul(v.substr(0, comma)), (uint32_t)std::stoul(v.substr(comma + 1)));
        }
        else if (a == "--dump-scene") dump = true;
        else if (a == "-h" || a == "--help") {
            std::puts("rt-render [--scene scene.toml] [--width W] [--height H] [--spp S] [--bounces B] [--seed N] "
                      "[--f32] [--root2] [--mode vectorized2|vectorized|vectorized3|scalar] [--out output.png] [--block-size B] "
                      "[--sample-parallel] [--progressive n1,n2,...] [--adaptive TOL --spp-min N [--count-map PATH] "
                      "[--device-plan]] [--guides] [--dump-scene] [--pick COL,ROW]... [--look-from X,Y,Z] [--look-at X,Y,Z] "
                      "[--up X,Y,Z] [--projection ortho|equirect|fisheye [--proj-angle DEG] [--proj-extent E] [--aa G]]");
            return 0;
        } else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
    }
    std::vector<uint32_t> counts;   // --progressive: the sample counts before --spp
    if (progressive) {
        auto bad = [](const std::string& why) {
            std::fprintf(stderr, "--progressive: %s\n", why.c_str());
            return 2;
        };
        if (flags & RT_FLAG_ROOT2)
            return bad("not with --root2: a session keeps per-sample records, which only the live path's kernels write "
                       "(the --root2 kernels reduce a pixel inside the wave)");
        if (flags & (RT_FLAG_MODE_VECTORIZED | RT_FLAG_MODE_SCALAR | RT_FLAG_MODE_VECTORIZED3))
            return bad("only with --mode vectorized2: a session keeps per-sample records, which only the live path's "
                       "kernels write (the other modes reduce a pixel inside the wave)");
        if (block_size != 0) return bad("not with --block-size: every step is one launch over the whole image");
        std::stringstream ps(progressive_arg);
        std::string tok;
        while (std::getline(ps, tok, ',')) {
            if (tok.empty() || tok.find_first_not_of("0123456789") != std::string::npos || tok.size() > 9)
                return bad("'" + tok + "' is not a sample count (expected n1,n2,...)");
            const uint32_t n = (uint32_t)std::stoul(tok);
            if (n == 0) return bad("a sample count of 0");
            if (!counts.empty() && n <= counts.back()) return bad("the counts must be strictly increasing");
            if (n >= spp) return bad("the counts must be below --spp (" + std::to_string(spp) + "), where --out is written");
            counts.push_back(n);
        }
        if (counts.empty() || progressive_arg.back() == ',') return bad("expected n1,n2,...");
    }
    if (adaptive) {
        auto bad = [](const std::string& why) {
            std::fprintf(stderr, "--adaptive: %s\n", why.c_str());
            return 2;
        };
        if (flags & RT_FLAG_ROOT2) return bad("not with --root2: a session's records are the live path's");
        if (flags & (RT_FLAG_MODE_VECTORIZED | RT_FLAG_MODE_SCALAR | RT_FLAG_MODE_VECTORIZED3))
            return bad("only with --mode vectorized2: a session's records are the live path's");
        if (block_size != 0) return bad("not with --block-size: every step is one launch over the whole image");
        if (progressive) return bad("not with --progressive: the error estimate picks the counts");
        if (tolerance != tolerance) return bad("the tolerance is NaN");
        if (spp_min < 1 || spp_min > spp)
            return bad("--spp-min must be between 1 and --spp (" + std::to_string(spp) + "), the most a pixel gets");
    } else if (spp_min != 0 || !count_map.empty() || device_plan) {
        std::fprintf(stderr, "--spp-min, --count-map and --device-plan go with --adaptive\n");
        return 2;
    }
    if (guides) {
        auto bad = [](const std::string& why) {
            std::fprintf(stderr, "--guides: %s\n", why.c_str());
            return 2;
        };
        if (flags & RT_FLAG_ROOT2) return bad("not with --root2: the guides are the live path's first hits");
        if (flags & (RT_FLAG_MODE_VECTORIZED | RT_FLAG_MODE_SCALAR | RT_FLAG_MODE_VECTORIZED3))
            return bad("only with --mode vectorized2: the guides are the live path's first hits");
        if (block_size != 0) return bad("not with --block-size: the guide pass is one launch over the whole image");
    }
    if (!picks.empty()) {
        auto bad = [](const std::string& why) {
            std::fprintf(stderr, "--pick: %s\n", why.c_str());
            return 2;
        };
        if (flags & (RT_FLAG_MODE_VECTORIZED | RT_FLAG_MODE_SCALAR | RT_FLAG_MODE_VECTORIZED3))
            return bad("only with --mode vectorized2: a query is the live path's closest hit");
        if (progressive || adaptive || guides || sample_parallel || block_size != 0 || out_given)
            return bad("not with --out, --block-size, --sample-parallel, --progressive, --adaptive or --guides: nothing is "
                       "rendered and no file is written");
        for (const auto& p : picks)
            if (p.first >= width || p.second >= height)
                return bad("(" + std::to_string(p.first) + ", " + std::to_string(p.second) + ") is outside the " +
                           std::to_string(width) + " x " + std::to_string(height) + " frame");
    }
    uint32_t proj_model = 0;
    if (!projection.empty()) {
        auto bad = [](const std::string& why) {
            std::fprintf(stderr, "--projection: %s\n", why.c_str());
            return 2;
        };
        if (projection == "ortho") proj_model = RT_PROJ_ORTHOGRAPHIC;
        else if (projection == "equirect") proj_model = RT_PROJ_EQUIRECT;
        else if (projection == "fisheye") proj_model = RT_PROJ_FISHEYE;
        else return bad("unknown projection '" + projection + "' (ortho, equirect or fisheye)");
        if (mode_given) return bad("not with --mode: caller rays are path-traced on the live path only");
        if (block_size != 0) return bad("not with --block-size: the frame's rays are rendered in one launch");
        if (sample_parallel) return bad("not with --sample-parallel: caller rays have no sample-parallel kernels");
        if (progressive) return bad("not with --progressive: a session traces the perspective camera's rays");
        if (adaptive) return bad("not with --adaptive: a session traces the perspective camera's rays");
        if (guides) return bad("not with --guides: the guide buffers are the perspective camera's first hits");
        if (!picks.empty()) return bad("not with --pick: a pick goes through the perspective camera's pixel centres");
        if (aa == 0 || aa > 1024) return bad("--aa must be between 1 and 1024");
        if ((uint64_t)aa * aa > spp)
            return bad("--aa " + std::to_string(aa) + " needs --spp >= " + std::to_string((uint64_t)aa * aa) +
                       " (one sample per ray of the pixel's grid at least)");
    } else if (proj_opts) {
        std::fprintf(stderr, "--proj-angle, --proj-extent and --aa go with --projection\n");
        return 2;
    }
    try {
        std::ifstream in(scene_path, std::ios::binary);   // main.rs:31-34
        if (!in) throw Panic("Can't read scene from file " + scene_path);
        std::stringstream ss;
        ss << in.rdbuf();
        Scene scene;
        try {
            scene = scene_from_toml(ss.str());
        } catch (const toml::ParseError& e) {
            throw Panic("Failed parsing scene from file " + scene_path + ": " + e.what());   // main.rs:36-39
        }
        if (dump) { dump_scene(scene); return 0; }

        const double* from = look_from;   // main.rs:51-58 unless --look-from, --look-at or --up say otherwise
        Camera camera(width, height, 10.0, 30.0, Vec3{look_from[0], look_from[1], look_from[2]},
                      Vec3{look_at[0], look_at[1], look_at[2]}, Vec3{up[0], up[1], up[2]}, 0.0);
        const double vh = std::tan((30.0 * (3.141592653589793 / 180.0)) / 2.0) * 10.0 * 2.0;   // ray_tracing.rs:29
        std::printf("Parameters:\n");                                                          // ray_tracing.rs:46-50
        std::printf("\tCamera Center:            %s\n", rs3(from).c_str());
        std::printf("\tViewport Height:          %s\n", rs(vh).c_str());
        std::printf("\tViewport Width:           %s\n", rs(vh * ((double)width / (double)height)).c_str());
        std::printf("\tViewport Top Left Corner: %s\n", rs3(camera.c.ulc).c_str());
        std::printf("\t Number of objects: \t %zu\n", scene.len());                           // main.rs:60

        GpuRenderer renderer(seed, flags, block_size, sample_parallel);   // block_size 128: TileRenderer::new(None, 128), main.rs:62
        if (!picks.empty()) {
            static const char* const kinds[3] = {"lambertian", "metal", "dielectric"};
            const int digits = (flags & RT_FLAG_F32) ? 9 : 17;
            for (const GpuRenderer::Pick& p : renderer.pick(picks, scene, camera)) {
                if (p.index < 0) {
                    std::printf("Pick (%u, %u): %s\n", p.col, p.row, p.index == RT_QUERY_MISS ? "miss" : "invalid");
                    continue;
                }
                std::printf("Pick (%u, %u): sphere %d %s t %.*g point [%.*g, %.*g, %.*g] normal [%.*g, %.*g, %.*g] front %d\n",
                            p.col, p.row, p.index, kinds[p.kind < 3 ? p.kind : 0], digits, p.t, digits, p.point[0], digits,
                            p.point[1], digits, p.point[2], digits, p.normal[0], digits, p.normal[1], digits, p.normal[2],
                            p.front ? 1 : 0);
            }
            return 0;
        }
        std::fprintf(stderr, "Rendering %u by %u image on %s (%s)...\n", width, height, rt_version(),
                     (flags & RT_FLAG_F32) ? "fp32" : "fp64");
        auto step = [&](uint32_t n, const RgbImage& im, const rt_stats& so_far, bool range_err) {
            const size_t dot = out.find_last_of('.'), slash = out.find_last_of('/');
            const bool ext = dot != std::string::npos && (slash == std::string::npos || dot > slash);
            char tag[32];
            std::snprintf(tag, sizeof tag, "_spp%07u", n);
            const std::string path = (ext ? out.substr(0, dot) : out) + tag + (ext ? out.substr(dot) : "");
            save_image(path, im.width, im.height, im.data.data());
            std::printf("Progressive: %u spp -> %s, kernel %.3f ms, %.2f Msamples/s%s\n", n, path.c_str(), so_far.kernel_ms,
                        so_far.kernel_ms > 0 ? (double)so_far.samples / (so_far.kernel_ms * 1e-3) / 1e6 : 0.0,
                        range_err ? " (a pixel channel exceeded 2.0 at this count)" : "");
            std::fflush(stdout);
        };
        std::vector<uint32_t> pixel_counts;   // --adaptive: the samples each pixel got
        uint32_t steps = 0;
        auto adaptive_step = [&](size_t active, uint64_t traced) {
            std::printf("Adaptive: step %u, %zu active pixels, %llu samples traced\n", ++steps, active,
                        (unsigned long long)traced);
            std::fflush(stdout);
        };
        rt_projection proj{};
        proj.model = proj_model;
        proj.image_width = width;
        proj.image_height = height;
        for (int k = 0; k < 3; ++k) { proj.center[k] = look_from[k]; proj.look_at[k] = look_at[k]; proj.up[k] = up[k]; }
        proj.angle_deg = proj_angle;
        proj.extent = proj_extent;
        auto [image, stat] = !projection.empty() ? renderer.render_projection(bounces, spp, scene, proj, aa)
                             : adaptive ? renderer.render_adaptive(bounces, spp_min, spp, tolerance, scene, camera,
                                                                 pixel_counts, adaptive_step, device_plan)
                             : progressive ? renderer.render_progressive(bounces, spp, scene, camera, counts, step)
                                           : renderer.render(bounces, spp, scene, camera);     // main.rs:64
        save_image(out, image.width, image.height, image.data.data());                         // main.rs:66
        if (guides) {
            const GpuRenderer::Guides g = renderer.render_guides(spp, scene, camera);
            const size_t dot = out.find_last_of('.'), slash = out.find_last_of('/');
            const bool ext = dot != std::string::npos && (slash == std::string::npos || dot > slash);
            const std::string stem = ext ? out.substr(0, dot) : out;
            write_pfm(stem + "_albedo.pfm", g.width, g.height, 3, g.albedo.data());
            write_pfm(stem + "_normal.pfm", g.width, g.height, 3, g.normal.data());
            write_pfm(stem + "_depth.pfm", g.width, g.height, 1, g.depth.data());
            write_pfm(stem + "_coverage.pfm", g.width, g.height, 1, g.coverage.data());
            std::printf("Guides: %u spp -> %s_{albedo,normal,depth,coverage}.pfm, kernel %.3f ms, %.2f Msamples/s\n", spp,
                        stem.c_str(), g.gpu.kernel_ms,
                        g.gpu.kernel_ms > 0 ? (double)g.gpu.samples / (g.gpu.kernel_ms * 1e-3) / 1e6 : 0.0);
        }
        if (adaptive) {
            const double full = (double)image.width * image.height * spp;
            std::printf("Adaptive: %u steps, %llu samples traced, %.1f %% of %u x %u x %u spp\n", steps,
                        (unsigned long long)stat.gpu.samples, 100.0 * (double)stat.gpu.samples / full, image.width,
                        image.height, spp);
            if (!count_map.empty()) {
                std::vector<uint8_t> grey(pixel_counts.size() * 3);
                for (size_t p = 0; p < pixel_counts.size(); ++p)
                    grey[3 * p] = grey[3 * p + 1] = grey[3 * p + 2] = (uint8_t)(255ull * pixel_counts[p] / spp);
                save_image(count_map, image.width, image.height, grey.data());
            }
        }
        std::printf("Image Size: %u x %u\n", camera.image_width(), camera.image_height());    // main.rs:68-71
        std::printf("Total Pixels: %zu\n", stat.pixels_rendered);
        std::printf("Time Taken: %.3f seconds\n", stat.duration.count());
        std::printf("Average Pixel Rate: %.2f px/s\n", stat.pixels_per_second);
        std::printf("Sample Rate: %.2f Msamples/s (kernel %.3f ms, %llu ray segments)\n",
                    (double)stat.gpu.samples / stat.duration.count() / 1e6, stat.gpu.kernel_ms,
                    (unsigned long long)stat.gpu.ray_segments);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "thread 'main' panicked: %s\n", e.what());
        return 101;   // Rust's panic exit status
    }
    return 0;
}
