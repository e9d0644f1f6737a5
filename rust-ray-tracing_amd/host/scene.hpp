// scene.hpp — C++ host mirror of the reference's host-side surface, above the C ABI:
//   Vec3/Color::from_toml, toml_utils::to_float        src/geometry.rs:190-211, src/color.rs:99-123,
//                                                       src/toml_utils.rs:2-12
//   Material (Lambertian / Metal / Dielectric)          src/materials.rs:12-155
//   Object::Sphere, get_object_list                     src/objects.rs:17-52, 203-300
//   Scene, Camera::new                                  src/ray_tracing.rs:27-62, 100-104, 217-229
//   Renderer, RenderStat                                src/renderer.rs:11-40
// Where the reference panics (unwrap / panic! / Index on a missing key), these throw rt_host::Panic
// with the reference's message.
#pragma once
#include <algorithm>
#include <cctype>
#include <chrono>
#include <cstring>
#include <map>
#include <memory>
#include <optional>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rt_mi355x.h"
#include "toml.hpp"

namespace rt_host {

struct Panic : std::runtime_error {
    using std::runtime_error::runtime_error;
};

inline const toml::Value& index(const toml::Table& t, const std::string& k) {   // Index<&str> for Map
    auto it = t.find(k);
    if (it == t.end()) throw Panic("index not found: key \"" + k + "\" missing from table");
    return it->second;
}
template <typename T> T unwrap(const std::optional<T>& o, const char* what) {
    if (!o) throw Panic(std::string("called `Option::unwrap()` on a `None` value (") + what + ")");
    return *o;
}
inline std::string lower(std::string s) {
    for (auto& c : s) c = (char)std::tolower((unsigned char)c);
    return s;
}

// toml_utils.rs:2-12
inline std::optional<double> to_float(const toml::Value& v) {
    if (v.is_float()) return v.f;
    if (v.is_int()) return (double)v.i;
    return std::nullopt;
}

struct Vec3 {
    double x = 0, y = 0, z = 0;
    // geometry.rs:190-211
    static std::optional<Vec3> from_toml(const toml::Value& v) {
        if (auto* t = v.as_table())
            return Vec3{unwrap(to_float(index(*t, "x")), "x"), unwrap(to_float(index(*t, "y")), "y"),
                        unwrap(to_float(index(*t, "z")), "z")};
        if (auto* a = v.as_array()) {
            if (a->size() < 3) throw Panic("assertion failed: array.len() >= 3");
            return Vec3{unwrap(to_float((*a)[0]), "x"), unwrap(to_float((*a)[1]), "y"), unwrap(to_float((*a)[2]), "z")};
        }
        return std::nullopt;
    }
};

struct Color {
    double red = 0, green = 0, blue = 0;
    // color.rs:99-123 (table entries that are not numbers read as 0.0; missing keys panic)
    static std::optional<Color> from_toml(const toml::Value& v) {
        if (auto* t = v.as_table())
            return Color{to_float(index(*t, "red")).value_or(0.0), to_float(index(*t, "green")).value_or(0.0),
                         to_float(index(*t, "blue")).value_or(0.0)};
        if (auto* a = v.as_array()) {
            if (a->size() < 3) throw Panic("assertion failed: array.len() >= 3");
            return Color{unwrap(to_float((*a)[0]), "red"), unwrap(to_float((*a)[1]), "green"),
                         unwrap(to_float((*a)[2]), "blue")};
        }
        return std::nullopt;
    }
};

// trait Material (materials.rs:35-39); to_rt() flattens a material for the C ABI.
struct Material {
    virtual ~Material() = default;
    virtual rt_material to_rt() const = 0;
};

struct Lambertian : Material {   // materials.rs:41-69
    Color albedo;
    explicit Lambertian(Color a) : albedo(a) {}
    rt_material to_rt() const override {
        rt_material m{};
        m.kind = RT_LAMBERTIAN;
        m.albedo[0] = albedo.red; m.albedo[1] = albedo.green; m.albedo[2] = albedo.blue;
        return m;
    }
    static std::shared_ptr<Material> from_table(const toml::Table& t) {
        return std::make_shared<Lambertian>(unwrap(Color::from_toml(index(t, "albedo")), "albedo"));
    }
};

struct Metal : Material {   // materials.rs:71-107
    Color albedo;
    double fuzzy_factor;
    Metal(Color a, double f) : albedo(a), fuzzy_factor(rt_metal_clamp_fuzz(f)) {}   // Metal::new clamp
    rt_material to_rt() const override {
        rt_material m{};
        m.kind = RT_METAL;
        m.albedo[0] = albedo.red; m.albedo[1] = albedo.green; m.albedo[2] = albedo.blue;
        m.fuzz = fuzzy_factor;
        return m;
    }
    static std::shared_ptr<Material> from_table(const toml::Table& t) {
        return std::make_shared<Metal>(unwrap(Color::from_toml(index(t, "albedo")), "albedo"),
                                       unwrap(to_float(index(t, "fuzzy_factor")), "fuzzy_factor"));
    }
};

struct Dielectric : Material {   // materials.rs:109-155
    double index_of_refraction;
    bool hollow;
    Dielectric(double ior, bool h) : index_of_refraction(ior), hollow(h) {}
    rt_material to_rt() const override {
        rt_material m{};
        m.kind = RT_DIELECTRIC;
        m.hollow = hollow ? 1u : 0u;
        m.ior = index_of_refraction;
        return m;
    }
    static std::shared_ptr<Material> from_table(const toml::Table& t) {
        const toml::Value& h = index(t, "hollow");
        if (!h.is_bool()) throw Panic("called `Option::unwrap()` on a `None` value (hollow)");
        return std::make_shared<Dielectric>(unwrap(to_float(index(t, "index_of_refraction")), "index_of_refraction"), h.b);
    }
};

using MaterialTable = std::map<std::string, std::shared_ptr<Material>>;

// materials.rs:21-33
inline std::shared_ptr<Material> load_material_from_toml(const toml::Table& t) {
    const std::string* ty = index(t, "type").as_str();
    if (!ty) throw Panic("called `Option::unwrap()` on a `None` value (type)");
    const std::string k = lower(*ty);
    if (k == "lambertian") return Lambertian::from_table(t);
    if (k == "metal") return Metal::from_table(t);
    if (k == "dielectric") return Dielectric::from_table(t);
    throw Panic("Unknown material type " + k + "!");
}

// materials.rs:12-19
inline MaterialTable get_materials(const toml::Table& t) {
    MaterialTable out;
    for (const auto& [key, value] : t) {
        const toml::Table* mt = value.as_table();
        if (!mt) throw Panic("called `Option::unwrap()` on a `None` value (material table)");
        out.emplace(key, load_material_from_toml(*mt));
    }
    return out;
}

struct Sphere {   // objects.rs:203-214, 292-299
    Vec3 center;
    double radius;
    std::shared_ptr<Material> material;
    static Sphere from_table(const toml::Table& t, const MaterialTable& mats) {
        Vec3 c = unwrap(Vec3::from_toml(index(t, "center")), "center");
        double r = unwrap(to_float(index(t, "radius")), "radius");
        const std::string* name = index(t, "material").as_str();
        if (!name) throw Panic("called `Option::unwrap()` on a `None` value (material)");
        auto it = mats.find(*name);
        if (it == mats.end()) throw Panic("called `Option::unwrap()` on a `None` value (material \"" + *name + "\")");
        return Sphere{c, r, it->second};
    }
};

// objects.rs:38-52
inline Sphere load_object_from_toml(const toml::Table& t, const MaterialTable& mats) {
    const std::string* ty = index(t, "type").as_str();
    if (!ty) throw Panic("called `Option::unwrap()` on a `None` value (type)");
    const std::string k = lower(*ty);
    if (k == "sphere") return Sphere::from_table(t, mats);
    throw Panic("Unknown object type " + k);
}
inline std::vector<Sphere> get_object_list(const toml::Array& a, const MaterialTable& mats) {
    std::vector<Sphere> out;
    for (const auto& v : a) {
        const toml::Table* t = v.as_table();
        if (!t) throw Panic("called `Option::unwrap()` on a `None` value (hitable)");
        out.push_back(load_object_from_toml(*t, mats));
    }
    return out;
}

// Owning SoA image of a Scene in the C-ABI layout (scene order kept: ties -> later sphere).
struct FlatScene {
    std::vector<double> center, radius;
    std::vector<uint32_t> material;
    std::vector<rt_material> materials;
    rt_scene view() const {
        rt_scene s{};
        s.n_spheres = (uint32_t)radius.size();
        s.n_materials = (uint32_t)materials.size();
        s.center = center.data(); s.radius = radius.data(); s.material = material.data();
        s.materials = materials.data();
        return s;
    }
};

struct Scene {   // ray_tracing.rs:100-104, 217-229, 308-310
    std::vector<Sphere> objects;
    static Scene from_list(const std::vector<Sphere>& l) { return Scene{l}; }
    void add(Sphere s) { objects.push_back(std::move(s)); }
    size_t len() const { return objects.size(); }
    FlatScene flatten() const {
        FlatScene f;
        std::map<const Material*, uint32_t> ids;
        for (const auto& s : objects) {
            auto [it, fresh] = ids.emplace(s.material.get(), (uint32_t)f.materials.size());
            if (fresh) f.materials.push_back(s.material->to_rt());
            f.center.insert(f.center.end(), {s.center.x, s.center.y, s.center.z});
            f.radius.push_back(s.radius);
            f.material.push_back(it->second);
        }
        return f;
    }
};

// src/main.rs:29-43: a scene file -> Scene
inline Scene scene_from_toml(const std::string& text) {
    toml::Value root = toml::parse(text);
    const toml::Table& r = *root.as_table();
    const toml::Table* mats = index(r, "materials").as_table();
    if (!mats) throw Panic("called `Option::unwrap()` on a `None` value (materials)");
    const toml::Array* hit = index(r, "hitables").as_array();
    if (!hit) throw Panic("called `Option::unwrap()` on a `None` value (hitables)");
    MaterialTable mt = get_materials(*mats);
    return Scene::from_list(get_object_list(*hit, mt));
}

struct Camera {   // ray_tracing.rs:27-62 via rt_camera_new
    rt_camera c{};
    Camera(uint32_t w, uint32_t h, double focal_length, double view_angle, Vec3 center, Vec3 look_at, Vec3 up,
           double defocus_angle) {
        const double ce[3] = {center.x, center.y, center.z}, la[3] = {look_at.x, look_at.y, look_at.z},
                     u[3] = {up.x, up.y, up.z};
        if (rt_camera_new(&c, w, h, focal_length, view_angle, ce, la, u, defocus_angle) != RT_OK)
            throw Panic(rt_last_error());
    }
    uint32_t image_width() const { return c.image_width; }
    uint32_t image_height() const { return c.image_height; }
};

struct RenderStat {   // renderer.rs:11-34
    std::chrono::duration<double> duration;
    size_t pixels_rendered;
    double pixels_per_second;
    rt_stats gpu;
    RenderStat(std::chrono::duration<double> d, size_t px, rt_stats g = {})
        : duration(d), pixels_rendered(px), pixels_per_second(px / d.count()), gpu(g) {}
};

struct RgbImage {
    uint32_t width = 0, height = 0;
    std::vector<uint8_t> data;   // row-major interleaved RGB8 (image::RgbImage raw layout)
};

struct Renderer {   // renderer.rs:38-40
    virtual ~Renderer() = default;
    virtual std::pair<RgbImage, RenderStat> render(size_t max_bounces, size_t samples_per_pixel, const Scene& scene,
                                                   const Camera& camera) = 0;
};

// The GPU implementation of Renderer (replaces TileRenderer, renderer.rs:232-387).
// block_size 0: the whole image in one launch (rt_render).  block_size B > 0: TileRenderer's
// decomposition (renderer.rs:248-266): B x B blocks, row-major, one launch each on one device
// context, and after each the reference's per-block line (renderer.rs:339), with the block's pixel
// rate from the launch's kernel time: "Device 0 complete block (x, y) at R px/s".  The image is the
// same either way (the RNG is keyed by the global pixel index).
// sample_parallel: every launch goes through rt_render_split_async with its own plan, which deals a pixel's
// samples to several waves where the launch has fewer pixels than the chip has waves (the live path only;
// the same image).
struct GpuRenderer : Renderer {
    uint64_t seed;
    uint32_t flags;
    uint32_t block_size;
    bool sample_parallel;
    explicit GpuRenderer(uint64_t s = 0x5EED0001ull, uint32_t f = 0, uint32_t b = 0, bool sp = false)
        : seed(s), flags(f), block_size(b), sample_parallel(sp) {}
    std::pair<RgbImage, RenderStat> render(size_t max_bounces, size_t spp, const Scene& scene,
                                           const Camera& camera) override {
        const auto t0 = std::chrono::steady_clock::now();
        FlatScene flat = scene.flatten();
        rt_scene rs = flat.view();
        RgbImage img{camera.image_width(), camera.image_height(), {}};
        img.data.resize((size_t)img.width * img.height * 3);
        rt_stats st{};
        if (block_size == 0 && sample_parallel) {   // one launch of the whole image on a device context
            render_blocks(rs, camera, (uint32_t)max_bounces, (uint32_t)spp, img, st, std::max(img.width, img.height), false);
        } else if (block_size == 0) {
            const int rc = rt_render(&rs, &camera.c, (uint32_t)max_bounces, (uint32_t)spp, seed, flags, nullptr,
                                     img.data.data(), nullptr, &st);
            if (rc == RT_ERR_RANGE) throw Panic(std::string("assertion failed: ") + rt_last_error());
            if (rc != RT_OK) throw Panic(std::string("rt_render failed: ") + rt_last_error());
        } else {
            render_blocks(rs, camera, (uint32_t)max_bounces, (uint32_t)spp, img, st, block_size, true);
        }
        const size_t npx = (size_t)img.width * img.height;
        RenderStat stat(std::chrono::steady_clock::now() - t0, npx, st);
        return {std::move(img), stat};
    }

    // Progressive render (rt_progressive_*): one session of capacity spp over the whole image, extended to
    // each of `counts` (strictly increasing, all below spp) and then to spp, an image at every step; only the
    // new samples of a step are traced, and every image is the one render() gives at that sample count.
    // step(count, image, stats so far, range error at this count) is called after each of `counts`.  A channel
    // above 2.0 at a step is reported, not thrown (at a few samples the reference's own arithmetic gets there);
    // at spp it panics as render() does.  The live path only (flags: RT_FLAG_F32 or none).
    template <typename Step>
    std::pair<RgbImage, RenderStat> render_progressive(size_t max_bounces, size_t spp, const Scene& scene,
                                                       const Camera& camera, const std::vector<uint32_t>& counts,
                                                       Step&& step) {
        const auto t0 = std::chrono::steady_clock::now();
        FlatScene flat = scene.flatten();
        rt_scene rs = flat.view();
        RgbImage img{camera.image_width(), camera.image_height(), {}};
        const size_t npx = (size_t)img.width * img.height;
        img.data.resize(npx * 3);
        struct Ctx {
            rt_context* c = nullptr;
            void* buf = nullptr;
            ~Ctx() { if (buf) rt_device_free(c, buf); if (c) rt_context_destroy(c); }   // destroy ends the session
        } x;
        auto chk = [](int rc, const char* what) {
            if (rc != RT_OK) throw Panic(std::string(what) + ": " + rt_last_error());
        };
        chk(rt_context_create(0, &x.c), "rt_context_create");
        chk(rt_context_set_scene(x.c, &rs), "rt_context_set_scene");
        chk(rt_device_alloc(x.c, npx * 3, &x.buf), "rt_device_alloc");
        chk(rt_progressive_begin(x.c, &camera.c, (uint32_t)max_bounces, (uint32_t)spp, seed, flags, nullptr, 0),
            "rt_progressive_begin");
        rt_stats total{};
        auto extend = [&](uint32_t n) -> bool {   // true: RT_ERR_RANGE at this count
            chk(rt_progressive_extend_async(x.c, n, x.buf, nullptr, nullptr), "rt_progressive_extend_async");
            rt_stats st{};
            const int rc = rt_context_collect(x.c, nullptr, &st);
            if (rc != RT_ERR_RANGE) chk(rc, "rt_context_collect");
            chk(rt_memcpy_d2h(x.c, img.data.data(), x.buf, npx * 3), "rt_memcpy_d2h");
            total.kernel_ms += st.kernel_ms;
            total.pixels = npx;
            total.samples += st.samples;
            total.ray_segments += st.ray_segments;
            total.lane_slots += st.lane_slots;
            total.bounce_iters += st.bounce_iters;
            total.kernel_id = st.kernel_id;
            total.kernel_wg_per_cu = st.kernel_wg_per_cu;
            return rc == RT_ERR_RANGE;
        };
        for (uint32_t n : counts) {
            const bool range_err = extend(n);
            step(n, img, total, range_err);
        }
        if (extend((uint32_t)spp)) throw Panic("assertion failed: a pixel channel exceeded 2.0 (color.rs:55-57)");
        chk(rt_progressive_end(x.c), "rt_progressive_end");
        RenderStat stat(std::chrono::steady_clock::now() - t0, npx, total);
        return {std::move(img), stat};
    }

    // Adaptive render (rt_progressive_extend_map_async and its kin; GpuRenderer.adaptive of the Python package,
    // step for step): a session of capacity spp, every pixel to spp_min samples, then, while some pixel's error
    // estimate (rt_progressive_error_async) is above `tolerance` and its count below spp, those pixels double
    // their count (up to spp).  Pixel p of the image is render()'s at counts[p] samples.  step(active pixels,
    // samples the step traced) is called after every refinement step.  The live path only.
    // device_plan: the steps are rt_progressive_refine's, which estimates, selects and plans on the device; the
    // counts come down once, at the end.  Same steps, same counts, same image.
    template <typename Step>
    std::pair<RgbImage, RenderStat> render_adaptive(size_t max_bounces, size_t spp_min, size_t spp, double tolerance,
                                                    const Scene& scene, const Camera& camera,
                                                    std::vector<uint32_t>& counts, Step&& step,
                                                    bool device_plan = false) {
        const auto t0 = std::chrono::steady_clock::now();
        FlatScene flat = scene.flatten();
        rt_scene rs = flat.view();
        RgbImage img{camera.image_width(), camera.image_height(), {}};
        const size_t npx = (size_t)img.width * img.height;
        img.data.resize(npx * 3);
        struct Ctx {
            rt_context* c = nullptr;
            void* buf = nullptr;
            void* err = nullptr;
            ~Ctx() {   // destroy ends the session
                if (buf) rt_device_free(c, buf);
                if (err) rt_device_free(c, err);
                if (c) rt_context_destroy(c);
            }
        } x;
        auto chk = [](int rc, const char* what) {
            if (rc != RT_OK) throw Panic(std::string(what) + ": " + rt_last_error());
        };
        chk(rt_context_create(0, &x.c), "rt_context_create");
        chk(rt_context_set_scene(x.c, &rs), "rt_context_set_scene");
        chk(rt_device_alloc(x.c, npx * 3, &x.buf), "rt_device_alloc");
        chk(rt_device_alloc(x.c, npx * sizeof(double), &x.err), "rt_device_alloc");
        chk(rt_progressive_begin(x.c, &camera.c, (uint32_t)max_bounces, (uint32_t)spp, seed, flags, nullptr, 0),
            "rt_progressive_begin");
        rt_stats total{};
        auto collect = [&]() -> bool {   // true: RT_ERR_RANGE
            rt_stats st{};
            const int rc = rt_context_collect(x.c, nullptr, &st);
            if (rc != RT_ERR_RANGE) chk(rc, "rt_context_collect");
            total.kernel_ms += st.kernel_ms;
            total.pixels = npx;
            total.samples += st.samples;
            total.ray_segments += st.ray_segments;
            total.lane_slots += st.lane_slots;
            total.bounce_iters += st.bounce_iters;
            total.kernel_id = st.kernel_id;
            total.kernel_wg_per_cu = st.kernel_wg_per_cu;
            return rc == RT_ERR_RANGE;
        };
        chk(rt_progressive_extend_async(x.c, (uint32_t)spp_min, nullptr, nullptr, nullptr), "rt_progressive_extend_async");
        (void)collect();
        counts.assign(npx, 0u);
        std::vector<double> err(npx);
        while (device_plan) {
            uint64_t active = 0, traced = 0;
            chk(rt_progressive_refine(x.c, tolerance, (uint32_t)spp, nullptr, &active, &traced), "rt_progressive_refine");
            if (active == 0) {
                (void)collect();   // a half-count snapshot above 2.0 is not the image's
                chk(rt_progressive_counts(x.c, counts.data()), "rt_progressive_counts");
                break;
            }
            step((size_t)active, traced);
        }
        while (!device_plan) {
            chk(rt_progressive_error_async(x.c, x.err, nullptr), "rt_progressive_error_async");
            (void)collect();   // a half-count snapshot above 2.0 is not the image's
            chk(rt_memcpy_d2h(x.c, err.data(), x.err, npx * sizeof(double)), "rt_memcpy_d2h");
            chk(rt_progressive_counts(x.c, counts.data()), "rt_progressive_counts");
            size_t active = 0;
            for (size_t p = 0; p < npx; ++p)
                if (err[p] > tolerance && counts[p] < spp) {
                    counts[p] = (uint32_t)std::min<uint64_t>(2ull * counts[p], spp);
                    ++active;
                }
            if (active == 0) break;
            chk(rt_progressive_extend_map_async(x.c, counts.data(), nullptr, nullptr, nullptr), "rt_progressive_extend_map_async");
            const uint64_t before = total.samples;
            (void)collect();
            step(active, total.samples - before);
        }
        chk(rt_progressive_snapshot_map_async(x.c, nullptr, x.buf, nullptr, nullptr), "rt_progressive_snapshot_map_async");
        if (collect()) throw Panic("assertion failed: a pixel channel exceeded 2.0 (color.rs:55-57)");
        chk(rt_memcpy_d2h(x.c, img.data.data(), x.buf, npx * 3), "rt_memcpy_d2h");
        chk(rt_progressive_end(x.c), "rt_progressive_end");
        RenderStat stat(std::chrono::steady_clock::now() - t0, npx, total);
        return {std::move(img), stat};
    }

    // Guide buffers (rt_render_guides_async): per pixel the mean first-hit albedo, normal, depth and coverage over
    // the primary rays of render()'s image at spp samples, as exact float32 values, row-major from the top row.
    // One launch over the whole image on a context of its own.  The live path only.
    struct Guides {
        uint32_t width = 0, height = 0;
        std::vector<float> albedo, normal, depth, coverage;   // [h][w][3], [h][w][3], [h][w], [h][w]
        rt_stats gpu{};
    };
    Guides render_guides(size_t spp, const Scene& scene, const Camera& camera) {
        FlatScene flat = scene.flatten();
        rt_scene rs = flat.view();
        Guides g;
        g.width = camera.image_width();
        g.height = camera.image_height();
        const size_t npx = (size_t)g.width * g.height;
        struct Ctx {
            rt_context* c = nullptr;
            void* buf[4] = {nullptr, nullptr, nullptr, nullptr};
            ~Ctx() {
                for (void* b : buf) if (b) rt_device_free(c, b);
                if (c) rt_context_destroy(c);
            }
        } x;
        auto chk = [](int rc, const char* what) {
            if (rc != RT_OK) throw Panic(std::string(what) + ": " + rt_last_error());
        };
        chk(rt_context_create(0, &x.c), "rt_context_create");
        chk(rt_context_set_scene(x.c, &rs), "rt_context_set_scene");
        std::vector<float>* out[4] = {&g.albedo, &g.normal, &g.depth, &g.coverage};
        const size_t ch[4] = {3, 3, 1, 1};
        for (int i = 0; i < 4; ++i) chk(rt_device_alloc(x.c, npx * ch[i] * sizeof(float), &x.buf[i]), "rt_device_alloc");
        chk(rt_render_guides_async(x.c, &camera.c, (uint32_t)spp, seed, flags, nullptr, x.buf[0], x.buf[1], x.buf[2],
                                   x.buf[3], nullptr),
            "rt_render_guides_async");
        chk(rt_context_collect(x.c, nullptr, &g.gpu), "rt_context_collect");
        for (int i = 0; i < 4; ++i) {
            out[i]->resize(npx * ch[i]);
            chk(rt_memcpy_d2h(x.c, out[i]->data(), x.buf[i], npx * ch[i] * sizeof(float)), "rt_memcpy_d2h");
        }
        return g;
    }

    // Picking (rt_query_hits_async): what lies under the centre of each pixel (col, row) of `pixels`.  The ray starts
    // at the camera centre and goes through the pixel centre, Camera::get_ray (ray_tracing.rs:77-84) with both jitter
    // draws at 0.5 and no defocus offset, computed here in the render's precision T; the shared-origin path with
    // RT_FLAG_ROOT2 (a camera inside a sphere picks that sphere).  One launch on a context of its own.
    struct Pick {
        uint32_t col = 0, row = 0;
        int32_t index = -1;          // scene index; RT_QUERY_MISS, RT_QUERY_INVALID
        uint32_t kind = 0;           // the hit sphere's material kind
        double t = 0, point[3] = {0, 0, 0}, normal[3] = {0, 0, 0};
        bool front = false;
    };
    template <typename T>
    std::vector<Pick> pick_t(const std::vector<std::pair<uint32_t, uint32_t>>& pixels, const Scene& scene,
                             const Camera& camera) {
        FlatScene flat = scene.flatten();
        rt_scene rs = flat.view();
        const size_t n = pixels.size();
        const rt_camera& c = camera.c;
        std::vector<T> dir(3 * n);
        for (size_t i = 0; i < n; ++i) {
            const T fx = ((T)pixels[i].first + T(0.5)) / (T)c.image_width;     // ray_tracing.rs:78-80
            const T fy = ((T)pixels[i].second + T(0.5)) / (T)c.image_height;
            T v[3];
            for (int a = 0; a < 3; ++a) {
                const T off = (T)c.vu[a] * fx + (T)c.vv[a] * fy;
                const T pc = (T)c.ulc[a] + off;                                 // :81
                v[a] = pc - (T)c.center[a];                                     // :84
            }
            const T len = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);   // unit_vector, no FMA
            for (int a = 0; a < 3; ++a) dir[3 * i + a] = v[a] / len;
        }
        struct Ctx {
            rt_context* c = nullptr;
            void* buf[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
            ~Ctx() {
                for (void* b : buf) if (b) rt_device_free(c, b);
                if (c) rt_context_destroy(c);
            }
        } x;
        auto chk = [](int rc, const char* what) {
            if (rc != RT_OK) throw Panic(std::string(what) + ": " + rt_last_error());
        };
        chk(rt_context_create(0, &x.c), "rt_context_create");
        chk(rt_context_set_scene(x.c, &rs), "rt_context_set_scene");
        const size_t bytes[6] = {3 * n * sizeof(T), n * sizeof(T), n * sizeof(int32_t), 3 * n * sizeof(T), 3 * n * sizeof(T), n};
        for (int i = 0; i < 6; ++i) chk(rt_device_alloc(x.c, bytes[i], &x.buf[i]), "rt_device_alloc");
        std::vector<Pick> out(n);
        if (n == 0) return out;
        chk(rt_memcpy_h2d(x.c, x.buf[0], dir.data(), bytes[0]), "rt_memcpy_h2d");
        const uint32_t qflags = (flags & RT_FLAG_F32) | RT_FLAG_ROOT2;
        chk(rt_query_hits_async(x.c, n, nullptr, c.center, x.buf[0], qflags, x.buf[1], x.buf[2], x.buf[3], x.buf[4],
                                x.buf[5], nullptr),
            "rt_query_hits_async");
        chk(rt_context_collect(x.c, nullptr, nullptr), "rt_context_collect");
        std::vector<T> t(n), nrm(3 * n), pnt(3 * n);
        std::vector<int32_t> idx(n);
        std::vector<uint8_t> fr(n);
        chk(rt_memcpy_d2h(x.c, t.data(), x.buf[1], bytes[1]), "rt_memcpy_d2h");
        chk(rt_memcpy_d2h(x.c, idx.data(), x.buf[2], bytes[2]), "rt_memcpy_d2h");
        chk(rt_memcpy_d2h(x.c, nrm.data(), x.buf[3], bytes[3]), "rt_memcpy_d2h");
        chk(rt_memcpy_d2h(x.c, pnt.data(), x.buf[4], bytes[4]), "rt_memcpy_d2h");
        chk(rt_memcpy_d2h(x.c, fr.data(), x.buf[5], bytes[5]), "rt_memcpy_d2h");
        for (size_t i = 0; i < n; ++i) {
            Pick& p = out[i];
            p.col = pixels[i].first;
            p.row = pixels[i].second;
            p.index = idx[i];
            p.kind = idx[i] >= 0 ? flat.materials[flat.material[(size_t)idx[i]]].kind : 0u;
            p.t = (double)t[i];
            for (int a = 0; a < 3; ++a) { p.point[a] = (double)pnt[3 * i + a]; p.normal[a] = (double)nrm[3 * i + a]; }
            p.front = fr[i] != 0;
        }
        return out;
    }
    std::vector<Pick> pick(const std::vector<std::pair<uint32_t, uint32_t>>& pixels, const Scene& scene,
                           const Camera& camera) {
        return (flags & RT_FLAG_F32) ? pick_t<float>(pixels, scene, camera) : pick_t<double>(pixels, scene, camera);
    }

    // A camera model the reference lacks (rt_camera_rays: orthographic, panorama, fisheye), path-traced with
    // rt_render_rays_async: grid x grid rays per pixel on the host, uploaded once, sample s of a pixel starting as
    // its ray s % grid^2.  One launch on a context of its own; RT_FLAG_F32 and RT_FLAG_ROOT2 are passed on.
    template <typename T>
    std::pair<RgbImage, RenderStat> render_projection_t(size_t max_bounces, size_t spp, const Scene& scene,
                                                        const rt_projection& proj, uint32_t grid) {
        const auto t0 = std::chrono::steady_clock::now();
        FlatScene flat = scene.flatten();
        rt_scene rs = flat.view();
        RgbImage img{proj.image_width, proj.image_height, {}};
        const size_t npx = (size_t)img.width * img.height, nrays = npx * grid * grid;
        img.data.resize(npx * 3);
        auto chk = [](int rc, const char* what) {
            if (rc != RT_OK) throw Panic(std::string(what) + ": " + rt_last_error());
        };
        std::vector<T> org(3 * nrays), dir(3 * nrays);
        const uint32_t rflags = flags & (RT_FLAG_F32 | RT_FLAG_ROOT2);
        chk(rt_camera_rays(&proj, grid, rflags & RT_FLAG_F32, org.data(), dir.data()), "rt_camera_rays");
        struct Ctx {
            rt_context* c = nullptr;
            void* buf[3] = {nullptr, nullptr, nullptr};
            ~Ctx() {
                for (void* b : buf) if (b) rt_device_free(c, b);
                if (c) rt_context_destroy(c);
            }
        } x;
        chk(rt_context_create(0, &x.c), "rt_context_create");
        chk(rt_context_set_scene(x.c, &rs), "rt_context_set_scene");
        const size_t bytes = 3 * nrays * sizeof(T);
        chk(rt_device_alloc(x.c, bytes, &x.buf[0]), "rt_device_alloc");
        chk(rt_device_alloc(x.c, bytes, &x.buf[1]), "rt_device_alloc");
        chk(rt_device_alloc(x.c, npx * 3, &x.buf[2]), "rt_device_alloc");
        chk(rt_memcpy_h2d(x.c, x.buf[0], org.data(), bytes), "rt_memcpy_h2d");
        chk(rt_memcpy_h2d(x.c, x.buf[1], dir.data(), bytes), "rt_memcpy_h2d");
        chk(rt_render_rays_async(x.c, npx, (uint32_t)spp, grid * grid, x.buf[0], nullptr, x.buf[1], (uint32_t)max_bounces,
                                 seed, 0u, rflags, x.buf[2], nullptr, nullptr),
            "rt_render_rays_async");
        rt_stats st{};
        const int rc = rt_context_collect(x.c, nullptr, &st);
        if (rc == RT_ERR_RANGE) throw Panic(std::string("assertion failed: ") + rt_last_error());
        chk(rc, "rt_context_collect");
        chk(rt_memcpy_d2h(x.c, img.data.data(), x.buf[2], npx * 3), "rt_memcpy_d2h");
        RenderStat stat(std::chrono::steady_clock::now() - t0, npx, st);
        return {std::move(img), stat};
    }
    std::pair<RgbImage, RenderStat> render_projection(size_t max_bounces, size_t spp, const Scene& scene,
                                                      const rt_projection& proj, uint32_t grid) {
        return (flags & RT_FLAG_F32) ? render_projection_t<float>(max_bounces, spp, scene, proj, grid)
                                     : render_projection_t<double>(max_bounces, spp, scene, proj, grid);
    }

  private:
    void render_blocks(const rt_scene& rs, const Camera& camera, uint32_t max_bounces, uint32_t spp, RgbImage& img,
                       rt_stats& total, uint32_t B, bool print_blocks) {
        struct Ctx {
            rt_context* c = nullptr;
            void* buf = nullptr;
            ~Ctx() { if (buf) rt_device_free(c, buf); if (c) rt_context_destroy(c); }
        } x;
        auto chk = [](int rc, const char* what) {
            if (rc == RT_ERR_RANGE) throw Panic(std::string("assertion failed: ") + rt_last_error());
            if (rc != RT_OK) throw Panic(std::string(what) + ": " + rt_last_error());
        };
        chk(rt_context_create(0, &x.c), "rt_context_create");
        chk(rt_context_set_scene(x.c, &rs), "rt_context_set_scene");
        const uint32_t W = img.width, H = img.height;
        const size_t tile_px = (size_t)std::min(B, W) * std::min(B, H);
        chk(rt_device_alloc(x.c, tile_px * 3, &x.buf), "rt_device_alloc");
        std::vector<uint8_t> tile(tile_px * 3);
        const uint32_t nbx = (W + B - 1) / B, nby = (H + B - 1) / B;   // renderer.rs:248-266
        bool range_err = false;
        for (uint32_t by = 0; by < nby; ++by)
            for (uint32_t bx = 0; bx < nbx; ++bx) {
                const uint32_t c0 = bx * B, r0 = by * B;
                const rt_tile_range tr{r0, 1, std::min(B, H - r0), c0, std::min(B, W - c0)};
                if (sample_parallel)
                    chk(rt_render_split_async(x.c, &camera.c, max_bounces, spp, seed, flags, &tr, x.buf, nullptr, nullptr, 0u),
                        "rt_render_split_async");
                else
                    chk(rt_render_async(x.c, &camera.c, max_bounces, spp, seed, flags, &tr, x.buf, nullptr, nullptr),
                        "rt_render_async");
                rt_stats st{};
                const int rc = rt_context_collect(x.c, nullptr, &st);
                if (rc == RT_ERR_RANGE) range_err = true;
                else chk(rc, "rt_context_collect");
                const size_t npx = (size_t)tr.row_count * tr.col_count;
                chk(rt_memcpy_d2h(x.c, tile.data(), x.buf, npx * 3), "rt_memcpy_d2h");
                for (uint32_t r = 0; r < tr.row_count; ++r)
                    std::memcpy(&img.data[((size_t)(r0 + r) * W + c0) * 3], &tile[(size_t)r * tr.col_count * 3],
                                (size_t)tr.col_count * 3);
                // renderer.rs:339: "Thread {} complete block ({}, {}) at {:.2} px/s"
                if (print_blocks) std::printf("Device 0 complete block (%u, %u) at %.2f px/s\n", bx, by, st.pixels_per_second);
                total.kernel_ms += st.kernel_ms;
                total.pixels += st.pixels;
                total.samples += st.samples;
                total.ray_segments += st.ray_segments;
                total.lane_slots += st.lane_slots;
                total.direct_sky_samples += st.direct_sky_samples;
                total.bounce_iters += st.bounce_iters;
            }
        if (range_err) throw Panic("assertion failed: a pixel channel exceeded 2.0 (color.rs:55-57)");
    }
};

}  // namespace rt_host
