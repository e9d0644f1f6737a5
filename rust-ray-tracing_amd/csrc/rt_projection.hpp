// rt_projection.hpp — primary rays of the camera models the reference lacks (rt_camera_rays): orthographic, a
// 360 x 180 degree panorama (equirectangular) and an equidistant fisheye, as host arrays that rt_render_rays_async
// and rt_query_hits_async take once uploaded.  Pure host C++ (no HIP): the library, and the stand-alone sanitizer
// program tests/sanitize/projection_san.cpp include it.
//
// Everything is computed in double and rounded to the ray type last.  The frame is Camera::new's
// (ray_tracing.rs:34-37, Vec3 ops without FMA: compile with -ffp-contract=off): dir = unit(look_at - center),
// w = -dir, u = unit(up x w), v = w x u; u points right in the image, v up.  Pixel (col, row) holds grid x grid rays,
// ray j grid + i through the sub-pixel position ((i + 0.5) / grid, (j + 0.5) / grid); row 0 is the top row.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rt_mi355x.h"

namespace rt {

// Return codes, the values of RT_OK / RT_ERR_INVALID / RT_ERR_UNSUPPORTED (include/rt_mi355x.h).
constexpr int kProjOk = 0, kProjInvalid = 1, kProjUnsupported = 4;
constexpr uint32_t kProjMaxGrid = 1024;              // grid^2 rays per pixel <= the ABI's spp limit, 2^20
constexpr uint64_t kProjMaxPixels = 0x7FFFFFFFull;   // pixels of one rt_render_rays_async call

struct ProjFrame { double dir[3], u[3], v[3]; };

inline bool proj_finite3(const double a[3]) { return isfinite(a[0]) && isfinite(a[1]) && isfinite(a[2]); }

// Camera::new's frame; false where it does not exist (look_at == center, up along the view axis, a non-finite input).
inline bool proj_frame(const rt_projection& p, ProjFrame& f) {
    if (!proj_finite3(p.center) || !proj_finite3(p.look_at) || !proj_finite3(p.up)) return false;
    const double dv[3] = {p.look_at[0] - p.center[0], p.look_at[1] - p.center[1], p.look_at[2] - p.center[2]};
    const double dl = sqrt(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]);
    if (!(dl > 0.0) || !isfinite(dl)) return false;
    double w[3];
    for (int i = 0; i < 3; ++i) { f.dir[i] = dv[i] / dl; w[i] = -f.dir[i]; }
    const double cr[3] = {p.up[1] * w[2] - p.up[2] * w[1], p.up[2] * w[0] - p.up[0] * w[2], p.up[0] * w[1] - p.up[1] * w[0]};
    const double cl = sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
    if (!(cl > 0.0) || !isfinite(cl)) return false;
    for (int i = 0; i < 3; ++i) f.u[i] = cr[i] / cl;
    f.v[0] = w[1] * f.u[2] - w[2] * f.u[1];
    f.v[1] = w[2] * f.u[0] - w[0] * f.u[2];
    f.v[2] = w[0] * f.u[1] - w[1] * f.u[0];
    return true;
}

// One ray: the image position (x, y) in pixels from the top-left corner.  o, d in double.
inline void proj_ray(const rt_projection& p, const ProjFrame& f, double x, double y, double o[3], double d[3]) {
    const double W = (double)p.image_width, H = (double)p.image_height;
    const double kPi = 3.141592653589793;
    for (int i = 0; i < 3; ++i) o[i] = p.center[i];
    if (p.model == RT_PROJ_ORTHOGRAPHIC) {
        const double height = p.extent, width = height * (W / H);
        const double a = (x / W - 0.5) * width, b = (0.5 - y / H) * height;
        for (int i = 0; i < 3; ++i) {
            o[i] = (p.center[i] + f.u[i] * a) + f.v[i] * b;
            d[i] = f.dir[i];
        }
    } else if (p.model == RT_PROJ_EQUIRECT) {
        const double lon = (x / W - 0.5) * (2.0 * kPi), lat = (0.5 - y / H) * kPi;
        const double cl = cos(lat), a = cl * cos(lon), b = cl * sin(lon), c = sin(lat);
        for (int i = 0; i < 3; ++i) d[i] = (f.dir[i] * a + f.u[i] * b) + f.v[i] * c;
    } else {   // RT_PROJ_FISHEYE, equidistant
        const double half = (p.image_width < p.image_height ? W : H) / 2.0;
        const double px = x - W / 2.0, py = y - H / 2.0;
        const double rp = sqrt(px * px + py * py), r = rp / half;
        if (r > 1.0) {   // outside the image circle: a zero direction, an invalid ray
            d[0] = d[1] = d[2] = 0.0;
        } else if (rp == 0.0) {
            for (int i = 0; i < 3; ++i) d[i] = f.dir[i];
        } else {
            const double theta = r * ((p.angle_deg / 2.0) * (kPi / 180.0));
            const double ct = cos(theta), st = sin(theta), a = (px / rp) * st, b = (py / rp) * st;
            for (int i = 0; i < 3; ++i) d[i] = (f.dir[i] * ct + f.u[i] * a) - f.v[i] * b;
        }
    }
}

template <typename T>
inline void proj_fill(const rt_projection& p, const ProjFrame& f, uint32_t grid, T* origins, T* directions) {
    size_t ray = 0;
    for (uint32_t row = 0; row < p.image_height; ++row)
        for (uint32_t col = 0; col < p.image_width; ++col)
            for (uint32_t j = 0; j < grid; ++j)
                for (uint32_t i = 0; i < grid; ++i, ++ray) {
                    double o[3], d[3];
                    proj_ray(p, f, (double)col + ((double)i + 0.5) / (double)grid, (double)row + ((double)j + 0.5) / (double)grid, o, d);
                    for (int a = 0; a < 3; ++a) {
                        origins[3 * ray + a] = (T)o[a];
                        directions[3 * ray + a] = (T)d[a];
                    }
                }
}

// rt_camera_rays: origins and directions are host arrays [W H grid^2][3] of float (RT_FLAG_F32) or double.
inline int camera_rays(const rt_projection* p, uint32_t grid, uint32_t flags, void* origins, void* directions) {
    if (!p || !origins || !directions) return kProjInvalid;
    if (p->image_width == 0 || p->image_height == 0 || grid == 0) return kProjInvalid;
    if (p->model > RT_PROJ_FISHEYE || (flags & ~RT_FLAG_F32)) return kProjInvalid;
    if (p->model == RT_PROJ_FISHEYE && !(p->angle_deg > 0.0 && p->angle_deg <= 360.0)) return kProjInvalid;
    if (p->model == RT_PROJ_ORTHOGRAPHIC && !(p->extent > 0.0 && isfinite(p->extent))) return kProjInvalid;
    ProjFrame f;
    if (!proj_frame(*p, f)) return kProjInvalid;
    if ((uint64_t)p->image_width * p->image_height > kProjMaxPixels || grid > kProjMaxGrid) return kProjUnsupported;
    if (flags & RT_FLAG_F32) proj_fill<float>(*p, f, grid, (float*)origins, (float*)directions);
    else proj_fill<double>(*p, f, grid, (double*)origins, (double*)directions);
    return kProjOk;
}

}  // namespace rt
