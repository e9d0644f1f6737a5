// rt_formats.hpp — the formats the host's scene layout (rt_layout.hpp) and the device code (rt_common.hpp)
// share: record types, group sizes and the filter's constants.  No HIP: plain C++, so the layout code
// builds and runs without a GPU toolchain.
#pragma once
#include <stdint.h>

namespace rt {

template <typename T> struct MatT {
    uint32_t kind, hollow;
    // Lambertian / metal: {albedo r, g, b, fuzz}; dielectric: {ior, 1/ior, r0_front, r0_back} -- the constants
    // precomputed on the host in T with the reference's operations (IEEE, no contraction, so the bits equal the
    // per-ray device computation): 1/ior (materials.rs:131) and Schlick's r0 = ((1-ratio)/(1+ratio))^2
    // (materials.rs:122) for ratio = 1/ior and ior.  Only the fields of the record's kind: fp64 40 bytes, fp32 24.
    T p[4];
};

// Device sphere layout (build_scene_image): 64-byte groups, one s_load_dwordx16 each, padded
// with never-hit dummies (r^2 = -inf makes the discriminant -inf) to whole groups.
//   fp32: 4 spheres per group as 2 pair-interleaved records {cx0,cx1, cy0,cy1, cz0,cz1, r0,r1}
//         so each quantity of a sphere pair is an adjacent SGPR pair for packed-FP32 VALU ops;
//   fp64: 2 spheres per group as {cx, cy, cz, r^2}.
// A separate AoS table {cx, cy, cz, signed radius} per sphere serves the per-lane finalize gather.
// The filter stream (both precisions) is fp32 in the fp32 layout, with r^2 replaced by the filter's
// r2f: r^2 rounded up to fp32, +inf for "always exact" spheres, -inf for dummies (see
// general_sweep).
template <typename T> constexpr uint32_t kGroup = 64 / (4 * sizeof(T));

// One top group of the general sweep: 4 cluster boxes {centre, half-extent} (pack_sweep), 96 bytes,
// pair-interleaved like SphGroup: pair q at 12 q, {cx0,cx1, cy0,cy1, cz0,cz1, hx0,hx1, hy0,hy1, hz0,hz1}.
constexpr uint32_t kBoxFloats = 24;

constexpr float kFilterMargin = 48.0f * 0x1.0p-24f;   // general-sweep filter margin factor (nearest_hit)
constexpr double kExactRatio = 8.0;  // spheres with |c|_1 + r > kExactRatio x the median are "always exact"

}  // namespace rt
