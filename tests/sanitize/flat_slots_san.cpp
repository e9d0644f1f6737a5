// AddressSanitizer + UBSan harness of the flat slot table (csrc/rt_layout.hpp, pack_flat: one {cx, cy, cz, r^2}
// record per slot, the table nearest_hit's per-lane exact tests gather from).  Pure host C++: no HIP.
// It builds its scenes itself: n spheres of radius 0.2 .. 0.3 in a slab (all filtered), optionally with a ground
// sphere (always exact: far out) and three radius-1 spheres (big: always exact too), for n = 1, 16, 17, 500, 2048.
// For every slot of every image it checks, bit for bit, that the flat record holds the centre of the slot's filter
// group and the r^2 of its record in the cluster block of the fp32 filter stream (inline_stream; the always-exact
// slots: the centre of their filter group and the r^2 of the fp32 exact stream), that the block's index word
// equals ridx[slot], that a dummy slot is {0, 0, 0, -inf}, and that the table ends with ridx.  A violation exits
// non-zero even without a sanitizer report.
// stdout: one line per scene, "name n n_xg n_xs n_top n_mg slots dummies".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../rust-ray-tracing_amd/csrc/rt_layout.hpp"

static int g_bad = 0;
static std::string g_name;
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) { std::fprintf(stderr, "%s: violated: %s\n", g_name.c_str(), #cond); g_bad = 1; } \
    } while (0)

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static double uniform() {   // xorshift64*, [0, 1)
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return (double)((g_rng * 0x2545F4914F6CDD1Dull) >> 11) * 0x1.0p-53;
}

static void check_scene(const char* name, unsigned n, bool exact) {
    g_name = name;
    std::vector<double> center, radius;
    for (unsigned i = 0; i < n; ++i) {
        center.push_back(32.0 * uniform() - 16.0);
        center.push_back(0.4 + 1.2 * uniform());
        center.push_back(32.0 * uniform() - 16.0);
        radius.push_back(0.2 + 0.1 * uniform());
    }
    if (exact) {
        // after sphere n / 2: the always-exact spheres sit in the middle of the scene order
        const size_t at = n / 2;
        const double big[4][4] = {{0.0, -1000.0, 0.0, 1000.0}, {0.0, 1.0, 0.0, 1.0}, {-4.0, 1.0, 0.0, 1.0}, {4.0, 1.0, 0.0, 1.0}};
        for (int k = 3; k >= 0; --k) {
            center.insert(center.begin() + 3 * at, big[k], big[k] + 3);
            radius.insert(radius.begin() + at, big[k][3]);
        }
    }
    const uint32_t ns = (uint32_t)radius.size();
    std::vector<uint32_t> material(ns, 0u);
    rt_material mat;
    std::memset(&mat, 0, sizeof(mat));
    mat.albedo[0] = mat.albedo[1] = mat.albedo[2] = 0.5;
    rt_scene s;
    std::memset(&s, 0, sizeof(s));
    s.n_spheres = ns;
    s.center = center.data();
    s.radius = radius.data();
    s.material = material.data();
    s.n_materials = 1;
    s.materials = &mat;

    const SceneImage im = build_scene_image(&s);
    const SceneTables<float>& t = im.t32;
    const size_t nxg = im.n.n_xg, ncl = 4 * (size_t)im.n.n_top, nslots = im.ridx.size();
    CHECK(im.t64.rflat.empty());                        // fp64 rays keep the wave-level tests
    CHECK(nslots == im.n.n_cslots && nslots == 4 * nxg + 16 * ncl + 64);
    CHECK(t.rflat.size() == 4 * nslots);                // record i and ridx[i] are the same slot
    CHECK(t.rfsph.size() == 16 * nxg + 96 * ncl + 32);
    CHECK(t.rsph.size() == 16 * (nxg + 4 * ncl + 1));
    if (g_bad) return;
    const float ninf = -std::numeric_limits<float>::infinity();
    size_t dummies = 0, real = 0;
    for (size_t i = 0; i < nslots; ++i) {
        const float* r = &t.rflat[4 * i];
        float want[4] = {0.0f, 0.0f, 0.0f, ninf};
        uint32_t idx = 0xFFFFFFFFu;
        if (i < 4 * nxg) {
            // an always-exact slot: group i / 4 at the head of both streams, pair-interleaved
            const size_t g = i / 4, j = i % 4;
            for (int f = 0; f < 3; ++f) want[f] = t.rfsph[16 * g + 8 * (j / 2) + 2 * f + (j % 2)];
            want[3] = t.rsph[16 * g + 8 * (j / 2) + 6 + (j % 2)];
            idx = im.ridx[i];
        } else if (i < 4 * nxg + 16 * ncl) {
            // slot sl of cluster k: the centre in group sl / 4 of the cluster's block, r^2 and the scene index in
            // the record of that group behind the four groups
            const size_t k = (i - 4 * nxg) / 16, sl = (i - 4 * nxg) % 16;
            const float* b = &t.rfsph[16 * nxg + 96 * k];
            for (int f = 0; f < 3; ++f) want[f] = b[16 * (sl / 4) + 8 * ((sl % 4) / 2) + 2 * f + (sl % 2)];
            want[3] = b[64 + 8 * (sl / 4) + (sl % 4)];
            std::memcpy(&idx, &b[68 + 8 * (sl / 4) + (sl % 4)], 4);
            CHECK(idx == im.ridx[i]);
            // ... the same values as the exact stream's
            const size_t g = nxg + 4 * k + sl / 4, j = sl % 4;
            CHECK(same_bits(want[3], t.rsph[16 * g + 8 * (j / 2) + 6 + (j % 2)]));
        } else {
            CHECK(im.ridx[i] == 0xFFFFFFFFu);           // past the last cluster
        }
        for (int f = 0; f < 4; ++f)
            if (!same_bits(r[f], want[f])) {
                std::fprintf(stderr, "%s: slot %zu word %d: flat %a, stream %a\n", name, i, f, (double)r[f], (double)want[f]);
                g_bad = 1;
            }
        if (idx == 0xFFFFFFFFu) {
            ++dummies;
            CHECK(same_bits(r[3], ninf) && r[0] == 0.0f && r[1] == 0.0f && r[2] == 0.0f);   // never a candidate, never hit
        } else {
            ++real;
            CHECK(idx < ns);
            if (idx < ns) {
                const float rr = (float)radius[idx];
                CHECK(same_bits(r[0], (float)center[3 * idx]) && same_bits(r[1], (float)center[3 * idx + 1]) &&
                      same_bits(r[2], (float)center[3 * idx + 2]) && same_bits(r[3], rr * rr));
            }
        }
    }
    CHECK(real == ns);
    std::printf("%s %u %u %u %u %u %zu %zu\n", name, ns, im.n.n_xg, im.n.n_xs, im.n.n_top, im.n.n_mg, nslots, dummies);
}

int main() {
    const unsigned counts[] = {1, 16, 17, 500, 2048};
    for (unsigned n : counts)
        for (int exact = 0; exact < 2; ++exact) {
            char name[64];
            std::snprintf(name, sizeof(name), "slab%u%s", n, exact ? "_exact" : "");
            check_scene(name, n, exact != 0);
        }
    return g_bad;
}
