// AddressSanitizer + UBSan harness of the scene image (csrc/rt_layout.hpp, pure host C++: no HIP).
// stdin: scenes as text, "name n_spheres n_materials", then per sphere "cx cy cz r material", then per
// material "kind hollow r g b fuzz ior".  Each scene goes through build_scene_image and the invariants of
// the image are checked here, so a violation exits non-zero even without a sanitizer report.
// stdout: one line per scene, "name n n_xg n_xs n_top n_mg n_gg n_supc".
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../rust-ray-tracing_amd/csrc/rt_layout.hpp"

static int g_bad = 0;
static const char* g_name = "";
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::fprintf(stderr, "%s: violated: %s\n", g_name, #cond); g_bad = 1; } \
    } while (0)

template <typename T>
static void check_tables(const SceneImage& im, const SceneTables<T>& t, size_t ncl) {
    const SceneCounts& n = im.n;
    const size_t ns = 4 * (size_t)n.n_xg + 16 * ncl, nsg = ((size_t)n.n_top + 3) / 4, nmg = (nsg + 3) / 4;
    const size_t one = n.n_spheres ? n.n_spheres : 1;
    constexpr size_t NE = 64 / sizeof(T), G = kGroup<T>;
    CHECK(t.cen.size() == 4 * one);
    CHECK(t.mats.size() == one);
    CHECK(t.rsph.size() == NE * (ns / G + 1));
    CHECK(t.top.size() == kBoxFloats * ((size_t)n.n_top + 1));   // n_top + 1 groups
    CHECK(t.sup.size() == kBoxFloats * (nsg + 1));
    // the inline stream as inline_stream sizes it: a slot-order stream of ns / 4 groups + the dummy, n_xg
    // leading groups, the rest in clusters of 4 groups and 96 floats
    const size_t ngf = (16 * (ns / 4 + 1)) / 16 - 1, nk = (ngf - n.n_xg) / 4;
    CHECK(nk == ncl);
    CHECK(t.rfsph.size() == 16 * (size_t)n.n_xg + 96 * nk + 32);
    CHECK(t.clus.size() == 4 * (size_t)((n.n_clp + n.n_supc) ? n.n_clp + n.n_supc : 1));
    // the local levels are present exactly when there is a mega level
    const bool mega = n.n_mg > 0;
    CHECK(t.meg.empty() == !mega);
    CHECK(t.lfs.empty() == !mega);
    for (int lv = 0; lv < 4; ++lv) CHECK(t.lbx[lv].empty() == !mega);
    if (mega) {
        CHECK(n.n_mg == nmg);
        CHECK(t.meg.size() == kBoxFloats * ((size_t)n.n_mg + 1));
        CHECK(t.lfs.size() == t.rfsph.size());
        CHECK(t.lbx[0].size() == kLBoxFloats * ((size_t)n.n_top + 1));
        CHECK(t.lbx[1].size() == kLBoxFloats * (nsg + 1));
        CHECK(t.lbx[2].size() == kLBoxFloats * (nmg + 1));
        CHECK(t.lbx[3].size() == kLBoxFloats * ((nmg + 3) / 4 + 1));
    }
    CHECK(t.cam_bytes.camx == 4 * (size_t)n.n_cslots * sizeof(T));
    CHECK(t.cam_bytes.cull == 4 * (size_t)n.n_cslots * sizeof(float));
    CHECK(t.cam_bytes.cullc == t.clus.size() * sizeof(float));
}

static void check_scene(const rt_scene& s) {
    const SceneImage im = build_scene_image(&s);
    const SceneCounts& n = im.n;
    const SweepLayout L = build_layout(&s);
    const size_t ncl = L.members.size();
    for (const auto& m : L.members) CHECK(m.size() <= kClusterMax);   // no cluster has more than 16 members
    CHECK(ncl % 4 == 0 && n.n_top == ncl / 4);
    CHECK(n.n_spheres == s.n_spheres);
    CHECK(n.n_cslots == 4 * n.n_xg + 16 * ncl + 64);
    CHECK(n.n_clp % 64 == 0 && n.n_clp >= ncl);
    CHECK(n.n_supc % 64 == 0 && (n.n_supc != 0) == (ncl > 128) && (n.n_supc == 0 || n.n_supc >= ncl / 4));
    CHECK(n.n_xs <= 4 * n.n_xg && 4 * n.n_xg < n.n_xs + 4);
    CHECK(n.n_gg == 0 || (n.n_mg > 0 && n.n_mg <= 16));   // the giga pre-test: at most 16 mega groups
    CHECK(im.mtiers.empty() == (n.n_mg == 0));
    if (n.n_mg) CHECK(im.mtiers.size() == (size_t)4 * n.mt_n[0] * n.mt_n[1] * n.mt_n[2]);
    // every scene index exactly once in ridx, every other slot the dummy
    CHECK(im.ridx.size() == n.n_cslots);
    std::vector<uint32_t> seen(s.n_spheres, 0);
    for (uint32_t v : im.ridx) {
        if (v == 0xFFFFFFFFu) continue;
        CHECK(v < s.n_spheres);
        if (v < s.n_spheres) ++seen[v];
    }
    for (uint32_t i = 0; i < s.n_spheres; ++i)
        if (seen[i] != 1) { std::fprintf(stderr, "%s: sphere %u is in %u slots\n", g_name, i, seen[i]); g_bad = 1; break; }
    check_tables(im, im.t64, ncl);
    check_tables(im, im.t32, ncl);
    std::printf("%s %u %u %u %u %u %u %u\n", g_name, n.n_spheres, n.n_xg, n.n_xs, n.n_top, n.n_mg, n.n_gg, n.n_supc);
}

int main() {
    char name[128];
    unsigned ns = 0, nm = 0;
    int scenes = 0;
    while (std::scanf("%127s %u %u", name, &ns, &nm) == 3) {
        std::vector<double> center(3 * (size_t)ns), radius(ns);
        std::vector<uint32_t> material(ns);
        std::vector<rt_material> mats(nm);
        for (unsigned i = 0; i < ns; ++i)
            if (std::scanf("%lf %lf %lf %lf %u", &center[3 * i], &center[3 * i + 1], &center[3 * i + 2], &radius[i],
                           &material[i]) != 5) return 2;
        for (unsigned i = 0; i < nm; ++i) {
            rt_material& m = mats[i];
            memset(&m, 0, sizeof(m));
            if (std::scanf("%u %u %lf %lf %lf %lf %lf", &m.kind, &m.hollow, &m.albedo[0], &m.albedo[1], &m.albedo[2],
                           &m.fuzz, &m.ior) != 7) return 2;
        }
        rt_scene s;
        memset(&s, 0, sizeof(s));
        s.n_spheres = ns;
        s.center = center.data();
        s.radius = radius.data();
        s.material = material.data();
        s.n_materials = nm;
        s.materials = mats.data();
        const std::string keep = name;
        g_name = keep.c_str();
        check_scene(s);
        ++scenes;
    }
    return scenes ? g_bad : 2;
}
