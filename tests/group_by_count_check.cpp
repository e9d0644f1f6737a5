// group_by_count (csrc/rt_progressive_plan.hpp) against a naive grouping written here: the distinct non-zero counts
// sorted ascending, then the pixels appended to their class in pixel order.  Checked per case: the return value,
// the classes' spp / first / n, the index list, and that the pass without a list gives the classes of the pass
// with one (run_map calls the first, then the second on the same vector).  Prints one line per case, "NAME ok" or
// "NAME FAIL: why"; exits 1 if any failed.  Built and run by tests/test_group_by_count.py.
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "../rust-ray-tracing_amd/csrc/rt_progressive_plan.hpp"

using rt::CountClass;

static bool same(const std::vector<CountClass>& a, const std::vector<CountClass>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].spp != b[i].spp || a[i].first != b[i].first || a[i].n != b[i].n) return false;
    return true;
}

// Empty: the case holds.
static std::string check(const std::vector<uint32_t>& counts) {
    const uint32_t n_pix = (uint32_t)counts.size();
    std::vector<uint32_t> distinct;
    for (uint32_t v : counts)
        if (v != 0u && std::find(distinct.begin(), distinct.end(), v) == distinct.end()) distinct.push_back(v);
    std::sort(distinct.begin(), distinct.end());
    const bool accept = distinct.size() <= rt::kMaxCountClasses;
    std::vector<CountClass> want;
    std::vector<uint32_t> want_list;
    for (uint32_t v : distinct) {
        CountClass k{v, (uint32_t)want_list.size(), 0u};
        for (uint32_t p = 0; p < n_pix; ++p)
            if (counts[p] == v) { want_list.push_back(p); ++k.n; }
        want.push_back(k);
    }
    constexpr uint32_t kGuard = 0xDEADBEEFu;   // behind the list: group_by_count writes one word per non-zero pixel
    std::vector<uint32_t> list(n_pix + 1u, kGuard), list2(n_pix + 1u, kGuard);
    std::vector<CountClass> two_pass{CountClass{7u, 7u, 7u}}, fresh;   // a vector in use is cleared
    const bool r1 = rt::group_by_count(counts.data(), n_pix, nullptr, two_pass);
    if (r1 != accept) return "return value without a list";
    if (accept && !same(two_pass, want)) return "classes without a list";
    const bool r2 = rt::group_by_count(counts.data(), n_pix, list.data(), two_pass);
    const bool r3 = rt::group_by_count(counts.data(), n_pix, list2.data(), fresh);
    if (r2 != accept || r3 != accept) return "return value with a list";
    if (!accept) return "";
    if (!same(two_pass, want) || !same(fresh, want)) return "classes with a list";
    for (const std::vector<uint32_t>* l : {&list, &list2}) {
        if (!std::equal(want_list.begin(), want_list.end(), l->begin())) return "list";
        for (size_t i = want_list.size(); i < l->size(); ++i)
            if ((*l)[i] != kGuard) return "a write behind the list";
    }
    return "";
}

static int g_failed = 0;
static void run(const std::string& name, const std::vector<uint32_t>& counts) {
    const std::string why = check(counts);
    if (!why.empty()) ++g_failed;
    printf("%s %s%s\n", name.c_str(), why.empty() ? "ok" : "FAIL: ", why.c_str());
}

int main() {
    for (uint32_t n : {0u, 1u, 2u, 5u, 64u}) {
        const std::string at = "_n" + std::to_string(n);
        std::vector<uint32_t> c(n);
        run("all_zero" + at, c);
        std::fill(c.begin(), c.end(), 48u);
        run("one_class" + at, c);
        for (uint32_t p = 0; p < n; ++p) c[p] = p % 2u ? 16u : 512u;   // the one-entry cache misses at every pixel
        run("alternating" + at, c);
        for (uint32_t p = 0; p < n; ++p) c[p] = 4u * (n - p);           // every new class goes in at the front
        run("descending" + at, c);
        for (uint32_t p = 0; p < n; ++p) c[p] = p % 3u == 1u ? 0u : (p % 2u ? 32u : 8u);
        run("zeros_interleaved" + at, c);
        for (uint32_t p = 0; p < n; ++p) c[p] = p % 2u ? 0u : 4u * (n - p);   // zeros between front inserts
        run("zeros_descending" + at, c);
    }
    {
        // 299 pixels cycle through 256 distinct counts (descending: front inserts until the table is full); the
        // last pixel repeats one of them (accepted) or brings the 257th (refused)
        std::vector<uint32_t> c(300);
        for (uint32_t p = 0; p < 300u; ++p) c[p] = 1000u - p % 256u;
        run("distinct_256", c);
        c[299] = 2000u;
        run("distinct_257_at_last_pixel", c);
        c[299] = 1u;
        run("distinct_257_at_last_pixel_front", c);
    }
    std::mt19937 rng(0x5EED0001u);
    int bad = 0;
    for (int m = 0; m < 400; ++m) {
        const uint32_t n = 1u + rng() % 1000u, kinds = 1u + rng() % 8u, run_len = 1u + rng() % 9u;
        uint32_t palette[8];
        for (uint32_t& v : palette) v = rng() % 4u == 0u ? 0u : 1u + rng() % (1u << 20);   // zero: left out
        std::vector<uint32_t> c(n);
        for (uint32_t p = 0; p < n; ++p)   // runs of neighbours that share a count, as an image has them
            c[p] = (p % run_len && p) ? c[p - 1] : palette[rng() % kinds];
        const std::string why = check(c);
        if (!why.empty()) {
            ++bad;
            printf("random map %d FAIL: %s\n", m, why.c_str());
        }
    }
    g_failed += bad;
    printf("random_400 %s\n", bad ? "FAIL" : "ok");
    return g_failed ? 1 : 0;
}
