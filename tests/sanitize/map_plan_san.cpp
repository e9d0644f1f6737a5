// AddressSanitizer + UBSan harness of the per-pixel-count plan (csrc/rt_progressive_plan.hpp, pure host C++).
// stdin: cases "n resident_waves slack  done_0 target_0 ... done_{n-1} target_{n-1}".  Each case runs
// progressive_map_plan twice, counting and then writing into a heap array of exactly n_items + slack records
// (slack < 0: too small, the call must refuse and write nothing), so a write past the plan's own count is an
// ASan report.  stdout: one line "rc S n_items" per case, then the items "pixel first end" of an accepted one.
// Every accepted plan is checked here as well (the items tile each window once, in pixel order, on the grain), so
// a violation exits non-zero even without a sanitizer report.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../rust-ray-tracing_amd/csrc/rt_progressive_plan.hpp"

static int check_items(const std::vector<uint32_t>& done, const std::vector<uint32_t>& target, uint32_t S,
                       const uint32_t* it, uint64_t n_items) {
    uint64_t at = 0;
    for (size_t p = 0; p < done.size(); ++p) {
        uint32_t covered = done[p];
        uint32_t n = 0;
        while (at < n_items && it[4 * at] == p) {
            const uint32_t first = it[4 * at + 1], end = it[4 * at + 2];
            if (first != covered || end <= first || end > target[p] || it[4 * at + 3] != 0u) return 1;
            if (S % rt::kSplitGrain == 0u) {
                if (first != done[p] && first % rt::kSplitGrain != 0u) return 1;
                if (end != target[p] && end % rt::kSplitGrain != 0u) return 1;
                if (end - first > S) return 1;
            }
            covered = end;
            ++at;
            ++n;
        }
        if (covered != target[p]) return 1;
        if (S % rt::kSplitGrain != 0u && n != (target[p] > done[p] ? 1u : 0u)) return 1;
    }
    return at == n_items ? 0 : 1;   // nothing out of pixel order, nothing left over
}

int main() {
    unsigned long long n = 0, waves = 0;
    long long slack = 0;
    int bad = 0;
    while (std::scanf("%llu %llu %lld", &n, &waves, &slack) == 3) {
        std::vector<uint32_t> done(n), target(n);
        for (size_t p = 0; p < n; ++p)
            if (std::scanf("%" SCNu32 " %" SCNu32, &done[p], &target[p]) != 2) return 2;
        uint32_t S = 0xDEADu;
        uint64_t count = 0xDEADu;
        int rc = rt::progressive_map_plan(n, done.data(), target.data(), (uint32_t)waves, &S, &count, nullptr, 0u);
        if (rc != rt::kPlanOk) {
            std::printf("%d %" PRIu32 " %" PRIu64 "\n", rc, S, count);
            continue;
        }
        const uint64_t cap = slack < 0 && (uint64_t)-slack > count ? 0u : count + slack;
        uint32_t* items = (uint32_t*)std::malloc(cap * 4u * sizeof(uint32_t) + 1u);   // exactly cap records
        uint32_t S2 = 0;
        uint64_t count2 = 0;
        rc = rt::progressive_map_plan(n, done.data(), target.data(), (uint32_t)waves, &S2, &count2, items, cap);
        if (S2 != S || count2 != count) bad = 1;
        std::printf("%d %" PRIu32 " %" PRIu64 "\n", rc, S2, count2);
        if (cap < count) {
            if (rc != rt::kPlanInvalid) bad = 1;
        } else if (rc != rt::kPlanOk || check_items(done, target, S, items, count)) {
            std::fprintf(stderr, "bad plan (rc %d)\n", rc);
            bad = 1;
        } else {
            for (uint64_t i = 0; i < count; ++i)
                std::printf("%" PRIu32 " %" PRIu32 " %" PRIu32 "\n", items[4 * i], items[4 * i + 1], items[4 * i + 2]);
        }
        std::free(items);
    }
    // refusals: outputs cleared, nothing dereferenced
    uint32_t S = 0xDEADu, one = 1u, two = 2u, big = rt::kSplitMaxSpp + 1u;
    uint64_t count = 0xDEADu;
    if (rt::progressive_map_plan(1, &one, &two, 8, nullptr, &count, nullptr, 0) != rt::kPlanInvalid) bad = 1;
    if (rt::progressive_map_plan(1, &one, &two, 8, &S, nullptr, nullptr, 0) != rt::kPlanInvalid) bad = 1;
    if (rt::progressive_map_plan(1, nullptr, &two, 8, &S, &count, nullptr, 0) != rt::kPlanInvalid || S || count) bad = 1;
    if (rt::progressive_map_plan(1, &one, nullptr, 8, &S, &count, nullptr, 0) != rt::kPlanInvalid) bad = 1;
    if (rt::progressive_map_plan(0, &one, &two, 8, &S, &count, nullptr, 0) != rt::kPlanInvalid) bad = 1;
    if (rt::progressive_map_plan(1, &two, &one, 8, &S, &count, nullptr, 0) != rt::kPlanInvalid || S || count) bad = 1;
    if (rt::progressive_map_plan(1, &one, &big, 8, &S, &count, nullptr, 0) != rt::kPlanUnsupported || S || count) bad = 1;
    if (rt::progressive_map_plan(rt::kSplitMaxItems + 1u, &one, &two, 8, &S, &count, nullptr, 0) != rt::kPlanUnsupported) bad = 1;
    return bad;
}
