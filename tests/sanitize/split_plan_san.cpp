// AddressSanitizer + UBSan harness of the sample-parallel plan (csrc/rt_split_plan.hpp, pure host C++).
// stdin: triples "n_pixels spp resident_waves"; stdout: one line "rc S n_items" per triple.  Each plan is
// also checked here (cover, grain, item count), so a violation exits non-zero even without a report.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "../../rust-ray-tracing_amd/csrc/rt_split_plan.hpp"

int main() {
    unsigned long long np = 0, spp = 0, waves = 0;
    int bad = 0;
    while (std::scanf("%llu %llu %llu", &np, &spp, &waves) == 3) {
        uint32_t S = 0xDEADu;
        uint64_t items = 0xDEADu;
        const int rc = rt::split_plan((uint64_t)np, (uint32_t)spp, (uint32_t)waves, &S, &items);
        std::printf("%d %" PRIu32 " %" PRIu64 "\n", rc, S, items);
        if (rc != rt::kPlanOk) {
            if (S != 0 || items != 0) { std::fprintf(stderr, "outputs not cleared on rc %d\n", rc); bad = 1; }
            continue;
        }
        const uint32_t nsub = rt::split_nsub((uint32_t)spp, S);
        // the items of a pixel cover [0, spp) exactly once: item j holds [j S, min(spp, (j + 1) S))
        uint64_t covered = 0;
        for (uint32_t j = 0; j < nsub; ++j) {
            const uint64_t b = (uint64_t)j * S, e = b + S < spp ? b + S : spp;
            if (b != covered || e <= b) { std::fprintf(stderr, "gap at item %u\n", j); bad = 1; break; }
            covered = e;
        }
        if (covered != spp) { std::fprintf(stderr, "cover %llu of %llu\n", (unsigned long long)covered, spp); bad = 1; }
        if (items != (uint64_t)np * nsub || items > rt::kSplitMaxItems) { std::fprintf(stderr, "item count\n"); bad = 1; }
        if (nsub > 1 && S % rt::kSplitGrain != 0) { std::fprintf(stderr, "grain\n"); bad = 1; }
    }
    // NULL outputs are refused, not written
    uint32_t S = 0;
    uint64_t items = 0;
    if (rt::split_plan(1, 1, 1, nullptr, &items) != rt::kPlanInvalid) bad = 1;
    if (rt::split_plan(1, 1, 1, &S, nullptr) != rt::kPlanInvalid) bad = 1;
    return bad;
}
