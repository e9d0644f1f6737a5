// rt_list.hpp — ray lists: path steps over the live rays only, and the next list left on the device
// (rt_path_step_list_async, rt_ray_list_compact_async).  A list is uint32 ray ids list[n] plus a device word count; the
// ray arrays stay where they are and are indexed by ray id, only the list shrinks.
//   * path_step_list<T, ROOT2, MEGA>: path_step_rays' batch loop with one indirection.  Batch b is list positions
//     64 b .. 64 b + 63, the lane's ray is list_in[64 b + lane] (the position itself without a list); count is read
//     once at kernel entry, wave-uniform, so a wave whose first batch is past it returns at once.  Per listed ray it is
//     path_step_rays' body restated (that kernel's code stays as it was measured); nothing is written at a ray that is
//     not listed.  After the scatter lane 0 stores the batch's survivor ballot, one 64-bit word per batch.
//   * keep_ballots: the same words from the caller's mask, keep[list_in[i]] != 0 (rt_ray_list_compact_async).
//   * the compaction, stable in list position: list_tile_sums (per tile of `tile` rays the popcount of its ballots),
//     list_scan_tiles (one workgroup: the exclusive scan of the tile sums in chunks of kListScanChunk, and *count_out),
//     list_scatter (a wave per batch: its offset is its tile's plus the popcounts of the tile's batches before it; the
//     set lanes write list_out[off + rank]).  Three launches order the three levels: no workgroup waits for another.
// Every level bounds itself by count (the batches below ceil(count / 64); the producers clear the lanes at and past
// count in the last one), so the stale words a longer list left in the ballot scratch are never read.  A list entry
// >= n and a count > n (clamped) raise word 1 of the error flags; no kernel reads or writes outside its arrays for
// any list contents.  Offsets are 32-bit: a list holds at most 0x7FFFFFFF rays.
#pragma once
#include "rt_step.hpp"

namespace rt {

constexpr uint32_t kListTileDefault = 65536u;   // rays per tile (RT_LIST_TILE: 64 .. 65536, a power of two)
constexpr uint32_t kListScanChunk = 256u;       // tiles list_scan_tiles scans at once: its workgroup's threads

// Arguments of path_step_list: path_step_rays' (s.k.n_items: the capacity n of the ray arrays), then the list.
template <typename T> struct PlParams {
    PsParams<T> s;
    const uint32_t* list_in;       // [n]; NULL: the identity list
    const uint32_t* count_in;      // one word; NULL: n
    unsigned long long* ballots;   // [ceil(n / 64)]: bit l of word b: list position 64 b + l scattered; NULL: not written
};

// Arguments of the compaction kernels.
struct LcParams {
    uint32_t n;                    // capacity: ray ids and the count lie below it
    uint32_t tile_batches;         // batches per tile, a power of two
    const uint32_t* list_in;       // NULL: the identity list
    const uint32_t* count_in;      // NULL: n
    const uint8_t* keep;           // keep_ballots: [n], by ray id
    unsigned long long* ballots;   // [ceil(n / 64)]
    uint32_t* tiles;               // [tiles of n]: the sums, then their exclusive scan
    uint32_t* list_out;            // [n]
    uint32_t* count_out;
    uint32_t* err;                 // the context's error words
};

// The list's count: the word at count_in (NULL: n), clamped to n; over: it was above n.  Wave-uniform.
__device__ __forceinline__ uint32_t list_count(const uint32_t* count_in, uint32_t n, bool& over) {
    uint32_t c = n;
    if (count_in) c = __builtin_amdgcn_readfirstlane(*count_in);
    over = c > n;
    return over ? n : c;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

template <typename T, bool ROOT2, bool MEGA>
__global__ __launch_bounds__(256, kWavesQuery<T>) void path_step_list(PlParams<T> lp) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (lane < kNWork) g_work[wave][lane] = 0ull;
#ifdef RT_KSTATS
    if (lane < kNKstat) g_kst[wave][lane] = 0;
#endif
    const uint32_t gw = blockIdx.x * 4u + wave, nw = gridDim.x * 4u;
    const uint32_t n = cold_args<T>()->n_items;   // <= 0x7FFFFFFF rays
    bool any_bad = false;
    const uint32_t count = list_count(lp.count_in, n, any_bad);
    const uint32_t n_batches = (count + 63u) / 64u;   // <= 2^25: batch + nw does not wrap
    unsigned long long n_seg = 0, n_slots = 0;
    for (uint32_t batch = gw; batch < n_batches; batch += nw) {
        const uint32_t pos = batch * 64u + lane;   // <= 0x7FFFFFFF + 63
        const bool listed = pos < count;
        uint32_t ray = pos;
        // the list's two pointers are read through cold() where they are used: as plain arguments they are loaded at
        // the kernel's entry in one 16-dword block with the step's outputs, and the block's spill slot stays reserved
        // (68 bytes of scratch per lane that no instruction touches)
        const uint32_t* lin = cold<PlParams<T>>()->list_in;
        if (listed && lin) ray = lin[pos];
        const bool in = listed && ray < n;   // an entry outside the arrays is skipped
        any_bad = any_bad || (listed && !in);
        V3<T> o = mk(T(0), T(0), T(0)), d = o;
        if (in) {
            const T* dp = lp.s.directions + (size_t)3 * ray;
            d = mk(dp[0], dp[1], dp[2]);
            const T* op = lp.s.origins + (size_t)3 * ray;
            o = mk(op[0], op[1], op[2]);
        }
        const T a = pk_len2(d);
        const bool v = in && query_finite(o) && query_finite(d) && a >= kQueryLen2Min<T> && a <= kQueryLen2Max<T>;
        const unsigned long long vm = __ballot(v);
        T t = T(INFINITY);
        int hi = -1;
        if (vm != 0ull) {   // wave-uniform
            if (v) hi = nearest_hit<T, ROOT2, false, MEGA>(o, d, t);
            n_slots += 64u;
            n_seg += (unsigned long long)__builtin_popcountll(vm);
        }
        const bool hit = v && hi >= 0;
        if (hit) {
            // the query's outputs of the hit that is scattered, as path_step_rays has them
            const auto& q = *cold_args<T>();
            const T* sgp = q.cen + 4 * hi;
            const V3<T> hcen = mk(sgp[0], sgp[1], sgp[2]);
            const V3<T> loc = mk(o.x + d.x * t, o.y + d.y * t, o.z + d.z * t);   // at_t
            const V3<T> vec = sub(loc, hcen);
            const V3<T> u = dvs(vec, sqrt_len(pk_len2(vec)));
            const bool front = pk_dot(d, u) < T(0.0);
            const V3<T> nrm = front ? u : neg(u);
            if (lp.s.normal) {
                T* np = lp.s.normal + (size_t)3 * ray;
                np[0] = nrm.x; np[1] = nrm.y; np[2] = nrm.z;
            }
            if (lp.s.front) lp.s.front[ray] = front ? 1u : 0u;
        } else if (in) {
            if (lp.s.normal) {
                T* np = lp.s.normal + (size_t)3 * ray;
                np[0] = T(0); np[1] = T(0); np[2] = T(0);
            }
            if (lp.s.front) lp.s.front[ray] = 0u;
        }
        if (in) {
            if (lp.s.t) lp.s.t[ray] = v ? (hit ? t : T(INFINITY)) : T(NAN);
            if (lp.s.index) lp.s.index[ray] = v ? (hit ? hi : -1) : kQueryInvalid;
        }
        bool bad = false;
        const bool go = hit && step_scatters(hi, lp.s.sample[ray], cold_args<T>()->n_spheres, bad);
        any_bad = any_bad || bad;
        if (go) {
            V3<T> c = mk(T(1.0), T(1.0), T(1.0));
            if (lp.s.colour) {
                const T* cp = lp.s.colour + (size_t)3 * ray;
                c = mk(cp[0], cp[1], cp[2]);
            }
            next_ray<T, false>(false, 0u, 0u, lp.s.pixel[ray], lp.s.sample[ray], lp.s.bounce, hi, t, o, d, c);
            T* op = lp.s.origins + (size_t)3 * ray;
            op[0] = o.x; op[1] = o.y; op[2] = o.z;
            T* dp = lp.s.directions + (size_t)3 * ray;
            dp[0] = d.x; dp[1] = d.y; dp[2] = d.z;
            if (lp.s.colour) {
                T* cp = lp.s.colour + (size_t)3 * ray;
                cp[0] = c.x; cp[1] = c.y; cp[2] = c.z;
            }
        }
        if (in && lp.s.status) lp.s.status[ray] = v ? (go ? kStepScattered : kStepMissed) : kStepInvalid;
        const unsigned long long gm = __ballot(go);   // the survivors, by list position
        unsigned long long* bal = cold<PlParams<T>>()->ballots;
        if (bal && lane == 0) bal[batch] = gm;
    }
    const unsigned long long bm = __ballot(any_bad);
    if (lane == 0) {
        const auto& q = *cold_args<T>();
        unsigned long long* cc = &q.segs[(gw & (kSegShards - 1)) * kSegStride];
        if (n_seg) {
            atomicAdd(cc + 0, n_seg);
            atomicAdd(cc + kQuerySlot, n_seg);
        }
        if (n_slots) atomicAdd(cc + 1, n_slots);
        if (bm) atomicOr(q.err + 1, 1u);
        for (uint32_t i = 0; i < kNWork; ++i)
            if (g_work[wave][i]) atomicAdd(cc + kWorkSlot + i, g_work[wave][i]);
#ifdef RT_KSTATS
        for (int i = 0; i < kNKstat; ++i) atomicAdd(cc + kstat_slot(i), g_kst[wave][i]);
#endif
    }
}

// The compaction call's producer: a wave per batch, word b = the ballot of keep[list_in[64 b + lane]] != 0.
__global__ __launch_bounds__(256) void keep_ballots(LcParams p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gw = blockIdx.x * 4u + (threadIdx.x >> 6), nw = gridDim.x * 4u;
    bool any_bad = false;
    const uint32_t count = list_count(p.count_in, p.n, any_bad);
    const uint32_t n_batches = (count + 63u) / 64u;
    for (uint32_t batch = gw; batch < n_batches; batch += nw) {
        const uint32_t pos = batch * 64u + lane;
        const bool listed = pos < count;
        uint32_t ray = pos;
        if (listed && p.list_in) ray = p.list_in[pos];
        const bool in = listed && ray < p.n;
        any_bad = any_bad || (listed && !in);
        const unsigned long long km = __ballot(in && p.keep[ray] != 0u);
        if (lane == 0) p.ballots[batch] = km;
    }
    if (__ballot(any_bad) != 0ull && lane == 0) atomicOr(p.err + 1, 1u);
}

// Level 1: tiles[t] = the survivors of tile t, a workgroup per tile (the workgroups stride over the list's tiles).
__global__ __launch_bounds__(256) void list_tile_sums(LcParams p) {
    __shared__ uint32_t part[4];
    bool over = false;
    const uint32_t count = list_count(p.count_in, p.n, over);
    const uint32_t n_batches = (count + 63u) / 64u;
    const uint32_t n_tiles = (n_batches + p.tile_batches - 1u) / p.tile_batches;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t b0 = tile * p.tile_batches;   // < n_batches <= 2^25
        const uint32_t b1 = min(b0 + p.tile_batches, n_batches);
        uint32_t acc = 0;
        for (uint32_t b = b0 + threadIdx.x; b < b1; b += 256u) acc += (uint32_t)__builtin_popcountll(p.ballots[b]);
        acc = wave_sum(acc);
        if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) p.tiles[tile] = part[0] + part[1] + part[2] + part[3];
        __syncthreads();
    }
}

// Level 2, one workgroup of kListScanChunk threads: tiles[] becomes its exclusive scan, kListScanChunk tiles at a time
// with the running total carried from chunk to chunk, and *count_out the total.
__global__ __launch_bounds__(kListScanChunk) void list_scan_tiles(LcParams p) {
    __shared__ uint32_t part[kListScanChunk / 64u];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    bool over = false;
    const uint32_t count = list_count(p.count_in, p.n, over);
    const uint32_t n_batches = (count + 63u) / 64u;
    const uint32_t n_tiles = (n_batches + p.tile_batches - 1u) / p.tile_batches;
    uint32_t carry = 0;   // the same in every thread
    for (uint32_t c0 = 0; c0 < n_tiles; c0 += kListScanChunk) {
        const uint32_t i = c0 + threadIdx.x;
        const uint32_t own = i < n_tiles ? p.tiles[i] : 0u;
        uint32_t inc = own;   // inclusive scan over the wave
        for (int s = 1; s < 64; s <<= 1) {
            const uint32_t up = __shfl_up(inc, s, 64);
            if (lane >= (uint32_t)s) inc += up;
        }
        if (lane == 63u) part[wave] = inc;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < kListScanChunk / 64u; ++w) {
            before += w < wave ? part[w] : 0u;
            total += part[w];
        }
        if (i < n_tiles) p.tiles[i] = carry + before + inc - own;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *p.count_out = carry;
}

// Level 3: a wave per batch with a survivor.  Its offset: the tile's, plus the popcounts of the tile's batches before
// it; lane l of the ballot writes at its rank among the set lanes, so list_out keeps the order of the list positions.
__global__ __launch_bounds__(256) void list_scatter(LcParams p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gw = blockIdx.x * 4u + (threadIdx.x >> 6), nw = gridDim.x * 4u;
    bool over = false;
    const uint32_t count = list_count(p.count_in, p.n, over);
    const uint32_t n_batches = (count + 63u) / 64u;
    for (uint32_t batch = gw; batch < n_batches; batch += nw) {
        const unsigned long long m = p.ballots[batch];   // wave-uniform
        if (m == 0ull) continue;
        const uint32_t tile = batch / p.tile_batches;
        uint32_t acc = 0;
        for (uint32_t b = tile * p.tile_batches + lane; b < batch; b += 64u) acc += (uint32_t)__builtin_popcountll(p.ballots[b]);
        const uint32_t off = p.tiles[tile] + wave_sum(acc);
        const uint32_t pos = batch * 64u + lane;
        if (((m >> lane) & 1ull) && pos < count) {   // the producers clear the lanes at and past count themselves
            const uint32_t ray = p.list_in ? p.list_in[pos] : pos;
            const uint32_t dst = off + lanes_below(m);
            if (dst < p.n) p.list_out[dst] = ray;   // always, for ballots and sums of one count
        }
    }
}

}  // namespace rt
