// rt_trace.hpp — the persistent path-regeneration kernel trace_paths: work distribution (guided
// blocks through a workgroup pool), camera batches and their LDS queue, the per-iteration
// next-ray / sweep / terminate loop (TileRenderTask::render_vectorized2, renderer.rs:141-176).
#pragma once
#include "rt_sweep.hpp"
#include "rt_camera.hpp"
#include "rt_finish.hpp"

namespace rt {

// Wave-uniform issue state, parked in LDS between refills for the same reason.  Every word is read into an SGPR
// through a VALU instruction and written back through another, so the words are few and a call touches only the
// ones it needs: a batch served whole from the open item (issue()'s fast path) reads the first five, in two LDS
// reads, and writes cur_next alone.
//   flags: the small fields, kIS*: busy (slots with samples in flight), need (slots opened since their pixel's
//          camera candidate list was last built), nolist (slots whose pixel has no list, pixel_list's 0xFFFF: its
//          batches run camera_sweep), cur (the slot being issued), drained (no item left to claim)
//   q:     the camera queue, head | count << 16 (both <= kQCap)
struct alignas(16) IssueState { uint32_t cur_next, cur_pix, cur_row, cur_col, flags, q, blk_next, blk_end; };
// ... of the sample-parallel kernels (SPLIT): cur_end, the end of the item being issued (the others stop at spp)
struct alignas(16) IssueStateS { uint32_t cur_next, cur_pix, cur_row, cur_col, flags, q, blk_next, blk_end, cur_end; };
constexpr uint32_t kISBusy = 0, kISNeed = 8, kISNoList = 16, kISCur = 24;   // bit offsets in flags: 8, 8, 8 and 3 bits
constexpr uint32_t kISDrained = 1u << 27;
static_assert(kSlots <= 8u, "a slot mask is 8 bits of IssueState::flags, a slot index 3");

// Work items (pixels) are claimed in blocks.  One global counter counts blocks, and block j's items
// are a fixed function of j (guided_block): sizes G, G/2, ..., 2 while more than G T, ..., 2T items
// remain after it, then single items (T = kTMul x workgroups), so blocks shrink to one item towards
// the end without any wave estimating how much is left.  The claiming wave takes the block's first
// item and offers the rest to its workgroup through an LDS pool (s_pool, a lock-free 64-bit CAS;
// if another wave refilled the pool first, the claimer keeps the rest to itself).  Waves take items
// from their private rest, then the pool, then the counter.
//   * Global atomics are the cost: the device sustained ~90 M/s on this counter (11 ns each; spread
//     over 16 counters, no faster).  One atomic per pixel held config B (921 600 pixels) at 10.6 ms
//     whatever its spp.
//   * The tail is the other cost: a block is worked off by the 4 waves of one workgroup, and a late
//     16-pixel block of long glass paths at 512 spp, claimed by one wave, ran ~15 ms past the rest.
//     G (a power of two <= kMaxBlock, chosen per launch by the host) keeps a block within
//     kBlockSamples samples and within 1/kBlockShare of a wave's share of the pixels.  The second
//     bound is for small launches: 8-way row shards of C (~50 pixels per wave) with G = 16 ended
//     with one workgroup on 16 adjacent glass pixels, 8.2 ms against 5.7 ideal; with G = 2 they
//     scale perfectly.  Scattering the claim order instead (pixels or 16-pixel tiles) cost 4-5 % at
//     config C: waves on a CU then walk different clusters, and the sphere data thrash the scalar cache.
constexpr uint32_t kMaxBlock = 16;
constexpr uint32_t kBlockShare = 24;
// The counter serves ~90 M claims/s, and the chip runs ~3e10 samples/s: a launch claims at most one
// block per kClaimSpp samples (G >= kClaimSpp / spp), so claims stay under ~half the counter's rate
// at any spp.  Without it the share bound took small launches to single pixels: a quarter of config B
// (128 spp) then made 230 k claims, 2.5 ms of atomics for 1 ms of work (tools/multirank_check.sh).
constexpr uint32_t kClaimSpp = 640;
// The blocks past the first gridDim.x (one per workgroup, taken without an atomic) are dealt round-robin
// to kStreams claim streams, stream s holding blocks gridDim.x + s + kStreams c (c = 0, 1, ...) behind its
// own counter, kCtrStride words apart (256 B: separate lines and memory channels).  A workgroup claims
// from stream blockIdx.x % kStreams (the XCD the hardware dispatches it to), and from the others once its
// own runs dry, so the counters of a launch are not one word every CU hammers: the sky rows' cheap
// pixels otherwise claimed faster than one word serves (~88 claims/us).
constexpr uint32_t kStreams = 8;
constexpr uint32_t kCtrStride = 64;

// Block j of np items -> items [start, end); false past the last block.
__device__ __forceinline__ bool guided_block(uint32_t np, uint32_t T, uint32_t G, uint32_t j, uint32_t& start,
                                             uint32_t& end) {
    uint32_t a = 0;
#pragma unroll
    for (uint32_t sz = kMaxBlock; sz >= 1u; sz >>= 1) {
        const uint32_t r = np - a, keep = sz * T;
        const uint32_t len = sz == 1u ? r : (sz <= G && r > keep ? ((r - keep) / sz) * sz : 0u);
        const uint32_t nb = len / sz;
        if (j < nb) { start = a + j * sz; end = start + sz; return true; }
        j -= nb;
        a += len;
    }
    return false;
}

// Persistent path-regeneration kernel (see above).  Wave-uniform state: the slot being issued
// (cur, next sample cur_next), the busy-slot mask, and per-slot pixel/remaining-sample counts held
// in lane s of two VGPRs.  Per iteration: hand free lanes new samples, trace one bounce for every
// live ray (one sphere sweep for the whole wave), record terminations, finish completed pixels.
//
// CAMQ (pinhole cameras, depth >= 1): primary rays are not mixed into the per-lane sweep.  They are
// traced in full-wave camera batches against the camera-origin table (5 instead of 12 packed ops
// per sphere pair); misses terminate on the spot, hits wait in a per-wave LDS queue and free lanes
// pop them as rays whose bounce-0 scatter is pending.  Every ray still meets every sphere.
constexpr uint32_t kQCap = 128;   // camera-batch queue entries per wave (a batch adds at most 64)

// SPLIT (trace_paths_split, the sample-parallel path): a work item is a (pixel, sample
// sub-range), its records go to the launch-wide record buffer (PixelRegions) instead of the wave's slots (WaveSlots), and
// a completed slot is only freed: finish_records reduces every pixel in a launch of its own.
//
// The kernel's statements are in rt_trace_body.hpp, which each of the two kernels below includes as its
// body.  They are shared as text, not as a function both kernels call: with the body in a callee (inlined)
// every trace_paths instantiation compiled to different code than with the body in the kernel itself
// (tools/isa_diff.py), and the benched kernels are to stay as they are.
// kSplitKernel: SPLIT as a value that depends on T, so that `if constexpr (SPLIT)` discards the other
// kernel's statements instead of compiling them.
template <typename T, bool B> constexpr bool kSplitKernel = B;

template <typename T, int W, bool ROOT2, int MODE = kModeV2, bool CAMQ = false, bool MEGA = false>
__global__ __launch_bounds__(256, W) void trace_paths(KParams<T> p) {
    constexpr bool SPLIT = kSplitKernel<T, false>, WIN = kSplitKernel<T, false>, ITEMS = kSplitKernel<T, false>;
    constexpr bool RAYS = kSplitKernel<T, false>;
#include "rt_trace_body.hpp"
}

// The sample-parallel path's tracing kernel (rt_render_split_async): the live path with SPLIT, launched
// over (pixel, sample sub-range) items; finish_records follows it on the same stream.
template <typename T, int W, bool CAMQ, bool MEGA>
__global__ __launch_bounds__(256, W) void trace_paths_split(SParams<T> sp) {
    constexpr bool SPLIT = kSplitKernel<T, true>, WIN = kSplitKernel<T, false>, ITEMS = kSplitKernel<T, false>, ROOT2 = false;
    constexpr bool RAYS = kSplitKernel<T, false>;
    constexpr int MODE = kModeV2;
#include "rt_trace_body.hpp"
}

// A progressive session's tracing kernel (rt_progressive_extend_async): trace_paths_split with WIN, its items
// tiling the sample window [s_begin, spp) of every pixel, the regions laid out for the session's capacity
// (WParams).  Kernels of their own beside trace_paths_split, whose code, names and arguments stay as they were.
template <typename T, int W, bool CAMQ, bool MEGA>
__global__ __launch_bounds__(256, W) void trace_paths_window(WParams<T> wp) {
    constexpr bool SPLIT = kSplitKernel<T, true>, WIN = kSplitKernel<T, true>, ITEMS = kSplitKernel<T, false>, ROOT2 = false;
    constexpr bool RAYS = kSplitKernel<T, false>;
    constexpr int MODE = kModeV2;
#include "rt_trace_body.hpp"
}

// A session's tracing kernel over per-pixel sample counts (rt_progressive_extend_map_async): trace_paths_split
// with ITEMS.  A claimed item is a record {pixel, first, end} of the item table, so every pixel has its own
// window; the claim scheme and the records are trace_paths_window's.  A kernel of its own beside
// trace_paths_window, whose code, name and arguments stay as they were.
template <typename T, int W, bool CAMQ, bool MEGA>
__global__ __launch_bounds__(256, W) void trace_paths_items(IParams<T> ip) {
    constexpr bool SPLIT = kSplitKernel<T, true>, WIN = kSplitKernel<T, false>, ITEMS = kSplitKernel<T, true>, ROOT2 = false;
    constexpr bool RAYS = kSplitKernel<T, false>;
    constexpr int MODE = kModeV2;
#include "rt_trace_body.hpp"
}

// The sample-parallel path's finish: waves stride over the pixels of the set and run finish_pixel on each
// pixel's region of the record buffer, which the trace kernel filled in the launch before this one (the
// kernel boundary is the only hand-off: nothing is read that this launch's other workgroups wrote).  The
// position map is in LDS up to kLMapCap positions, else in the wave's area of the scratch.  Each pixel's K
// goes to the bounce-iteration counter, as trace_paths adds it.
// The statements of the three kernels below, shared as text like rt_trace_body.hpp and for its reason: called
// as an inlined function they compiled to the same instructions in another order (tools/isa_diff.py).  In scope:
//   WINDOW: the regions are laid out for a session's capacity, P_cap (WParams), not for the count in the KParams
//   LIST:   the pixels are list[0 .. n_pix) (LParams), not 0 .. n_pix
#define RT_FINISH_BODY                                                                                              \
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[4][64];                                                 \
    __shared__ __attribute__((aligned(16))) T s_stage[4][3][64];                                                    \
    __shared__ __attribute__((aligned(16))) uint16_t s_lmap[4][kLMapCap > 0u ? kLMapCap : 2];                       \
    const uint32_t lane = threadIdx.x & 63u;                                                                        \
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);                                         \
    const auto& q = *cold<SParams<T>>();                                                                            \
    const uint32_t gw = blockIdx.x * 4u + wave, nw = gridDim.x * 4u;                                                \
    const PixelRegions<T> sc{q.k.scratch + (size_t)gw * q.k.scratch_stride, q.rec,                                  \
                             WINDOW ? cold<WParams<T>>()->P_cap : q.k.P, 0u, q.k.sbytes, q.k.swide};                \
    const uint32_t n_pix = q.n_pix;                                                                                 \
    const cptr<uint32_t> list = LIST ? (cptr<uint32_t>)cold<LParams<T>>()->list : nullptr;                          \
    unsigned long long iters = 0;                                                                                   \
    for (uint64_t i = gw; i < n_pix; i += nw) {                                                                     \
        const uint32_t px = LIST ? list[i] : (uint32_t)i; /* the region and the output element are pixel px's */    \
        iters += finish_pixel<T, kModeV2, true>(sc, px, px, s_hist[wave], s_stage[wave],                            \
                                                kLMapCap > 0u ? s_lmap[wave] : nullptr, false);                     \
        __builtin_amdgcn_wave_barrier();                                                                            \
    }                                                                                                               \
    if (lane == 0 && iters != 0ull) atomicAdd(&q.k.segs[(gw & (kSegShards - 1)) * kSegStride + 2], iters);

// finish_records: every pixel of a rt_render_split_async launch, after trace_paths_split.
template <typename T>
__global__ __launch_bounds__(256) void finish_records(SParams<T> sp) {
    constexpr bool WINDOW = false, LIST = false;
    RT_FINISH_BODY
}

// A session's snapshot: finish_records over the prefix [0, spp) of regions laid out for P_cap positions.  The
// counts (spp, P, C, s_sel, the map's width and bytes) in the KParams are the snapshot's, which finish_pixel
// reads as ever; only the record view's stride is the capacity's.  Samples at and past spp, traced by an
// earlier, longer extend or not at all, are never read.
template <typename T>
__global__ __launch_bounds__(256) void finish_window(WParams<T> wp) {
    constexpr bool WINDOW = true, LIST = false;
    RT_FINISH_BODY
}

// finish_window over an index list: the pixels of a session that are reduced at the same count (the counts in
// the KParams, as finish_window reads them), one launch per distinct count of a per-pixel map.
template <typename T>
__global__ __launch_bounds__(256) void finish_window_list(LParams<T> lp) {
    constexpr bool WINDOW = true, LIST = true;
    RT_FINISH_BODY
}
#undef RT_FINISH_BODY

// A session's error estimate (rt_progressive_error_async): per pixel the largest channel difference between the
// linear snapshot at its count and at half its count, both already in device memory as doubles; +inf below 2
// samples.
__global__ __launch_bounds__(256) void progressive_error(const double* full, const double* half,
                                                         const uint32_t* counts, double* out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    double e = __builtin_huge_val();
    if (counts[i] >= 2u) {
        e = 0.0;
        for (uint32_t ch = 0; ch < 3u; ++ch) e = fmax(e, fabs(full[3u * i + ch] - half[3u * i + ch]));
    }
    out[i] = e;
}

// ---- rt_progressive_refine: the selection of one refinement step, on the device ----
// The candidates of a step are the n pixels list[0 .. n) (list NULL: pixel i itself), in ascending pixel order,
// all at `count` samples.  Their linear values at `count` are in `fresh`, the values at count / 2 in `cur`.  Four
// launches, each reading only what an earlier launch wrote (the kernel boundary is the hand-off, as between the
// trace and finish kernels): refine_select (estimate, flag, count of active per block of kRefineBlock
// candidates), refine_scan (one workgroup: exclusive scan of the block counts), refine_scatter (stable
// compaction into the next active list and the list of the pixels that stop at `count`), refine_expand (the
// active list into the item table trace_paths_items reads).
constexpr uint32_t kRefineBlock = 256;

// Exclusive prefix of one value per thread over a 256-thread workgroup; *total: the workgroup's sum.
__device__ inline uint32_t refine_block_scan(uint32_t v, uint32_t* buf, uint32_t* total) {
    const uint32_t t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kRefineBlock; d <<= 1) {
        const uint32_t a = t >= d ? buf[t - d] : 0u;
        __syncthreads();
        buf[t] += a;
        __syncthreads();
    }
    const uint32_t incl = buf[t];
    *total = buf[kRefineBlock - 1];
    __syncthreads();   // the buffer may be written again
    return incl - v;
}

// Candidate i: progressive_error's estimate (+inf below 2 samples), fresh moved into cur, counts[p] = count,
// flags[i] = the estimate is above tol (a NaN is not) and the pixel may still grow; blk[block] = the block's
// active candidates.
__global__ __launch_bounds__(256) void refine_select(const uint32_t* list, uint32_t n, uint32_t count, double tol,
                                                     uint32_t may_grow, double* cur, const double* fresh,
                                                     uint32_t* counts, uint8_t* flags, uint32_t* blk) {
    __shared__ uint32_t s_buf[kRefineBlock];
    const uint32_t i = blockIdx.x * kRefineBlock + threadIdx.x;
    uint32_t act = 0u;
    if (i < n) {
        const size_t p = list ? list[i] : i;
        double e = __builtin_huge_val();
        if (count >= 2u) {
            e = 0.0;
            for (uint32_t ch = 0; ch < 3u; ++ch) e = fmax(e, fabs(fresh[3u * p + ch] - cur[3u * p + ch]));
        }
        for (uint32_t ch = 0; ch < 3u; ++ch) cur[3u * p + ch] = fresh[3u * p + ch];
        act = (e > tol && may_grow != 0u) ? 1u : 0u;
        counts[p] = count;
        flags[i] = (uint8_t)act;
    }
    uint32_t total = 0u;
    (void)refine_block_scan(act, s_buf, &total);
    if (threadIdx.x == 0u) blk[blockIdx.x] = total;
}

// blk[0 .. nb): the block counts, replaced by their exclusive prefix sums; ret[0] = their sum (ret: 4 words).
__global__ __launch_bounds__(256) void refine_scan(uint32_t* blk, uint32_t nb, uint32_t* ret) {
    __shared__ uint32_t s_buf[kRefineBlock];
    uint32_t carry = 0u;   // the same in every thread
    for (uint32_t base = 0; base < nb; base += kRefineBlock) {
        const uint32_t idx = base + threadIdx.x;
        const uint32_t v = idx < nb ? blk[idx] : 0u;
        uint32_t total = 0u;
        const uint32_t ex = refine_block_scan(v, s_buf, &total);
        if (idx < nb) blk[idx] = carry + ex;
        carry += total;
    }
    if (threadIdx.x < 4u) ret[threadIdx.x] = threadIdx.x == 0u ? carry : 0u;
}

// Stable compaction: the active candidates to next[0 .. A), the others to retired[0 .. n - A), both in candidate
// (ascending pixel) order.  off: refine_scan's prefix sums.
__global__ __launch_bounds__(256) void refine_scatter(const uint32_t* list, uint32_t n, const uint8_t* flags,
                                                      const uint32_t* off, uint32_t* next, uint32_t* retired) {
    __shared__ uint32_t s_buf[kRefineBlock];
    const uint32_t first = blockIdx.x * kRefineBlock, i = first + threadIdx.x;
    const uint32_t act = i < n ? (uint32_t)flags[i] : 0u;
    uint32_t total = 0u;
    const uint32_t rank = refine_block_scan(act, s_buf, &total);
    if (i >= n) return;
    const uint32_t p = list ? list[i] : i;
    const uint32_t a0 = off[blockIdx.x];           // active candidates before this block: a0 <= first
    if (act) next[a0 + rank] = p;                  // < A <= n
    else retired[(first - a0) + (threadIdx.x - rank)] = p;   // < n - A
}

// The item table of the step: active pixel i gets nsub records {pixel, first, end, 0}, the samples
// [max(done, base + j S), min(target, base + (j + 1) S)) (prog_item, rt_progressive_plan.hpp), and its count
// becomes target.
__global__ __launch_bounds__(256) void refine_expand(const uint32_t* act, uint32_t n_act, uint32_t* counts,
                                                     uint32_t done, uint32_t target, uint32_t base, uint32_t S,
                                                     uint32_t nsub, MapItem* items) {
    const uint32_t i = blockIdx.x * kRefineBlock + threadIdx.x;
    if (i >= n_act) return;
    const uint32_t p = act[i];
    counts[p] = target;
    for (uint32_t j = 0; j < nsub; ++j) {
        const uint32_t a = base + j * S, b = a + S;
        items[(size_t)i * nsub + j] = MapItem{p, a > done ? a : done, b < target ? b : target, 0u};
    }
}

}  // namespace rt
