// rt_session.hpp — a context's progressive session (rt_progressive_*), host only: its state
// (Session), its own launchers (launch_items, launch_classes) and its work: the uniform extend (extend_uniform),
// the per-pixel-count calls (run_map), a run's snapshot (snapshot_run) and one step of a refinement run on the
// device (refine_step and the steps it names).
#pragma once
#include "rt_launch.hpp"

namespace rt {

static_assert(sizeof(MapItem) == kMapItemWords * sizeof(uint32_t), "the plan's records are the kernel's");

// What rt_progressive_begin fixed, the samples each pixel's region holds so far (done, in the range's compact
// order; done_min == done_max: a uniform session), and the record buffer, which only the session's launches
// touch.  The per-pixel-count calls send their tables (the item table, the classes' index lists, the counts)
// through stage into tables, and the error estimate keeps its two linear snapshots in lin_full and lin_half.
struct Session {
    bool open = false;
    rt_camera cam{};
    rt_tile_range rg{};
    uint32_t depth = 0, cap = 0, flags = 0, done_min = 0, done_max = 0;
    std::vector<uint32_t> done;
    uint64_t seed = 0;
    DeviceBuffer rec;
    hipStream_t stream = nullptr;   // of the last call that enqueued work
    bool have_stream = false;
    PinnedStage stage;
    DeviceBuffer tables, lin_full, lin_half;
    bool f32() const { return (flags & RT_FLAG_F32) != 0; }
    uint32_t n_pix() const { return rg.row_count * rg.col_count; }
    void touch(hipStream_t st) { stream = st; have_stream = true; }
    void refresh_bounds() {
        done_min = *std::min_element(done.begin(), done.end());
        done_max = *std::max_element(done.begin(), done.end());
    }
    void set_done(uint32_t n) { std::fill(done.begin(), done.end(), n); done_min = done_max = n; }
    // The refinement run (rt_progressive_refine; one per session): its tolerance and cap, the candidates of the
    // next step (the n_cand pixels of act[cur], all at n_k samples; the run's first step takes every pixel),
    // the classes of the pixels that stopped (spp, first, n: their pixels are cls_list[first .. first + n) on
    // the device), and the last step's plan.  While a run is unbroken the device array counts is what the
    // pixels hold, and done_stale says that `done` has not been copied down since the last step.
    struct Refine {
        bool started = false, broken = false;
        double tol = 0.0;
        uint32_t spp_max = 0, n_k = 0, n_cand = 0, cls_used = 0, S = 0;
        int cur = 0;
        uint64_t n_items = 0;
        std::vector<CountClass> cls;
    } run;
    bool done_stale = false;
    DeviceBuffer counts, act[2], cls_list, sel, blk, ret, items, lin_cur, lin_new;
};

// The session's frame at `spp` samples with the given outputs.
static FrameArgs session_frame(const Session& s, uint32_t spp, void* rgb, void* lin) {
    return FrameArgs{&s.cam, s.depth, spp, s.seed, s.flags, s.rg, rgb, lin};
}

// Send the first `bytes` of the session's staging buffer to its device tables, on st.
static int send_tables(Session& s, size_t bytes, hipStream_t st) {
    const int rc = ensure_bytes(s.tables, bytes, st);
    if (rc != RT_OK) return rc;
    HIPCHK(hipMemcpyAsync(s.tables.p, s.stage.p, bytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(s.stage.ev, st));
    s.stage.pending = true;
    return RT_OK;
}

// After a step of a refinement run the counts are on the device: copy them down (4 bytes per pixel) before
// a call reads `done`.
static int sync_done(LaunchContext* c, Session& s) {
    if (!s.done_stale) return RT_OK;
    HIPCHK(hipSetDevice(c->device));
    if (s.have_stream) HIPCHK(hipStreamSynchronize(s.stream));
    HIPCHK(hipMemcpy(s.done.data(), s.counts.p, s.done.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    s.refresh_bounds();
    s.done_stale = false;
    return RT_OK;
}

// ---- the session's launchers ----
// trace_paths_items over the n_items records at `items` (device), item_spp samples each on average.
template <typename T>
static int launch_items(LaunchContext* c, const Session& s, const MapItem* items, uint32_t n_items, uint32_t item_spp,
                        hipStream_t st) {
    KParams<T> p;
    bool camq = false;
    int rc = frame_setup(c, session_frame(s, s.cap, nullptr, nullptr), 1u, st, p, camq);
    if (rc != RT_OK) return rc;
    const SplitPick<T> pick = pick_split<T>(camq, p.n_mg > 0);
    void (*const ifn)(IParams<T>) = pick_items<T>(camq, p.n_mg > 0);
    p.n_items = n_items;
    uint64_t nblocks = 0;
    rc = plan_grid(c, (const void*)ifn, pick.W, pick.id | kKernelItemsBit, n_items, item_spp, nblocks, p.blk_g);
    if (rc != RT_OK) return rc;
    // the records' strides are the capacity's (frame_setup laid the frame out for s.cap); the trace kernels read
    // no sample count from the arguments: every item carries its own
    IParams<T> ip;
    memset(&ip, 0, sizeof(ip));
    ip.w.s.k = p;
    ip.w.s.rec = (char*)s.rec.p;
    ip.w.s.n_pix = s.n_pix();
    ip.w.P_cap = p.P;
    ip.items = items;
    if ((rc = zero_claim_counters(c, st)) != RT_OK) return rc;
    hipLaunchKernelGGL(ifn, dim3((uint32_t)nblocks), dim3(256), 0, st, ip);
    HIPCHK(hipGetLastError());
    return RT_OK;
}

// finish_window_list once per class, over the classes' index lists at `list` (device).  set_id: no trace kernel
// ran in this call, so the kernel id is the session's sample-parallel kernels' without RT_KERNEL_ITEMS.
template <typename T>
static int launch_classes(LaunchContext* c, const Session& s, const std::vector<CountClass>& cls, const uint32_t* list,
                          void* rgb, void* lin, bool set_id, hipStream_t st) {
    const uint32_t P_cap = prog_positions(s.cap);
    // the scratch (one position map per wave) for the largest class, before the first launch reads it
    uint64_t need = 0;
    for (const CountClass& k : cls) {
        const uint32_t P = prog_positions(k.spp), vb = paths_vbytes(P, paths_wide(P, s.depth), false);
        need = std::max<uint64_t>(need, (uint64_t)vb * finish_grid(c, k.n, vb) * 4u);
    }
    int rc = ensure_bytes(c->scratch, need, st);
    if (rc != RT_OK) return rc;
    for (const CountClass& k : cls) {
        KParams<T> p;
        bool camq = false;
        if ((rc = frame_setup(c, session_frame(s, k.spp, rgb, lin), 1u, st, p, camq)) != RT_OK) return rc;
        if (set_id) {
            const SplitPick<T> pick = pick_split<T>(camq, p.n_mg > 0);
            uint64_t nb = 0;
            uint32_t g = 0;
            rc = plan_grid(c, (const void*)pick_window<T>(camq, p.n_mg > 0), pick.W, pick.id, p.n_items, 1u, nb, g);
            if (rc != RT_OK) return rc;
            set_id = false;
        }
        p.sbytes = paths_sbytes(P_cap, sizeof(T), p.swide);   // a region's size: the capacity's (launch_window)
        LParams<T> lp;
        memset(&lp, 0, sizeof(lp));
        uint64_t fblocks = 0;
        if ((rc = split_params(c, p, (char*)s.rec.p, 1u, 1u, k.n, st, lp.w.s, fblocks)) != RT_OK) return rc;
        lp.w.P_cap = P_cap;
        lp.list = list + k.first;
        hipLaunchKernelGGL(finish_window_list<T>, dim3((uint32_t)fblocks), dim3(256), 0, st, lp);
        HIPCHK(hipGetLastError());
    }
    return RT_OK;
}

// The launchers at the session's precision.  reduce_uniform: finish_window over every pixel of the session at
// `spp` samples into lin (no tracing).
static int trace_items(LaunchContext* c, const Session& s, const MapItem* items, uint32_t n_items, uint32_t item_spp,
                       hipStream_t st) {
    return with_precision(s.f32(), [&](auto t) { return launch_items<decltype(t)>(c, s, items, n_items, item_spp, st); });
}
static int reduce_classes(LaunchContext* c, const Session& s, const std::vector<CountClass>& cls, const uint32_t* list,
                          void* rgb, void* lin, bool set_id, hipStream_t st) {
    return with_precision(s.f32(), [&](auto t) { return launch_classes<decltype(t)>(c, s, cls, list, rgb, lin, set_id, st); });
}
static int reduce_uniform(LaunchContext* c, const Session& s, uint32_t spp, void* lin, hipStream_t st) {
    const SessionWindow w{(char*)s.rec.p, s.cap, spp, spp, 1u, 1u, false, true};
    const FrameArgs a = session_frame(s, spp, nullptr, lin);
    return with_precision(s.f32(), [&](auto t) { return launch_window<decltype(t)>(c, a, w, st); });
}

// ---- extends and snapshots ----
// An extend of a session whose pixels all hold s.done_min samples, to spp_total for every pixel:
// rt_progressive_extend_async, and a map that is uniform.
static int extend_uniform(LaunchContext* c, Session& s, const std::string& who, uint32_t spp_total, void* d_rgb8,
                          void* d_linear, void* stream) {
    const uint32_t done = s.done_min;
    if (spp_total == 0) return fail(RT_ERR_INVALID, who + ": spp_total == 0");
    if (spp_total < done) return fail(RT_ERR_INVALID, who + ": spp_total below the samples already traced");
    if (spp_total > s.cap) return fail(RT_ERR_INVALID, who + ": spp_total above the session's spp_capacity");
    const uint64_t n_pix = (uint64_t)s.rg.row_count * s.rg.col_count;
    SessionWindow w{(char*)s.rec.p, s.cap, done, done, 1u, 1u, spp_total > done, d_rgb8 != nullptr || d_linear != nullptr};
    if (!w.trace && !w.finish) return RT_OK;
    if (w.trace) {
        ProgWindow pw;
        const int prc = progressive_window(n_pix, done, spp_total, split_waves(c, s.f32()), &pw);
        if (prc != kPlanOk) return fail(prc, who + ": no plan for this window (more than 0x7FFFFFFF work items)");
        w.S = pw.S;
        w.nsub = pw.nsub;
        w.s_base = pw.base;
    }
    const FrameArgs a = session_frame(s, spp_total, d_rgb8, d_linear);
    hipStream_t st = (hipStream_t)stream;
    int rc = begin_launch(c, st);   // the session shares the counter, scratch and camera tables
    if (rc != RT_OK) return rc;
    rc = with_precision(s.f32(), [&](auto t) { return launch_window<decltype(t)>(c, a, w, st); });
    if (rc != RT_OK) return rc;
    if ((rc = end_launch(c, st, n_pix, n_pix * (uint64_t)(spp_total - done))) != RT_OK) return rc;
    if (w.trace) s.run.broken = s.run.started;   // a refinement run's lists no longer say what the pixels hold
    s.set_done(spp_total);
    s.touch(st);
    return RT_OK;
}

// One reduction of a call over per-pixel counts: the pixels with counts[p] > 0, each at its count, into the outputs.
struct MapReduce {
    const uint32_t* counts;
    void* rgb;
    void* lin;
};

// The work of the per-pixel-count calls.  Traces [s.done[p], target[p]) of every pixel (target == NULL: nothing),
// then runs the n_red reductions in order; `extra` (n_extra words, may be NULL) is sent to the device behind the
// other tables and *d_extra receives its device address.  The callers have checked the arrays.  Returns with
// *enqueued false when there was nothing to do.
static int run_map(LaunchContext* c, Session& s, const std::string& who, const uint32_t* target, const MapReduce* red,
                   size_t n_red, const uint32_t* extra, size_t n_extra, const uint32_t** d_extra, hipStream_t st,
                   bool* enqueued) {
    const uint32_t n_pix = s.n_pix(), waves = split_waves(c, s.f32());
    *enqueued = false;
    uint32_t S = 0;
    uint64_t n_items = 0, traced = 0;
    if (target) {
        const int prc = progressive_map_plan(n_pix, s.done.data(), target, waves, &S, &n_items, nullptr, 0u);
        if (prc != kPlanOk) return fail(prc, who + ": no plan for this map (more than 0x7FFFFFFF work items)");
        for (uint32_t p = 0; p < n_pix; ++p) traced += target[p] - s.done[p];
    }
    std::vector<std::vector<CountClass>> cls(n_red);
    size_t list_words = 0;
    for (size_t r = 0; r < n_red; ++r) {
        if (!group_by_count(red[r].counts, n_pix, nullptr, cls[r]))
            return fail(RT_ERR_UNSUPPORTED, who + ": more than 256 distinct sample counts in one reduction");
        if (!cls[r].empty()) list_words += n_pix;
    }
    if (n_items == 0 && list_words == 0) return RT_OK;
    // the tables, in one copy: the items' records, the reductions' index lists, the caller's words.  The host
    // fills them before the launch begins, so that the collect's kernel_ms is the device's time alone
    HIPCHK(hipSetDevice(c->device));
    const size_t item_words = (size_t)n_items * kMapItemWords, words = item_words + list_words + n_extra;
    int rc = stage_reserve(s.stage, words * sizeof(uint32_t));
    if (rc != RT_OK) return rc;
    uint32_t* const tab = (uint32_t*)s.stage.p;
    if (n_items && progressive_map_plan(n_pix, s.done.data(), target, waves, &S, &n_items, tab, n_items) != kPlanOk)
        return fail(RT_ERR_INVALID, who + ": internal: the plan's two passes disagree");
    size_t at = item_words;
    std::vector<size_t> list_at(n_red, 0);
    for (size_t r = 0; r < n_red; ++r) {
        if (cls[r].empty()) continue;
        (void)group_by_count(red[r].counts, n_pix, tab + at, cls[r]);
        list_at[r] = at;
        at += n_pix;
    }
    if (n_extra) memcpy(tab + at, extra, n_extra * sizeof(uint32_t));
    if ((rc = begin_launch(c, st)) != RT_OK) return rc;   // the session shares the counter, scratch and camera tables
    if ((rc = send_tables(s, words * sizeof(uint32_t), st)) != RT_OK) return rc;
    const uint32_t* const d_tab = (const uint32_t*)s.tables.p;
    if (d_extra) *d_extra = d_tab + at;
    if (n_items) {
        const uint32_t item_spp = (uint32_t)std::max<uint64_t>(1u, traced / n_items);   // the mean item
        if ((rc = trace_items(c, s, (const MapItem*)d_tab, (uint32_t)n_items, item_spp, st)) != RT_OK) return rc;
    }
    bool set_id = n_items == 0;
    for (size_t r = 0; r < n_red; ++r) {
        if (cls[r].empty()) continue;
        rc = reduce_classes(c, s, cls[r], d_tab + list_at[r], red[r].rgb, red[r].lin, set_id, st);
        if (rc != RT_OK) return rc;
        set_id = false;
    }
    if (target) {
        if (n_items) s.run.broken = s.run.started;   // as in extend_uniform
        s.done.assign(target, target + n_pix);
        s.refresh_bounds();
    }
    s.touch(st);
    *enqueued = true;
    return end_launch(c, st, n_pix, traced);
}

// rt_progressive_snapshot_map_async(ctx, NULL, ...) of a session in an unbroken run: one finish_window_list per
// class the run has built, then one over the candidates of its next step, which all hold n_k samples.
static int snapshot_run(LaunchContext* c, Session& s, void* d_rgb8, void* d_linear, hipStream_t st) {
    const Session::Refine& r = s.run;
    int rc = begin_launch(c, st);
    if (rc != RT_OK) return rc;
    if (!r.cls.empty()) {
        rc = reduce_classes(c, s, r.cls, (const uint32_t*)s.cls_list.p, d_rgb8, d_linear, true, st);
        if (rc != RT_OK) return rc;
    }
    if (r.n_cand) {
        const std::vector<CountClass> last{CountClass{r.n_k, 0u, r.n_cand}};
        rc = reduce_classes(c, s, last, (const uint32_t*)s.act[r.cur].p, d_rgb8, d_linear, r.cls.empty(), st);
        if (rc != RT_OK) return rc;
    }
    s.touch(st);
    return end_launch(c, st, (uint64_t)s.rg.row_count * s.rg.col_count, 0u);
}

// rt_progressive_error_async: the snapshot at half the count, then at the count, and progressive_error over the
// two; a pixel below 2 samples has no half (0: left out) and reads +inf, whatever its buffers hold.
static int estimate_error(LaunchContext* c, Session& s, const std::string& who, void* d_error, hipStream_t st) {
    const uint32_t n_pix = (uint32_t)s.done.size();
    HIPCHK(hipSetDevice(c->device));
    const size_t lin_bytes = (size_t)n_pix * 3u * sizeof(double);
    int rc = ensure_bytes(s.lin_full, lin_bytes, st);
    if (rc != RT_OK) return rc;
    if ((rc = ensure_bytes(s.lin_half, lin_bytes, st)) != RT_OK) return rc;
    std::vector<uint32_t> half(s.done);
    for (uint32_t& n : half) n /= 2u;
    const MapReduce red[2] = {{half.data(), nullptr, s.lin_half.p}, {s.done.data(), nullptr, s.lin_full.p}};
    const uint32_t* d_counts = nullptr;
    bool enqueued = false;
    if ((rc = run_map(c, s, who, nullptr, red, 2u, s.done.data(), n_pix, &d_counts, st, &enqueued)) != RT_OK) return rc;
    if (!enqueued) {   // no pixel holds a sample: every estimate is +inf, and the counts have not gone up
        if ((rc = begin_launch(c, st)) != RT_OK) return rc;
        if ((rc = stage_reserve(s.stage, (size_t)n_pix * sizeof(uint32_t))) != RT_OK) return rc;
        memcpy(s.stage.p, s.done.data(), (size_t)n_pix * sizeof(uint32_t));
        if ((rc = send_tables(s, (size_t)n_pix * sizeof(uint32_t), st)) != RT_OK) return rc;
        d_counts = (const uint32_t*)s.tables.p;
        s.touch(st);
    }
    hipLaunchKernelGGL(progressive_error, dim3((n_pix + 255u) / 256u), dim3(256), 0, st, (const double*)s.lin_full.p,
                       (const double*)s.lin_half.p, d_counts, (double*)d_error, n_pix);
    HIPCHK(hipGetLastError());
    return end_launch(c, st, 0u, 0u);   // kernel_ms covers the estimate's kernel as well
}

// ---- refinement on the device (rt_progressive_refine;DESIGN.md §4 "Planning on the device") ----
// One step as it stands before anything is enqueued: the n_cand candidates (first: every pixel; later the list
// act[cur]) all hold n_k samples, and the pixels that go on are written to act[nxt].
struct RefineStep {
    bool first;
    uint32_t n_pix, n_k, n_cand;
    int nxt;
};

// The arguments of a step against the run: the run's own on every call after the first, a uniform session that
// holds samples on the first.
static int refine_check(const Session& s, const std::string& who, double tolerance, uint32_t spp_max) {
    const Session::Refine& r = s.run;
    if (r.started) {
        if (tolerance != r.tol || spp_max != r.spp_max)
            return fail(RT_ERR_INVALID, who + ": tolerance or spp_max differs from the run's first call");
        if (r.broken)
            return fail(RT_ERR_UNSUPPORTED, who + ": another call has traced into the session since the run's last "
                                                  "step (rt_progressive_extend_map_async takes any map)");
        return RT_OK;
    }
    if (spp_max > s.cap) return fail(RT_ERR_INVALID, who + ": spp_max above the session's spp_capacity");
    if (spp_max < s.done_max) return fail(RT_ERR_INVALID, who + ": spp_max below the samples a pixel already holds");
    if (s.done_min != s.done_max)
        return fail(RT_ERR_UNSUPPORTED, who + ": a run starts on a uniform session (rt_progressive_extend_map_async "
                                              "takes any map)");
    if (s.done_min == 0u) return fail(RT_ERR_INVALID, who + ": the session holds no sample yet");
    return RT_OK;
}

// The run's device arrays, on its first call.
static int refine_alloc(Session& s, uint32_t n_pix) {
    const size_t words = (size_t)n_pix * sizeof(uint32_t), lin_bytes = (size_t)n_pix * 3u * sizeof(double);
    const size_t blocks = ((size_t)n_pix + kRefineBlock - 1u) / kRefineBlock;
    int rc = RT_OK;
    for (DeviceBuffer* b : {&s.counts, &s.act[0], &s.act[1], &s.cls_list})
        if ((rc = reserve(*b, words)) != RT_OK) return rc;
    if ((rc = reserve(s.sel, n_pix)) != RT_OK) return rc;
    if ((rc = reserve(s.blk, blocks * sizeof(uint32_t))) != RT_OK) return rc;
    if ((rc = reserve(s.ret, 4u * sizeof(uint32_t))) != RT_OK) return rc;
    if ((rc = reserve(s.lin_cur, lin_bytes)) != RT_OK) return rc;
    return reserve(s.lin_new, lin_bytes);
}

// The estimate's reductions: the whole frame at n0 / 2 and n0 at first, later the candidates alone at n_k, whose
// values at n_k / 2 (the count they held a step ago) are still in lin_cur.
static int refine_estimate(LaunchContext* c, Session& s, const RefineStep& k, hipStream_t st) {
    if (!k.first) {
        const std::vector<CountClass> cand{CountClass{k.n_k, 0u, k.n_cand}};
        return reduce_classes(c, s, cand, (const uint32_t*)s.act[s.run.cur].p, nullptr, s.lin_new.p, true, st);
    }
    if (k.n_k >= 2u) {
        const int rc = reduce_uniform(c, s, k.n_k / 2u, s.lin_cur.p, st);
        if (rc != RT_OK) return rc;
    }
    return reduce_uniform(c, s, k.n_k, s.lin_new.p, st);
}

// Select, scan, scatter: the next active list into the other act buffer, the rest behind the earlier classes.
// Then the step's one readback, and its one wait: *A, how many pixels go on.
static int refine_partition(Session& s, const RefineStep& k, double tolerance, uint32_t spp_max, hipStream_t st,
                            uint32_t* A) {
    const uint32_t* const list = k.first ? nullptr : (const uint32_t*)s.act[s.run.cur].p;
    const uint32_t n_cand = k.n_cand, n_k = k.n_k, nb = (n_cand + kRefineBlock - 1u) / kRefineBlock;
    uint32_t* const d_blk = (uint32_t*)s.blk.p;
    hipLaunchKernelGGL(refine_select, dim3(nb), dim3(kRefineBlock), 0, st, list, n_cand, n_k, tolerance,
                       n_k < spp_max ? 1u : 0u, (double*)s.lin_cur.p, (const double*)s.lin_new.p, (uint32_t*)s.counts.p,
                       (uint8_t*)s.sel.p, d_blk);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(refine_scan, dim3(1), dim3(kRefineBlock), 0, st, d_blk, nb, (uint32_t*)s.ret.p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(refine_scatter, dim3(nb), dim3(kRefineBlock), 0, st, list, n_cand, (const uint8_t*)s.sel.p,
                       (const uint32_t*)d_blk, (uint32_t*)s.act[k.nxt].p, (uint32_t*)s.cls_list.p + s.run.cls_used);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s.stage.p, s.ret.p, 4u * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *A = *(const volatile uint32_t*)s.stage.p;
    return RT_OK;
}

// The run after the partition: the pixels that stopped are a class at n_k, the A that go on are the candidates of
// the next step.  This step has built no item table yet.
static void refine_commit(Session& s, const RefineStep& k, double tolerance, uint32_t spp_max, uint32_t A, hipStream_t st) {
    Session::Refine& r = s.run;
    if (k.n_cand - A) r.cls.push_back(CountClass{k.n_k, r.cls_used, k.n_cand - A});
    r.cls_used += k.n_cand - A;
    r.started = true;
    r.tol = tolerance;
    r.spp_max = spp_max;
    r.cur = k.nxt;
    r.n_cand = A;
    r.n_k = k.n_k;
    r.S = 0u;
    r.n_items = 0u;
    s.done_stale = true;
    s.touch(st);
}

// The plan (rt_progressive_map_plan's for A pixels that all go from n_k to t: its mean is exact), refine_expand
// into the item table, and the trace.
static int refine_trace(LaunchContext* c, Session& s, const std::string& who, const RefineStep& k, uint32_t A,
                        hipStream_t st, uint64_t* n_active, uint64_t* n_samples) {
    Session::Refine& r = s.run;
    const uint32_t n_k = k.n_k, t = (uint32_t)std::min<uint64_t>(2ull * n_k, r.spp_max);
    uint32_t S = 0;
    uint64_t planned = 0;
    const int prc = split_plan(A, t - n_k, split_waves(c, s.f32()), &S, &planned);
    const bool grid = prc == kPlanOk && S % kSplitGrain == 0u;
    const uint32_t base = grid ? n_k - n_k % kSplitGrain : n_k;
    const uint32_t nsub = grid ? split_nsub(t - base, S) : 1u;
    const uint64_t n_items = (uint64_t)A * nsub;
    if (prc != kPlanOk || n_items > kSplitMaxItems) {
        r.broken = true;   // the active pixels stay at n_k, as the device counts say
        return fail(prc != kPlanOk ? prc : RT_ERR_UNSUPPORTED, who + ": no plan for this step (more than 0x7FFFFFFF work items)");
    }
    int rc = ensure_bytes(s.items, (size_t)n_items * sizeof(MapItem), st);
    if (rc != RT_OK) return rc;
    hipLaunchKernelGGL(refine_expand, dim3((A + kRefineBlock - 1u) / kRefineBlock), dim3(kRefineBlock), 0, st,
                       (const uint32_t*)s.act[r.cur].p, A, (uint32_t*)s.counts.p, n_k, t, base, grid ? S : t - n_k, nsub,
                       (MapItem*)s.items.p);
    HIPCHK(hipGetLastError());
    const uint64_t traced = (uint64_t)A * (t - n_k);
    const uint32_t item_spp = (uint32_t)std::max<uint64_t>(1u, traced / n_items);   // the mean item, as run_map
    if ((rc = trace_items(c, s, (const MapItem*)s.items.p, (uint32_t)n_items, item_spp, st)) != RT_OK) return rc;
    r.n_k = t;
    r.S = S;
    r.n_items = n_items;
    *n_active = A;
    *n_samples = traced;
    return end_launch(c, st, k.n_pix, traced);
}

// One step of rt_progressive_refine: check the arguments against the run; allocate on the first call; run the
// estimate's reductions; select, scan, scatter and read back; commit the run's state; plan, expand and trace.
static int refine_step(LaunchContext* c, Session& s, const std::string& who, double tolerance, uint32_t spp_max,
                       hipStream_t st, uint64_t* n_active, uint64_t* n_samples) {
    Session::Refine& r = s.run;
    int rc = refine_check(s, who, tolerance, spp_max);
    if (rc != RT_OK) return rc;
    const bool first = !r.started;
    const RefineStep k{first, s.n_pix(), first ? s.done_min : r.n_k, first ? s.n_pix() : r.n_cand, first ? 0 : 1 - r.cur};
    if (!first && (k.n_cand == 0u || k.n_k >= spp_max)) {   // converged, or every candidate is at the cap
        r.S = 0u;
        r.n_items = 0u;   // this step built no table
        return RT_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    if (first && (rc = refine_alloc(s, k.n_pix)) != RT_OK) return rc;
    if ((rc = stage_reserve(s.stage, 4u * sizeof(uint32_t))) != RT_OK) return rc;
    if ((rc = begin_launch(c, st)) != RT_OK) return rc;   // the session shares the counter, scratch and camera tables
    if ((rc = refine_estimate(c, s, k, st)) != RT_OK) return rc;
    uint32_t A = 0;
    if ((rc = refine_partition(s, k, tolerance, spp_max, st, &A)) != RT_OK) return rc;
    if (A > k.n_cand) return fail(RT_ERR_HIP, who + ": internal: more active pixels than candidates");
    refine_commit(s, k, tolerance, spp_max, A, st);
    if (A == 0u) return end_launch(c, st, k.n_pix, 0u);
    return refine_trace(c, s, who, k, A, st, n_active, n_samples);
}

}  // namespace rt
