// rt_trace_body.hpp -- the statements of the persistent path-regeneration kernel, included as the body of
// trace_paths and of trace_paths_split (rt_trace.hpp; not a header on its own).  In scope: T, W, ROOT2, MODE,
// CAMQ, MEGA, SPLIT, WIN (SPLIT only: the items tile a sample window, WParams<T>), ITEMS (SPLIT only: the items
// are read from a table, IParams<T>), RAYS (trace_paths_rays, rt_rays.hpp: the primary rays are the caller's,
// RParams<T>).  The kernel arguments (KParams<T>) are read through cold_args<T>().
    constexpr bool SC = MODE == kModeScalar;
    static_assert(!SPLIT || (MODE == kModeV2 && !ROOT2), "the sample-parallel kernels cover the live path only");
    static_assert(!ITEMS || (SPLIT && !WIN), "an item table replaces the window's decode");
    static_assert(!RAYS || (!SPLIT && !CAMQ && MODE == kModeV2), "caller rays: the live path, one item per pixel, no camera batches");
    // fp64 at 5+ waves per SIMD: a 64-entry queue (half the LDS), so the parked ray fits in 32 KB per
    // workgroup
    constexpr bool kF64Park = sizeof(T) == 8 && W >= 5;
    constexpr uint32_t QW = CAMQ ? 4 : 1, QN = CAMQ ? (kF64Park ? 64u : kQCap) : 1;
    __shared__ unsigned long long wcount[4][4];   // segments, lane slots, bounce iterations, direct sky samples
    // 8-byte aligned: finish_pixel keeps its 12 running sums (T, fp64 too) in this array
    __shared__ __attribute__((aligned(16))) uint32_t s_hist[4][64];
    __shared__ __attribute__((aligned(16))) T s_stage[4][3][64];   // finish_pixel: 64 positions' values per wave
    using IS = std::conditional_t<SPLIT, IssueStateS, IssueState>;
    __shared__ IS s_is[4];
    __shared__ unsigned long long s_pool;   // the workgroup's pool of claimed items: next << 32 | end
    __shared__ uint32_t s_dry;              // claim streams this workgroup found exhausted (bit s)
    __shared__ uint32_t q_sid[QW][QN];   // sid | slot << 29 (the pixel: s_slotpix[slot])
    __shared__ uint32_t s_slotpix[4][kSlots];   // the pixel of each open slot
    // ... and its work item (read at finish_pixel, not held in a VGPR); SPLIT: the pixel's index in the
    // rendered set, whose region of the record buffer the slot's samples write
    __shared__ uint32_t s_item[4][kSlots];
    __shared__ int q_hit[QW][QN];
    __shared__ T q_t[QW][QN], q_d[QW][3][QN];
    // camera candidate list of each open pixel slot (pixel_list): [0] = count (0xFFFF: none, sweep per batch)
    __shared__ alignas(16) uint16_t s_clist[QW][CAMQ ? kSlots : 1][kCList];   // 16 B lists: one LDS read (fp64)
    // fp32 at 6 waves per SIMD (80 VGPRs): each lane's ray origin and direction are parked in LDS
    // across the sphere sweeps and the camera batches and re-read right before the scatter, instead
    // of being held in VGPRs (the allocator otherwise spills them to scratch memory around the sweep).
    constexpr bool kPark = (sizeof(T) == 4 && W >= 6) || kF64Park;
    // the mega-level kernels park the path colour as well (their four-level sweep holds more state), and
    // so does fp32 at W6 since issue() finishes sky pixels (it pushed the colour into scratch spills
    // around the scatter; parked: C +0.9 % same-box, LDS 26.8 of 27.3 KB per workgroup)
    constexpr bool kParkC = kPark && (MEGA || (sizeof(T) == 4 && W == 6));
    __shared__ T s_park[kPark ? 4 : 1][kParkC ? 9 : 6][64];
    // finish_pixel's position map (P <= kLMapCap) in LDS: the fp64 live-path kernels without the mega level
    // (fp64 C +1.1 % same-box).  fp32 lost 7 % with it (the extra finish_pixel code pushed 5 more spills
    // into the hot loop at 80 VGPRs); the mega kernels' LDS is full at 6 waves per SIMD.
    constexpr bool kLMap = MODE == kModeV2 && !MEGA && kLMapCap > 0u && sizeof(T) == 8 && !kF64Park;
    __shared__ __attribute__((aligned(16))) uint16_t s_lmap[kLMap ? 4 : 1][kLMap ? kLMapCap : 2];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (lane == 0) { wcount[wave][0] = 0; wcount[wave][1] = 0; wcount[wave][2] = 0; wcount[wave][3] = 0; }
    if (lane < kNWork) g_work[wave][lane] = 0ull;
#ifdef RT_KSTATS
    if (lane < kNKstat) g_kst[wave][lane] = 0;
#endif
    if constexpr (SPLIT) {
        if (lane == 0) s_is[wave] = IssueStateS{};   // cur_next == cur_end: no item open
    } else {
        if (lane == 0) s_is[wave] = IssueState{cold_args<T>()->spp, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    }
    // The workgroup's first block is block blockIdx.x, taken without an atomic (the counter's claims
    // start at gridDim.x): the launch's opening burst of one global atomic per workgroup is gone.
    {
        const auto& q = *cold_args<T>();
        uint32_t b0 = 0, b1 = 0;
        const bool got = guided_block(q.n_items, max(1u, kTMul * gridDim.x), q.blk_g, blockIdx.x, b0, b1);
        if (threadIdx.x == 0) {
            s_pool = got ? ((unsigned long long)b0 << 32) | b1 : 0ull;   // {next, end}; {0, 0}: empty
            s_dry = 0u;
        }
    }
    __syncthreads();
    V3<T> o = mk(T(0), T(0), T(0)), d = o, c = o;
    // the lane's sample and pixel slot in one VGPR, sid | slot << 29 (as in the camera queue: spp <= 2^20,
    // kSlots <= 8); the slot's pixel is read from s_slotpix where the scatter needs it
    uint32_t ss = 0, k = 0;
    // The mega kernels keep ss in LDS, in this lane's word of the finish stage (s_stage, free outside
    // finish_pixel; terminate saves and restores it around the call): at 80 VGPRs the allocator
    // otherwise spills ss to scratch at every queue pop (config E's last hot-loop spill store).
    constexpr bool kParkSS = MEGA;
    uint32_t* const ssp = (uint32_t*)&s_stage[wave][0][0] + lane;
    auto ss_get = [&]() -> uint32_t {
        if constexpr (kParkSS) { asm volatile("" ::: "memory"); return *ssp; }
        else return ss;
    };
    auto ss_set = [&](uint32_t v) {
        if constexpr (kParkSS) *ssp = v;
        else ss = v;
    };
    if constexpr (kParkSS) *ssp = 0u;
    // lane s < kSlots: slot s's samples not yet terminated, | kSlotNZ once one of them terminated at a
    // bounce e > 0 (so finish_pixel knows a sky pixel without reading its records).  In a VGPR, not LDS:
    // the LDS round trip sat on terminate's path every iteration (config E -4.6 %, C +-0 against this)
    constexpr uint32_t kSlotNZ = 0x80000000u;
    uint32_t slot_left = 0;
    auto sid_of = [](uint32_t v) -> uint32_t { return v & 0x1FFFFFFFu; };
    auto slot_of = [](uint32_t v) -> uint32_t { return v >> 29; };
    bool live = false;
    bool scat = false;                 // hit at bounce k last iteration, still below depth: scatter now
    int hit_i = -1;
    T hit_t = T(0);
    auto park = [&](const V3<T>& po, const V3<T>& pd) {
        T* r = &s_park[kPark ? wave : 0][0][lane];
        r[0] = po.x; r[64] = po.y; r[128] = po.z; r[192] = pd.x; r[256] = pd.y; r[320] = pd.z;
    };
    auto unpark = [&](V3<T>& po, V3<T>& pd) {
        asm volatile("" ::: "memory");   // re-read: the registers must not be kept across the sweep
        const T* r = &s_park[kPark ? wave : 0][0][lane];
        po = mk(r[0], r[64], r[128]);
        pd = mk(r[192], r[256], r[320]);
    };
    auto park_c = [&](const V3<T>& pc) {
        T* r = &s_park[kPark ? wave : 0][kParkC ? 6 : 0][lane];
        r[0] = pc.x; r[64] = pc.y; r[128] = pc.z;
    };
    auto unpark_c = [&]() -> V3<T> {
        asm volatile("" ::: "memory");
        const T* r = &s_park[kPark ? wave : 0][kParkC ? 6 : 0][lane];
        return mk(r[0], r[64], r[128]);
    };

    // The samples' records go through trace_records<T, SPLIT>(wave), a slot's to the region
    // trace_region<SPLIT>(s_item[wave], slot) of it (rt_finish.hpp).  kRecY: the primary y is recorded.
    constexpr bool kRecY = SPLIT || MODE == kModeV2;

    // Hand the lanes of `want` new samples in rank order, opening pixel slots as needed; returns
    // true in the lanes that got one.
    // Camera batches on the live path: pixels whose camera candidate list is empty finish at claim time
    // (not SPLIT: its kernels never reduce a pixel; such a pixel is traced, its samples write e = 0)
    constexpr bool kDirectSky = CAMQ && MODE == kModeV2 && !SPLIT;
    // i_mask: the slots the samples were taken from (wave-uniform).
    auto issue = [&](unsigned long long want, uint32_t& i_sid, uint32_t& i_slot, uint32_t& i_pix,
                     uint32_t& i_row, uint32_t& i_col, uint32_t& i_mask) -> bool {
        i_mask = 0u;
        if (want == 0ull) return false;   // nothing asked: the state stays as it is
        const uint32_t spp = cold_args<T>()->spp;
        uint32_t cur_next = __builtin_amdgcn_readfirstlane(s_is[wave].cur_next);
        uint32_t cur_end = spp;   // the open item's last sample + 1
        if constexpr (SPLIT) cur_end = __builtin_amdgcn_readfirstlane(s_is[wave].cur_end);
        uint32_t flags = __builtin_amdgcn_readfirstlane(s_is[wave].flags);
        uint32_t cur_pix = __builtin_amdgcn_readfirstlane(s_is[wave].cur_pix);
        uint32_t cur_row = __builtin_amdgcn_readfirstlane(s_is[wave].cur_row);
        uint32_t cur_col = __builtin_amdgcn_readfirstlane(s_is[wave].cur_col);
        uint32_t cur = (flags >> kISCur) & 7u;
        // The common call: the open item holds every sample asked for (at 512 spp, seven of a pixel's eight
        // batches).  Only cur_next changes.  A drained wave has no open item (cur_next == cur_end).
        const uint32_t nwant = (uint32_t)__popcll(want);
        if (cur_end - cur_next >= nwant) {
            const bool isw = (want >> lane) & 1ull;
            if (isw) { i_sid = cur_next + lanes_below(want); i_slot = cur; i_pix = cur_pix; i_row = cur_row; i_col = cur_col; }
            if (lane == 0) s_is[wave].cur_next = cur_next + nwant;
            i_mask = 1u << cur;
            return isw;
        }
        // The flags stay packed, one SGPR, across the pixel's cone walk and finish_sky_direct below.
        bool got = false;
        uint32_t blk_next = __builtin_amdgcn_readfirstlane(s_is[wave].blk_next);
        uint32_t blk_end = __builtin_amdgcn_readfirstlane(s_is[wave].blk_end);
        while (want != 0ull && (flags & kISDrained) == 0u) {
            if (cur_next == cur_end) {
                const uint32_t avail = ~(flags >> kISBusy) & ((1u << kSlots) - 1u);
                if (avail == 0u) break;   // every slot waits for straggler rays
                const auto& q = *cold_args<T>();
                uint32_t item = blk_next;
                if (blk_next < blk_end) {   // this wave's private rest of a block
                    ++blk_next;
                } else {   // lane 0: the workgroup pool, else the next block from the counter
                    uint32_t it = 0xFFFFFFFFu, nb = 0, ne = 0;
                    if (lane == 0) {
                        unsigned long long pv = __hip_atomic_load(&s_pool, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        for (;;) {
                            if ((uint32_t)(pv >> 32) >= (uint32_t)pv) break;   // empty
                            const unsigned long long old = atomicCAS(&s_pool, pv, pv + (1ull << 32));
                            if (old == pv) { it = (uint32_t)(pv >> 32); break; }
                            pv = old;
                        }
                        uint32_t b0 = 0, b1 = 0;
                        bool claimed = false;
                        for (uint32_t r = 0; it == 0xFFFFFFFFu && r < kStreams && !claimed; ++r) {
                            const uint32_t s = (blockIdx.x + r) % kStreams;
                            if ((__hip_atomic_load(&s_dry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >> s) & 1u) continue;
                            const uint32_t j = gridDim.x + s + kStreams * atomicAdd(q.counter + kCtrStride * s, 1u);
                            claimed = guided_block(q.n_items, max(1u, kTMul * gridDim.x), q.blk_g, j, b0, b1);
                            if (!claimed) atomicOr(&s_dry, 1u << s);   // blocks of a stream only grow in j
                        }
                        if (claimed) {
                            it = b0;
                            if (b1 > b0 + 1u && atomicCAS(&s_pool, pv, ((unsigned long long)(b0 + 1u) << 32) | b1) != pv) {
                                nb = b0 + 1u;   // the pool was refilled meanwhile: keep the rest
                                ne = b1;
                            }
                        }
                    }
                    it = __builtin_amdgcn_readfirstlane(it);
                    if (it == 0xFFFFFFFFu) { flags |= kISDrained; break; }
                    item = it;
                    blk_next = __builtin_amdgcn_readfirstlane(nb);
                    blk_end = __builtin_amdgcn_readfirstlane(ne);
                }
                const uint32_t s = __builtin_ctz(avail);
                uint32_t sbits = (1u << (kISBusy + s)) | (CAMQ ? 1u << (kISNeed + s) : 0u);   // the slot's flags once open
                uint32_t first = 0;
                if constexpr (ITEMS) {   // item -> its 16-byte record {pixel, first, end}: wave-uniform scalar loads
                    const cptr<MapItem> tab = (cptr<MapItem>)__builtin_assume_aligned(cold<IParams<T>>()->items, 16);
                    first = tab[item].first;
                    cur_end = tab[item].end;
                    item = tab[item].pixel;
                } else if constexpr (SPLIT) {   // item -> (pixel, samples [first, cur_end))
                    const auto& sq = *cold<SParams<T>>();
                    const uint32_t px = item / sq.nsub;
                    first = (item - px * sq.nsub) * sq.S;
                    if constexpr (WIN) {   // a session's window [s_begin, spp), items on the grid s_base + j S
                        const auto& wq = *cold<WParams<T>>();
                        first += wq.s_base;
                        cur_end = min(spp, first + sq.S);
                        first = max(first, wq.s_begin);
                    } else {
                        cur_end = min(spp, first + sq.S);
                    }
                    item = px;
                }
                if constexpr (RAYS) {   // the caller's pixel: no camera, no image coordinates
                    const auto& rq = *cold<RParams<T>>();
                    cur_row = 0u;
                    cur_col = 0u;
                    cur_pix = rq.pixel_base + item;
                    // a pixel with an invalid ray is not traced: rays_validate wrote its outputs; its slot stays free
                    const cptr<uint64_t> skip = (cptr<uint64_t>)__builtin_assume_aligned(rq.skip, 8);
                    if ((skip[item >> 6] >> (item & 63u)) & 1ull) continue;
                } else {
                    const uint32_t ri = item / q.col_count, ci = item % q.col_count;
                    cur_row = q.row_begin + ri * q.row_step;
                    cur_col = q.col_begin + ci;
                    cur_pix = cur_row * q.W + cur_col;
                }
                if constexpr (kDirectSky) {
                    if (cold_args<T>()->depth > 1u) {
                        // the pixel's camera candidate list now, not at its slot's first batch: an empty
                        // one means no primary ray of the pixel can hit a sphere, so every sample escapes
                        // at bounce 0 and the pixel is finished here without tracing (finish_sky_direct);
                        // its slot stays free
                        const uint32_t nl = __builtin_amdgcn_readfirstlane(pixel_list<T, MEGA>(cur_col, cur_row, s_clist[wave][s]));
                        if (nl == 0u) {
                            const uint32_t ss_keep = kParkSS ? *ssp : 0u;   // the stage is overwritten
                            finish_sky_direct<T>(item, cur_col, cur_row, cur_pix, s_hist[wave], s_stage[wave]);
                            if constexpr (kParkSS) {
                                __builtin_amdgcn_wave_barrier();
                                *ssp = ss_keep;
                            }
                            // its spp primary segments and one bounce iteration, as traced; no lane held them
                            if (lane == 0) { wcount[wave][0] += spp; wcount[wave][3] += spp; wcount[wave][2] += 1u; }
                            continue;
                        }
                        sbits = (1u << (kISBusy + s)) | ((nl == 0xFFFFu ? 1u : 0u) << (kISNoList + s));   // listed: no need
                    }
                }
                if (lane == 0) { s_slotpix[wave][s] = cur_pix; s_item[wave][s] = item; }
                if (lane == s) slot_left = cur_end - first;
                flags = (flags & ~((1u << (kISNeed + s)) | (1u << (kISNoList + s)) | (7u << kISCur))) | sbits | (s << kISCur);
                cur = s;
                cur_next = first;
            }
            const bool isw = (want >> lane) & 1ull;
            const uint32_t take = min((uint32_t)__popcll(want), cur_end - cur_next);
            const uint32_t r = lanes_below(want);
            const bool mine = isw && r < take;
            if (mine) { got = true; i_sid = cur_next + r; i_slot = cur; i_pix = cur_pix; i_row = cur_row; i_col = cur_col; }
            want &= ~__ballot(mine);
            cur_next += take;
            i_mask |= (take != 0u ? 1u : 0u) << cur;
        }
        if (lane == 0) {
            s_is[wave].cur_next = cur_next; s_is[wave].cur_pix = cur_pix; s_is[wave].cur_row = cur_row;
            s_is[wave].cur_col = cur_col; s_is[wave].flags = flags; s_is[wave].blk_next = blk_next;
            s_is[wave].blk_end = blk_end;
            if constexpr (SPLIT) s_is[wave].cur_end = cur_end;
        }
        return got;
    };

    // Record this step's terminations (e: the bounce of a sky hit, or depth for a ray still
    // enabled) and finish every pixel whose last sample this was.
    auto terminate = [&](bool term, bool skyhit, uint32_t e, uint32_t t_slot, uint32_t t_sid, const V3<T>& tc,
                         const V3<T>& td) {
        if (term) {
            const auto sc = trace_records<T, SPLIT>(wave);
            const uint32_t rg = trace_region<SPLIT>(s_item[wave], t_slot);
            sc.set_e(rg, t_sid, e);
            if (MODE == kModeV2) {
                // A sky hit at bounce 0 is white: no record (its map entry carries kWhite, finish_pixel)
                if (skyhit && e != 0u) sc.store_c(rg, t_sid, tc.x, tc.y, tc.z);
            } else {   // own value: colour x sky of the escaping ray's direction (:365-370 / :283-292), or black
                V3<T> v = mk(T(0.0), T(0.0), T(0.0));
                if (skyhit) { const V3<T> sk = sky(td.y); v = mk(tc.x * sk.x, tc.y * sk.y, tc.z * sk.z); }
                sc.store_c(rg, t_sid, v.x, v.y, v.z);
            }
        }
        unsigned long long tm = __ballot(term);
        const unsigned long long nzl = MODE == kModeV2 && !SPLIT ? __ballot(term && e != 0u) : 0ull;
        bool synced = false;
        while (tm != 0ull) {
            const uint32_t s = __builtin_amdgcn_readlane(t_slot, __builtin_ctzll(tm));
            const unsigned long long m = __ballot(term && t_slot == s);
            tm &= ~m;
            if (lane == s) slot_left = (slot_left - (uint32_t)__popcll(m)) | ((m & nzl) != 0ull ? kSlotNZ : 0u);
            const uint32_t left = __builtin_amdgcn_readlane(slot_left, s);
            // pixel complete: once per spp samples -- marked unlikely, so the register allocator
            // places any spill code here rather than in the sphere sweeps
            if constexpr (SPLIT) {
                if (left == 0u) {   // item complete: free the slot (finish_records reduces the pixel)
                    const uint32_t b = __builtin_amdgcn_readfirstlane(s_is[wave].flags);
                    if (lane == 0) s_is[wave].flags = b & ~(1u << (kISBusy + s));
                }
            } else if (__builtin_expect((left & ~kSlotNZ) == 0u, 0)) {
                const uint32_t ss_keep = kParkSS ? *ssp : 0u;   // finish_pixel overwrites the stage
                if (!synced) { wave_mem_sync(); synced = true; }
                KSTAT(6);
                const uint32_t K = finish_pixel<T, MODE, !MEGA>(
                    wave_scratch<T>(wave), s, __builtin_amdgcn_readfirstlane(s_item[wave][s]), s_hist[wave], s_stage[wave],
                    kLMap ? s_lmap[wave] : nullptr, (left & kSlotNZ) == 0u);
                if constexpr (kParkSS) {
                    __builtin_amdgcn_wave_barrier();
                    *ssp = ss_keep;
                }
                if (lane == 0) wcount[wave][2] += K;
                const uint32_t b = __builtin_amdgcn_readfirstlane(s_is[wave].flags);
                if (lane == 0) s_is[wave].flags = b & ~(1u << (kISBusy + s));
            }
        }
    };

    // CAMQ: one full-wave batch of primary rays.  Returns false when no sample could be issued.
    auto camera_batch = [&]() -> bool {
        uint32_t bsid = 0, bslot = 0, bpix = 0, brow = 0, bcol = 0;
        // smask: the batch's pixel slots (one, or two where a pixel's samples end inside the batch)
        uint32_t smask = 0;
        const bool v = issue(~0ull, bsid, bslot, bpix, brow, bcol, smask);
        const unsigned long long vm = __ballot(v);
        if (vm == 0ull) return false;
        V3<T> bd = mk(T(0), T(0), T(0));
        if (v) {   // Camera::get_ray (ray_tracing.rs:77-89) with origin == centre
            const U4 r = [&] {
                const auto& q0 = *cold_args<T>();
                return rng<T>(bsid, bpix, 0u, 0u, q0.k0, q0.k1);
            }();
            const auto& q = *cold_args_after<T>(r.a ^ r.b);
            const T s1 = div_dim((T)bcol + u01a(r, T(0)), q.W, q.rW);
            const T s2 = div_dim((T)brow + u01b(r, T(0)), q.H, q.rH);
            const V3<T> vu = mk(q.vu[0], q.vu[1], q.vu[2]), vv = mk(q.vv[0], q.vv[1], q.vv[2]);
            const V3<T> pc = add(mk(q.ulc[0], q.ulc[1], q.ulc[2]), add(mul(vu, s1), mul(vv, s2)));
            bd = unit(sub(pc, mk(q.center[0], q.center[1], q.center[2])));
            if (kRecY) trace_records<T, SPLIT>(wave).y(trace_region<SPLIT>(s_item[wave], bslot), bsid) = bd.y;   // primary y (quirk Q2)
        }
        T bt = T(0);
        int bi = -1;
        {
            // each newly opened pixel's candidate list (one cone walk per pixel, not per batch).  The flags are read
            // again here, not handed over by issue(): an SGPR held across the camera ray's arithmetic is spilled.
            uint32_t fl = __builtin_amdgcn_readfirstlane(s_is[wave].flags);
            uint32_t need = (fl >> kISNeed) & smask;
            if (need != 0u) {
                fl &= ~(need << kISNeed);
                const uint32_t iw = cold_args<T>()->W;
                while (need != 0u) {
                    const uint32_t sl = (uint32_t)__builtin_ctz(need);
                    need &= need - 1u;
                    const uint32_t pxi = __builtin_amdgcn_readfirstlane(s_slotpix[wave][sl]);
                    const uint32_t row = pxi / iw;
                    const uint32_t nl = __builtin_amdgcn_readfirstlane(pixel_list<T, MEGA>(pxi - row * iw, row, s_clist[wave][sl]));
                    if (nl == 0xFFFFu) fl |= 1u << (kISNoList + sl);   // (issue() cleared the bit when it opened the slot)
                }
                if (lane == 0) s_is[wave].flags = fl;
            }
            const bool listed = ((fl >> kISNoList) & smask) == 0u;
            if (listed) bi = camera_listed<T, ROOT2, SC>(v, bd, bt, s_clist[wave], smask);
            else bi = camera_sweep<T, ROOT2, SC, MEGA>(v, bd, bt);   // whole wave: lanes are spheres in the cull
        }
        if (lane == 0) { wcount[wave][0] += (uint32_t)__popcll(vm); wcount[wave][1] += 64u; }
        const uint32_t depth = cold_args<T>()->depth;
        const bool skyhit = v && bi < 0;
        const bool term = v && (skyhit || depth == 1u);
        const bool push = v && !term;
        const unsigned long long pm = __ballot(push);
        const uint32_t q = __builtin_amdgcn_readfirstlane(s_is[wave].q);
        const uint32_t qhead = q & 0xFFFFu, qcount = q >> 16;
        if (push) {
            const uint32_t e = (qhead + qcount + lanes_below(pm)) % QN;
            q_sid[wave][e] = bsid | (bslot << 29);
            q_hit[wave][e] = bi;
            q_t[wave][e] = bt;
            q_d[wave][0][e] = bd.x; q_d[wave][1][e] = bd.y; q_d[wave][2][e] = bd.z;
        }
        if (lane == 0) s_is[wave].q = q + ((uint32_t)__popcll(pm) << 16);
        terminate(term, skyhit, skyhit ? 0u : depth, bslot, bsid, mk(T(1.0), T(1.0), T(1.0)), bd);
        return true;
    };

    for (;;) {
        bool fresh = false;
        uint32_t frow = 0, fcol = 0, npix = 0;
        if constexpr (CAMQ) {
            // ---- top up the queue with camera batches, then free lanes pop primary-ray hits ----
            const unsigned long long freem = __ballot(!live);
            const uint32_t nfree = (uint32_t)__popcll(freem);
            uint32_t q = 0;
            for (;;) {
                q = __builtin_amdgcn_readfirstlane(s_is[wave].q);
                if ((q >> 16) >= nfree || (q >> 16) + 64u > QN) break;
                if (!camera_batch()) {   // nothing issued.  Read again: q held across the call would be one more SGPR to spill
                    q = __builtin_amdgcn_readfirstlane(s_is[wave].q);
                    break;
                }
            }
            const uint32_t qhead = q & 0xFFFFu, qcount = q >> 16;
            const uint32_t take = min(nfree, qcount);
            const uint32_t r = lanes_below(freem);
            if (!live && r < take) {
                const uint32_t e = (qhead + r) % QN;
                ss_set(q_sid[wave][e]);
                hit_i = q_hit[wave][e];
                hit_t = q_t[wave][e];
                const auto& q = *cold_args<T>();
                const V3<T> pd = mk(q_d[wave][0][e], q_d[wave][1][e], q_d[wave][2][e]);
                const V3<T> po = mk(q.center[0], q.center[1], q.center[2]);
                if constexpr (kPark) park(po, pd);
                else { d = pd; o = po; }
                if constexpr (kParkC) park_c(mk(T(1.0), T(1.0), T(1.0)));
                else c = mk(T(1.0), T(1.0), T(1.0));
                k = 0;
                live = true;
                scat = true;
            }
            if (lane == 0) s_is[wave].q = ((qhead + take) % QN) | ((qcount - take) << 16);
        } else {
            // ---- hand free lanes the next samples (opening new pixel slots as needed) ----
            uint32_t nsid = 0, nslot = 0, nmask = 0;
            fresh = issue(__ballot(!live), nsid, nslot, npix, frow, fcol, nmask);
            if (fresh) ss_set(nsid | (nslot << 29));
        }
        // ---- next rays: camera rays for fresh lanes, scattered rays for last iteration's hits ----
        if constexpr (kPark) unpark(o, d);
        if constexpr (kParkC) c = unpark_c();
        if (fresh || scat) {
            const uint32_t ssv = ss_get();
            const uint32_t pix = (!CAMQ && fresh) ? npix : s_slotpix[wave][slot_of(ssv)];
            if constexpr (RAYS) {
                if (fresh) {   // the caller's ray p R + s % R, as given: not normalised, colour 1
                    const auto& rq = *cold<RParams<T>>();
                    const size_t ray = (size_t)(pix - rq.pixel_base) * rq.R + sid_of(ssv) % rq.R;
                    const T* dp = rq.directions + 3 * ray;
                    d = mk(dp[0], dp[1], dp[2]);
                    if (rq.origins != nullptr) {
                        const T* op = rq.origins + 3 * ray;
                        o = mk(op[0], op[1], op[2]);
                    } else {
                        o = mk(rq.k.center[0], rq.k.center[1], rq.k.center[2]);
                    }
                    c = mk(T(1.0), T(1.0), T(1.0));
                } else {
                    next_ray<T, SC>(false, fcol, frow, pix, sid_of(ssv), k, hit_i, hit_t, o, d, c);
                }
            } else {
                next_ray<T, SC>(CAMQ ? false : fresh, fcol, frow, pix, sid_of(ssv), k, hit_i, hit_t, o, d, c);
            }
        }
        if constexpr (kPark) park(o, d);
        if constexpr (kParkC) park_c(c);
        if (fresh) {
            k = 0;
            live = true;
            if (kRecY) {   // primary y (quirk Q2)
                const uint32_t ssv = ss_get();
                trace_records<T, SPLIT>(wave).y(trace_region<SPLIT>(s_item[wave], slot_of(ssv)), sid_of(ssv)) = d.y;
            }
        } else if (scat) {
            k += 1u;
        }
        if (__ballot(live) == 0ull) break;   // drained, and every slot finished
        // ---- one sphere sweep for every live ray ----
        const uint32_t depth = cold_args<T>()->depth;
        const bool act = live && k < depth;
        hit_i = -1;
        if (act) hit_i = nearest_hit<T, ROOT2, SC, MEGA>(o, d, hit_t);
        const unsigned long long bact = __ballot(act);
        if (lane == 0 && bact) { wcount[wave][0] += (uint32_t)__popcll(bact); wcount[wave][1] += 64u; }
        // ---- terminations: record e (and the colour of a sky hit) ----
        const bool skyhit = act && hit_i < 0;
        // A hit at the last bounce is not scattered: the ray stays enabled and reads black
        // whatever its colour (ray_tracing.rs:495-497), and the scatter draws nothing observable.
        const bool term = live && (!act || skyhit || k + 1 == depth);
        scat = act && hit_i >= 0 && k + 1 < depth;
        if constexpr (kPark) {
            if (MODE != kModeV2) { V3<T> po, pd; unpark(po, pd); d = pd; }   // the own-value modes read d
        }
        if constexpr (kParkC) c = unpark_c();
        {
            const uint32_t ssv = ss_get();
            terminate(term, skyhit, skyhit ? k : depth, slot_of(ssv), sid_of(ssv), c, d);
        }
        live = live && !term;
    }
    if (lane == 0) {
        const auto& q = *cold_args<T>();
        const uint32_t gw = blockIdx.x * (blockDim.x >> 6) + wave;
        unsigned long long* cc = &q.segs[(gw & (kSegShards - 1)) * kSegStride];
        atomicAdd(cc + 0, wcount[wave][0]);
        atomicAdd(cc + 1, wcount[wave][1]);
        atomicAdd(cc + 2, wcount[wave][2]);
        if (wcount[wave][3]) atomicAdd(cc + kDirectSkySlot, wcount[wave][3]);
        for (uint32_t i = 0; i < kNWork; ++i) atomicAdd(cc + kWorkSlot + i, g_work[wave][i]);
#ifdef RT_KSTATS
        for (int i = 0; i < kNKstat; ++i) atomicAdd(cc + kstat_slot(i), g_kst[wave][i]);
#endif
    }
