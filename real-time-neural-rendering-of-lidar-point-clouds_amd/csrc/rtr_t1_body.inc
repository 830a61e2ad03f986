// rtr_t1_body.inc -- the body of T1 (k_project_bin, k_project_bin_clip and k_project_bin_keep in rtr_kernels.hip, which
// include it with CLIP, `clip`, KEEP and `kmask` defined): one text for the three kernels, compiled in each as if written
// there, so that the kernels without clip planes or a keep mask keep exactly the code they had.
    (void)xp;
    // (!CULL: `bounds` carries the chunks' lane spreads of an unpacked cloud, or null; the packed form has them in its headers;
    // MV: the view table, which holds them)
    const ViewTab *const vt = MV ? reinterpret_cast<const ViewTab *>(bounds) : nullptr;
    const float *const spread = CULL ? nullptr : (MV ? vt->spread : bounds);
    const bool lane_test = (clear_split & 4) == 0;
    const uint4 *const pk_hdr = reinterpret_cast<const uint4 *>(x4);
    const uint32_t *const pk_planes = reinterpret_cast<const uint32_t *>(y4);    // the A streams
    const uint32_t *const pk_planes_b = reinterpret_cast<const uint32_t *>(z4);  // the B streams
    const float fW = (float)W, fH = (float)H;
    const float hiW = f_add(fW, 0.25f), hiH = f_add(fH, 0.25f);
    const int lane = threadIdx.x & 63;
    const uint32_t stx = (uint32_t)(W + 31) >> 5;  // storage tiles per row (tile_geom)
    uint32_t *fill = ts_fill(S);  // (MV: the served view's)
    // (a context holds < 2^32 points: quad and chunk indices are 32-bit, which keeps scalar registers free)
    // Chunk order: a chunk is 256 consecutive points (one quad per lane); round r of the grid stride
    // is the window of NW consecutive chunks r NW .. r NW + NW - 1, chunk r NW + w going to wave w.
    // A spatially ordered cloud makes a window ~a million neighbouring points: either none of them is
    // in the frustum or nearly all are, and then EVERY resident wave waits for its claims at the
    // same time -- nobody issues loads, HBM drains (T1 208 -> 300 us), and the claims queue up on a
    // handful of stream counters.  So the waves are cut into `phases` groups of consecutive
    // workgroups, and group g starts its rounds at g R / phases (wrapping around): at any moment the
    // groups sit in different windows, about one of them claiming while the others stream, and the
    // four workgroups resident on a CU (b, b + 256, ...) belong to four different groups.  Inside a
    // group neighbouring waves still read neighbouring kilobytes (DRAM row locality: dealing runs of
    // 16 chunks to each wave instead cost +50 us), and every wave still samples the whole cloud.
    const uint32_t nchunks = (n4 + 63u) / 64u, NW = gridDim.x * (kBlock / 64), wave = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const uint32_t R = (nchunks + NW - 1u) / NW;
#ifdef RTR_EXPERIMENT  // (how long do the waves run, how are the long chunks dealt: tools/stamps.py)
    const unsigned long long t_wave0 = wall_clock64();
    if (lane == 0 && (wave & 63u) == 0u) atomicMax(ts_dbg(S) + 59, ~t_wave0);
#endif
    // (LOAD BALANCE, measured in round 4 and not kept.  The launch ends with its most loaded wave: the chunks that take
    // the long path -- ~4.5 us each against ~1 us for a chunk that only streams -- come in runs shorter than a round, so
    // the waves hold 5 +- 1.5 of them, up to 9 on C3, and T1 = the stream + 9 x 4.5 us where the average wave has 5;
    // an RTR_EXPERIMENT build's histogram of the waves' durations shows the same +-17 us.  (a) A queue in device memory
    // for the candidates of waves past the previous frame's average + 1..3, served by the waves that have finished --
    // tickets, one waiter per slot, compare-and-swap on leaving so that every chunk is processed exactly once, bit-exact:
    // T1 137-197 us against 123 -- a hand-over costs its wave two dependent round trips, about what the chunk would
    // have cost, and the helpers only exist once their own share is done.  (b) The same inside a workgroup, through LDS,
    // its four waves dealt shares a quarter of a round apart so that their loads are independent: 120.5-122.5 against
    // 123 on C3, 25.8-26.4 against 23.5 on the 1e7-point cloud, whose stream the four fronts slow down.)
    // cblock = 0 (the default): one group, unless the PREVIOUS frame of this tile store had more than a quarter
    // of the cloud inside the frustum (its entry count is still in the header; T1's epilogue rewrites it when
    // every workgroup is past this line).  Then the claims, not the stream, bound the kernel -- ~390 k wave
    // claims on the dozen stream counters of a distant overview -- and 16 groups that sit in different parts
    // of the cloud, i.e. in different tiles, spread them: 1.45 -> 0.87 ms for 1e8 points inside 100 x 40
    // pixels, against +10 us on an ordinary view, which therefore keeps the single dense streaming front.
    // The packed kernel (round 4: the light path reads a quarter of each chunk through an LDS ring and is bound by the
    // instructions it issues, no longer by the stream) takes FIVE groups by default when a wave has at least 16 rounds: the
    // five workgroups of a CU then sit in five stretches of the cloud, so a stretch inside the frustum puts one of a
    // SIMD's five waves on the long path at a time instead of all of them -- 104.1 -> 99.5-100.8 us on C3; equal on the
    // sorted uniform_box and on BASELINE C2's 1e7 points (fewer rounds: one group); the fp32 stream, which IS at HBM's
    // rate, keeps its single front (five groups: 227 us against 201-205).
    const uint32_t auto_groups = ts_hdr(S)[kHdrEntries] > n4 ? 16u : ((PACKED && !CULL && GROUPS && R >= 16u) ? 5u : 1u);
    const uint32_t G = cblock < 1u ? auto_groups : (cblock > gridDim.x ? gridDim.x : cblock);
    const uint32_t phase = (uint32_t)((uint64_t)((blockIdx.x * G) / gridDim.x) * R / G);
    auto chunk_of = [&](uint32_t q) -> uint32_t {  // q-th chunk of this wave, q < R (>= nchunks: none)
        uint32_t r = q + phase;
        r = r >= R ? r - R : r;
        const uint32_t c = r * NW + wave;  // (< nchunks + NW < 2^25: a context holds < 2^32 points)
        return (q < R && c < nchunks) ? c : nchunks;
    };
    // one quad (four points per lane) of the wave; every exit is wave-uniform
    // the matrix rows for the four points of a lane (render.cu:33-40).  Only the r.z row before the first exit: about
    // half of the chunks of an indoor view lie behind the camera, and the r.x / r.y rows are a third of what a chunk
    // that leaves early costs
    struct Rows { float4 X, Y, Z; float rz[4]; };
    // The matrix lives in VECTOR registers: the kernel runs four waves per SIMD (128 vector registers each, 94 used)
    // but is short of scalar ones -- 63 of them spilled into lanes and came back through v_readlane in the hot loop;
    // with the twelve matrix entries out of the way it is 49, and T1 is 3.5 us faster (0.1880 -> 0.1845 ms per frame).
    float mv[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        mv[k] = P.m[k];
        asm volatile("" : "+v"(mv[k]));
    }
    // (the lane test's front slack: in a vector register for the fp32 kernel -- as a scalar it cost 8 more spilled scalar
    // registers there --, a scalar for the packed one, which is short of vector registers: a vector one was spilled to
    // scratch, and its reload's vmcnt(0) drained the ring on every chunk)
    float nzfront = -lt.zfront;
    if constexpr (!PACKED) asm volatile("" : "+v"(nzfront));
    // MV: serve view v (wave-uniform) from here on -- its matrix, lane-test constants and tile store
    auto use_view = [&](uint32_t v) {
        if constexpr (MV) {
            S = vt->S[v];
            fill = ts_fill(S);
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                mv[k] = vt->P[v].m[k];
                asm volatile("" : "+v"(mv[k]));
            }
            lt = vt->lt[v];
            nzfront = -lt.zfront;
            if constexpr (!PACKED) asm volatile("" : "+v"(nzfront));
        } else {
            (void)v;
        }
    };
#define RTR_M(k) mv[k]
    auto project_rows = [&](const float4 &X, const float4 &Y, const float4 &Z, Rows &r) {
        const float xs[4] = {X.x, X.y, X.z, X.w}, ys[4] = {Y.x, Y.y, Y.z, Y.w}, zs[4] = {Z.x, Z.y, Z.z, Z.w};
        r.X = X, r.Y = Y, r.Z = Z;
#pragma unroll
        for (int k = 0; k < 4; ++k) r.rz[k] = f_add(fmaf(RTR_M(10), zs[k], fmaf(RTR_M(9), ys[k], f_mul(RTR_M(8), xs[k]))), RTR_M(11));
    };
    // the lane test on a lane's first point (see above); wave-uniform result: does any lane stay a candidate
    auto lane_maybe = [&](float x0, float y0, float z0, float sp, bool live) -> bool {
        const float rz0 = f_add(fmaf(RTR_M(10), z0, fmaf(RTR_M(9), y0, f_mul(RTR_M(8), x0))), RTR_M(11));
        const float sz = f_mul(sp, lt.lz);
        const bool front = live && (f_add(rz0, sz) > nzfront);
        if (__ballot(front) == 0ull) return false;
        const float rx0 = f_add(fmaf(RTR_M(2), z0, fmaf(RTR_M(1), y0, f_mul(RTR_M(0), x0))), RTR_M(3));
        const float ry0 = f_add(fmaf(RTR_M(6), z0, fmaf(RTR_M(5), y0, f_mul(RTR_M(4), x0))), RTR_M(7));
        const float m = fminf(fminf(fmaf(hiW, rz0, -rx0), fmaf(hiH, rz0, -ry0)), fminf(fmaf(0.75f, rz0, rx0), fmaf(0.75f, rz0, ry0)));
        const bool out = (int)(f_sub(rz0, sz) > lt.zsafe) & (int)(m < -f_mul(sp, lt.lall));  // (no branch)
        return __ballot(front && !out) != 0ull;
    };
    uint32_t n_colour = 0;  // chunks of this wave whose colours were loaded (frame statistics)
    // (KEEP: the keep summary of the chunk do_quad serves, a scalar the paths below load when they take up the chunk, so
    // that its latency is not on the exact path)
    uint32_t kst = kKeepAll;
    (void)kst;
    // (Skipping the per-point conservative test below for chunks that have been through the lane test -- inside a stretch
    // of the cloud that lies in the frustum nearly every point passes it -- was measured: 135-142 us against 122-124.  A
    // chunk near the camera plane stays a candidate of the lane test, whose margin step needs r.z > zsafe, and it is this
    // per-point test that lets such a chunk go before the exact arithmetic.)
    auto do_quad = [&](uint32_t i, bool live, const Rows &r) {
        const float *rz = r.rz;
        // (one max3 + max + compare instead of four compares and their combination; fmaxf skips NaNs, and an
        // all-NaN quad compares false)
        const bool front = live && (fmaxf(fmaxf(rz[0], rz[1]), fmaxf(rz[2], rz[3])) > 0.0f);  // render.cu:63
        if (__ballot(front) == 0ull) return;
        float rx[4], ry[4];
        {
            const float xs[4] = {r.X.x, r.X.y, r.X.z, r.X.w}, ys[4] = {r.Y.x, r.Y.y, r.Y.z, r.Y.w}, zs[4] = {r.Z.x, r.Z.y, r.Z.z, r.Z.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                rx[k] = f_add(fmaf(RTR_M(2), zs[k], fmaf(RTR_M(1), ys[k], f_mul(RTR_M(0), xs[k]))), RTR_M(3));
                ry[k] = f_add(fmaf(RTR_M(6), zs[k], fmaf(RTR_M(5), ys[k], f_mul(RTR_M(4), xs[k]))), RTR_M(7));
            }
        }
        bool maybe[4], any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // branch-free: the four margins as fused multiply-adds (one rounding each, < 1e-3 z against margins of
            // 0.25 z: still conservative), their minimum, one compare.  A NaN margin is skipped by fminf: the
            // point then stays a candidate and the exact arithmetic below decides.
            const float z = rz[k];
            const float m = fminf(fminf(fmaf(hiW, z, -rx[k]), fmaf(hiH, z, -ry[k])), fminf(fmaf(0.75f, z, rx[k]), fmaf(0.75f, z, ry[k])));
            const bool out = (z > 1e-30f) && (m < 0.0f);
            maybe[k] = live && (z > 0.0f) && !out;
            any = any || maybe[k];
        }
        if (__ballot(any) == 0ull || RTR_XP(64)) return;
        if constexpr (CLIP) {  // the user's clip planes, exact (clip_keep), on what the conservative test has left
            const float xs[4] = {r.X.x, r.X.y, r.X.z, r.X.w}, ys[4] = {r.Y.x, r.Y.y, r.Y.z, r.Y.w}, zs[4] = {r.Z.x, r.Z.y, r.Z.z, r.Z.w};
            any = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                maybe[k] = maybe[k] && clip_keep(clip, xs[k], ys[k], zs[k]);
                any = any || maybe[k];
            }
            if (__ballot(any) == 0ull) return;
        }
        if constexpr (KEEP) {  // the keep mask, on what is left: the lane's four bits of a chunk that is partly hidden
            // (the lane test before this point looked at the lane's first point whether it is hidden or not: its bound
            // holds for the other three all the same, so it stays conservative)
            if (kst != kKeepAll) {
                const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)(i >> 6));  // (lane 0 is always live)
                const uint32_t kb = keep_bits(kmask, c, (uint32_t)lane);
                any = false;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    maybe[k] = maybe[k] && ((kb >> k) & 1u);
                    any = any || maybe[k];
                }
                if (__ballot(any) == 0ull) return;
            }
        }
        bool in[4];
        uint32_t st[4], pix[4];
        unsigned long long pm[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            in[k] = false;
            st[k] = 0;
            pix[k] = 0;
            pm[k] = 0ull;
            if (__ballot(maybe[k]) == 0ull) continue;
            float inv = 1.0f / rz[k];                 // correctly rounded (contract option B)
            float fu = rintf(f_mul(rx[k], inv));      // render.cu:65
            float fv = rintf(f_mul(ry[k], inv));      // render.cu:66
            in[k] = maybe[k] && (fu >= 0.0f) && (fu < fW) && (fv >= 0.0f) && (fv < fH);  // render.cu:68
            pm[k] = __ballot(in[k]);
            if (in[k]) {
                const int u = (int)fu, v = (int)fv;
                st[k] = (uint32_t)(v >> 4) * stx + (uint32_t)(u >> 5);
                pix[k] = (uint32_t)(((v & 15) << 5) | (u & 31));
            }
        }
        if ((pm[0] | pm[1] | pm[2] | pm[3]) == 0ull || RTR_XP(8)) return;
        n_colour += 1u;  // (wave-uniform: a scalar register)
        // the lane's four colours in one 16-byte load, in flight together with the claims.  Unconditional
        // (and the claims below write variables that have no other definition): a value that merges with
        // another one at the end of a divergent block is waited for right there, which turned one round
        // trip per quad into five
        const uint4 col = rgba4[i];
        // group by storage tile; group `it` is claimed by lane `it` (every lane is active here: the callers mask
        // points past the end of the cloud with `live` instead of branching around them)
        int grp[4] = {-1, -1, -1, -1};
        uint32_t rank[4] = {0, 0, 0, 0};
        uint32_t covered = 0;
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wuninitialized"
#pragma clang diagnostic ignored "-Wsometimes-uninitialized"
        uint32_t claim[kMaxGroups];  // only the claiming lane's value is ever read (readlane below)
#pragma clang diagnostic pop
        int ng = 0;
#pragma unroll
        for (int it = 0; it < (GROUPS ? kMaxGroups : 0); ++it) {
            const int kk = pm[0] ? 0 : (pm[1] ? 1 : (pm[2] ? 2 : (pm[3] ? 3 : -1)));
            if (kk < 0) continue;  // wave-uniform
            const unsigned long long pk = kk == 0 ? pm[0] : (kk == 1 ? pm[1] : (kk == 2 ? pm[2] : pm[3]));
            const uint32_t sk = kk == 0 ? st[0] : (kk == 1 ? st[1] : (kk == 2 ? st[2] : st[3]));
            const int first = __ffsll((long long)pk) - 1;
            const uint32_t lead = (uint32_t)__builtin_amdgcn_readlane((int)sk, first);
            // ranks are lane-major: the (up to four) entries of a lane are neighbours in the stream, so a
            // lane whose four points share the tile writes them as two 16-byte stores
            uint32_t total = 0, lower = 0;
            bool gk[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // (pm[k] IS "in the frustum and not grouped yet": one compare, the rest on the scalar unit; the mask comes
                // back as the lane's condition without a vector instruction)
                const unsigned long long m = __ballot(st[k] == lead) & pm[k];
                gk[k] = __builtin_amdgcn_inverse_ballot_w64(m);
                lower += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                total += (uint32_t)__popcll(m);
                pm[k] &= ~m;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (gk[k]) {
                    grp[k] = it;
                    rank[k] = lower++;
                }
            if (lane == it) claim[it] = atomicAdd(fill + ((size_t)lead << S.fill_shift), total);
            ng = it + 1;
            covered += total;
            if (it == 3 && covered <= 8u) {            // four tiles, at most two points each: an incoherent cloud (or a
                pm[0] = pm[1] = pm[2] = pm[3] = 0ull;  // sliver of the frustum's edge); more rounds cost more than they
            }                                          // save -- the remaining points claim per lane below
        }
        // whatever is left belongs to a fourth, fifth, ... tile: one claim per point
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (in[k] && grp[k] < 0) {
                rank[k] = atomicAdd(fill + ((size_t)st[k] << S.fill_shift), 1u);
                grp[k] = kMaxGroups;
            }
        // (only the ng groups that exist -- usually two or three of twelve -- cost a readlane and four selects)
        uint32_t bsel[4] = {0u, 0u, 0u, 0u};
        auto select_base = [&](auto self, auto it_tag) -> void {  // nested wave-uniform tests: it < ng, statically indexed
            constexpr int it = decltype(it_tag)::value;
            if constexpr (it < kMaxGroups) {
                if (it < ng) {
                    const uint32_t b_it = (uint32_t)__builtin_amdgcn_readlane((int)claim[it], it);
#pragma unroll
                    for (int k = 0; k < 4; ++k) bsel[k] = grp[k] == it ? b_it : bsel[k];
                    self(self, std::integral_constant<int, it + 1>{});
                }
            }
        };
        if (!RTR_XP(16)) select_base(select_base, std::integral_constant<int, 0>{});  // (xp 16: the claims are issued, never waited for)
        const uint32_t cs[4] = {col.x, col.y, col.z, col.w};
        uint32_t v[4];
        bool dyn = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = bsel[k] + rank[k];
            dyn = dyn || (in[k] && v[k] >= kS0);
        }
        if (RTR_XP(4)) return;
        if (RTR_XP(512)) {  // claims waited for, nothing stored
            if ((v[0] ^ v[1] ^ v[2] ^ v[3]) == 0x7FFFFFFFu) fill[0] = 0u;
            return;
        }
        if (__ballot(dyn) == 0ull) {  // the usual case: every position lies in its tile's static extent
            const bool quad = in[0] && in[1] && in[2] && in[3] && grp[0] < kMaxGroups && grp[0] == grp[1] &&
                              grp[0] == grp[2] && grp[0] == grp[3];  // same group: same tile, ranks r, r+1, r+2, r+3
            if (quad) {
                typedef unsigned long long ull2 __attribute__((ext_vector_type(2)));
                struct __attribute__((packed, aligned(8))) Pair { ull2 v; };
                Pair *dst = reinterpret_cast<Pair *>(S.ext0 + ((size_t)st[0] << kS0Shift) + v[0]);
                ull2 a, b;
                a.x = make_entry(__float_as_uint(rz[0]), pix[0], cs[0]);
                a.y = make_entry(__float_as_uint(rz[1]), pix[1], cs[1]);
                b.x = make_entry(__float_as_uint(rz[2]), pix[2], cs[2]);
                b.y = make_entry(__float_as_uint(rz[3]), pix[3], cs[3]);
                dst[0].v = a;
                dst[1].v = b;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (in[k]) S.ext0[((size_t)st[k] << kS0Shift) + v[k]] = make_entry(__float_as_uint(rz[k]), pix[k], cs[k]);
            }
        } else {
            unsigned long long own[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) own[k] = (in[k] && v[k] >= kS0) ? extent_alloc(S, st[k], v[k]) : 0ull;
            __builtin_amdgcn_wave_barrier();  // every allocation of this wave is published before it polls
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (in[k]) {
                    uint64_t *slot = v[k] < kS0 ? S.ext0 + ((size_t)st[k] << kS0Shift) + v[k] : extent_slot(S, st[k], v[k], own[k]);
                    // (a pointer that comes out of memory is "flat" to the compiler; say that it is global memory: with
                    // a flat store possibly in flight every wait of the kernel becomes a full drain)
                    typedef uint64_t __attribute__((address_space(1))) *gslot_t;
                    if (slot) *(gslot_t)slot = make_entry(__float_as_uint(rz[k]), pix[k], cs[k]);
                }
        }
    };

    if (!CULL && PACKED) {
        // HISTORY of this loop (rounds 2-4, one bit stream per axis, a register pipeline like the fp32 loop's below, one
        // stage deeper: header of chunk q + 2, planes of chunk q + 1 and the arithmetic of chunk q in flight together).
        // (Two chunks of planes in flight per wave -- buffers A / B, loop unrolled by two -- lift the loads alone from 95
        // to 87 us (one chunk per wave and memory round trip is 4096 x 1.3 KB / ~1 us = 5.4 TB/s), but the whole kernel
        // gets 5 us slower: 14 more spilled scalar registers and their v_readlane traffic.  Measured in rounds 2 and 3.
        // Round 4, with the lane test: a PAIR of chunks per iteration, the light path on 8-byte loads and the long path
        // re-reading the chunk in full (one copy of it in a two-trip loop): 140-145 us against 127-133; the long path
        // DEFERRED to the wave's own turn (one wave of a SIMD at a time on it, the others streaming; the noted chunk read
        // again): 125-133 against 121-125.  The kernel's duration is a wave's serial chain of iterations -- ~60 light ones
        // of about a memory round trip each and ~5 long ones of 5-6 us of dependent latency -- and neither form shortens
        // that chain; a re-read lengthens it.  An L2 PREFETCH of the chunk after next (its header held one step longer, one
        // dword per 64 bytes of its blocks requested into a register nobody reads): 161-162 us against 122 -- a second
        // pass of every line through L1 and the texture addresser costs far more than the shorter round trip gains.  The
        // planes staged through an LDS RING by LDS-DMA (global_load_lds_dwordx4, two slots per wave, the planes of chunk
        // q + 2 requested as soon as chunk q has been read out of its slot: two chunks in flight per wave, no register holds
        // data in flight; bit-exact at the first attempt): 121.4-121.6 us against 120.2-120.8, 1e7 points 22.1-22.6 against
        // 22.7-22.9 -- twice the bytes in flight buy nothing: the stream part of the launch already runs at the rate
        // the chip sustains, what is left is the chain of the chunks inside the frustum.)  All of that held while a chunk was
        // 1.3 KB; the form below reads a quarter of it.
        //
        // NOW: the light path reads the chunk's A streams only (every lane's FIRST value: a quarter of the chunk); the B
        // streams are requested when the lane test leaves a candidate lane.  Past its last chunk a wave re-requests the
        // cloud's last chunk and skips the position.
        //
        // THE RING.  With a quarter of the bytes per chunk the loop is no longer near HBM's rate but bound by its own
        // chain -- one chunk in flight per wave, one memory round trip per iteration (T1 112-117 us against 119-122: 60 %
        // fewer bytes bought 6 %).  So the A streams of the next kRing chunks are in flight at once, and in no register:
        // a chunk's A streams are one contiguous piece of at most 768 bytes, which ONE global_load_lds_dwordx4 (16 bytes
        // per lane, 48 lanes) lands in an LDS slot of the wave; the headers travel the same way (two lanes' worth,
        // 32 bytes), kLead chunks further ahead, because a chunk's data request needs the offset its header holds -- so
        // no header lives in scalar registers any more, and no scalar load's latency sits on the LDS reads' counter.
        // Iteration q: request header q + kRing + kLead; header q + kRing has landed (vmcnt(2 kLead): the requests return in
        // order, two per iteration) -> request its data into the slot chunk q - 1 has left; data q has landed (vmcnt(2 kRing))
        // -> read header and data q out of their slots.  The compiler knows nothing of these requests (inline assembly):
        // every wait for them is written here; its own waits for ordinary loads (the long path's B streams, colours,
        // claims) drain them too, which is only conservative.
        // The loop is bound by the instructions it issues -- the scalar unit is shared by a CU's twenty waves -- so the
        // ring sizes are powers of two, the chunk id runs along incrementally, and addresses are scalar base + lane offset.
        constexpr int kRing = RTR_T1_RING, kLead = RTR_T1_LEAD, kRingH = kRing + kLead;  // (kLead: iterations a header is ahead of its data)
        static_assert(((kRing + 1) & kRing) == 0 && ((kRingH + 1) & kRingH) == 0, "ring sizes: powers of two");
        typedef uint32_t __attribute__((address_space(3))) lds_u32;
        constexpr int kSlotDw = 256;  // (a chunk's A streams: <= 768 bytes; 48 lanes request 16 bytes each)
        __shared__ __attribute__((aligned(16))) uint32_t s_ring[kBlock / 64][kRing + 1][kSlotDw];  // data
        __shared__ __attribute__((aligned(16))) uint32_t s_rhdr[kBlock / 64][kRingH + 1][8];       // headers
        const uint32_t ring_lds = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)(lds_u32 *)s_ring[threadIdx.x >> 6]);
        const uint32_t rhdr_lds = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)(lds_u32 *)s_rhdr[threadIdx.x >> 6]);
        const uint32_t lane16 = 16u * (uint32_t)lane;
        // chunk of position q, incrementally: c(q + 1) = c(q) + NW, back to the wave's first chunk when the round wraps
        const uint32_t c_first = (uint32_t)__builtin_amdgcn_readfirstlane((int)(phase * NW + wave)), c_wrap = R * NW + wave;
        auto next_chunk = [&](uint32_t c) -> uint32_t {
            c += NW;
            return c >= c_wrap ? c - R * NW : c;
        };
        auto req_hdr = [&](uint32_t q, uint32_t c) {  // (c: position q's chunk; past the cloud's end: its last chunk, masked later)
            const uint32_t cc = c < nchunks ? c : nchunks - 1u;
            const uint32_t voff = 32u * cc + lane16, lds = rhdr_lds + 32u * (q & (uint32_t)kRingH);
            if (lane < 2) asm volatile("s_mov_b32 m0, %2\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(voff), "s"(pk_hdr), "s"(lds) : "memory", "m0");
        };
        auto req_data = [&](uint32_t q) {  // position q's header has landed
            const lds_u32 *const hs = (const lds_u32 *)(uintptr_t)(rhdr_lds + 32u * (q & (uint32_t)kRingH));
            const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)hs[4]), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)hs[5]);
            const uint8_t *src = reinterpret_cast<const uint8_t *>(pk_planes) + (((((uint64_t)hi) << 32) | (uint64_t)lo) << 3);
            const uint32_t lds = ring_lds + 4u * (uint32_t)kSlotDw * (q & (uint32_t)kRing);
            if (lane < 48) asm volatile("s_mov_b32 m0, %2\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(lane16), "s"(src), "s"(lds) : "memory", "m0");
        };
#ifdef RTR_EXPERIMENT
        uint32_t xp_sink = 0;
#endif
        typedef uint32_t u32x4_l __attribute__((ext_vector_type(4)));
        typedef u32x4_l __attribute__((address_space(3))) lds_u32x4;
        // one chunk out of its slot: the lane test on its A streams, then (a candidate) the long path.  g0 / g1: its header
        // words, c: its chunk (< nchunks)
        // (MV: vmask = the views that kept the chunk's header box)
        auto chunk_body = [&](const lds_u32 *slot, const u32x4_l &g0, const u32x4_l &g1, uint32_t c, uint32_t vmask) {
            // (KEEP: the chunk's summary -- the chunk test of one view has brought it with the chunk word and rejected
            // the hidden chunks before the ring; the ring of chunk_test = 0 brings every chunk: a hidden one goes here)
            if constexpr (KEEP && (MV || !CTEST)) {
                kst = keep_state(kmask, c);
                if (!CTEST && kst == kKeepNone) return;
            }
            const uint32_t ww = (uint32_t)__builtin_amdgcn_readfirstlane((int)g0.w);
            const uint32_t bx = g0.x, by = g0.y, bz = g0.z;  // (vector registers: they are only ever OR-ed into values)
            const uint32_t wx = ww & 63u, wy = (ww >> 6) & 63u, wz = (ww >> 12) & 63u;
            // the lane's two dwords of each A stream (bit b l: dword (b l) >> 5, shift (b l) & 31 -- one product for both)
            ChunkRawA raw;
            uint32_t px, py, pz;
            asm("v_mul_u32_u24 %0, %1, %2" : "=v"(px) : "s"(wx), "v"(lane));
            asm("v_mul_u32_u24 %0, %1, %2" : "=v"(py) : "s"(wy), "v"(lane));
            asm("v_mul_u32_u24 %0, %1, %2" : "=v"(pz) : "s"(wz), "v"(lane));
            {
                const uint32_t ix = px >> 5, iy = 2u * wx + (py >> 5), iz = 2u * (wx + wy) + (pz >> 5);
                raw.a[0].d[0] = slot[ix], raw.a[0].d[1] = slot[ix + 1];
                raw.a[1].d[0] = slot[iy], raw.a[1].d[1] = slot[iy + 1];
                raw.a[2].d[0] = slot[iz], raw.a[2].d[1] = slot[iz + 1];
            }
            Rows r;
            float4 X, Y, Z;
#ifdef RTR_EXPERIMENT
            if (RTR_XP(128)) {  // the stream alone: headers, A streams, loop bookkeeping
                xp_sink ^= raw.a[0].d[0] ^ raw.a[1].d[1] ^ raw.a[2].d[0] ^ raw.a[0].d[1] ^ raw.a[1].d[0] ^ raw.a[2].d[1];
                return;
            }
#endif
            // lane test: one point per lane; (wave-uniform) chunks with a 32-bit axis or without a finite spread skip it
            bool cand = true;
            const uint32_t sp_c = (uint32_t)__builtin_amdgcn_readfirstlane((int)g1.z);
            if (lane_test && !(ww & kPackWideFlag) && sp_c < 0x7F000000u) {
                // (b = 0: the mask is empty, the value is the base.  Lanes past the cloud's end hold copies of its last
                // quad -- k_pack_write -- so the test needs no mask of its own: the long path has one)
                auto value0 = [&](uint32_t d0, uint32_t d1, uint32_t prod, uint32_t b, uint32_t base) -> float {
                    uint32_t x;
                    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(x) : "v"(__builtin_amdgcn_alignbit(d1, d0, prod)), "s"((1u << b) - 1u), "v"(base));
                    return __uint_as_float(x);
                };
                const float x0 = value0(raw.a[0].d[0], raw.a[0].d[1], px, wx, bx);
                const float y0 = value0(raw.a[1].d[0], raw.a[1].d[1], py, wy, by);
                const float z0 = value0(raw.a[2].d[0], raw.a[2].d[1], pz, wz, bz);
                if constexpr (MV) {
                    uint32_t kept = 0u;
                    for (uint32_t m = vmask; m; m &= m - 1u) {
                        const uint32_t v = (uint32_t)__builtin_ctz(m);
                        use_view(v);
                        if (lane_maybe(x0, y0, z0, __uint_as_float(sp_c), true)) kept |= 1u << v;
                    }
                    vmask = kept;
                    cand = kept != 0u;
                } else {
                    cand = lane_maybe(x0, y0, z0, __uint_as_float(sp_c), true);
                }
            }
            if (!cand) return;
            uint32_t i_c = c * 64u + (uint32_t)lane;
            const bool live_c = i_c < n4;
            i_c = live_c ? i_c : n4 - 1u;  // (masked lanes: any valid address for the colour load)
            {
                const uint32_t sbx = (uint32_t)__builtin_amdgcn_readfirstlane((int)bx), sby = (uint32_t)__builtin_amdgcn_readfirstlane((int)by);
                const uint32_t sbz = (uint32_t)__builtin_amdgcn_readfirstlane((int)bz);
                const uint4 hc0 = make_uint4(sbx, sby, sbz, ww);
                const uint4 hc1 = make_uint4((uint32_t)__builtin_amdgcn_readfirstlane((int)g1.x), (uint32_t)__builtin_amdgcn_readfirstlane((int)g1.y), 0u, 0u);
                ChunkRaw raw_b;
#ifdef RTR_EXPERIMENT
                if (RTR_XP(1024)) {  // (what the B streams' round trip costs: the A data in their place, wrong frames)
#pragma unroll
                    for (int a = 0; a < 3; ++a) raw_b.a[a].d[0] = raw.a[a].d[0], raw_b.a[a].d[1] = raw.a[a].d[1], raw_b.a[a].d[2] = raw.a[a].d[0], raw_b.a[a].d[3] = raw.a[a].d[1];
                } else
#endif
                raw_b = load_chunk_b(pk_planes_b, hc0, hc1, lane);
                if constexpr (CTEST) {
                    // (all three B loads are waited for HERE: the decode skips an axis of width 0 -- a wall of the room --,
                    // and a load left pending makes the compiler wait for it where its register is next written, with a
                    // vmcnt(0) right behind the ring's wait on the next survivor: the ring drained)
#pragma unroll
                    for (int a = 0; a < 3; ++a) asm volatile("" : "+v"(raw_b.a[a].d[0]), "+v"(raw_b.a[a].d[1]), "+v"(raw_b.a[a].d[2]), "+v"(raw_b.a[a].d[3]));
                }
                unpack_chunk(raw, raw_b, ww, sbx, sby, sbz, X, Y, Z, lane);
                if constexpr (!MV) project_rows(X, Y, Z, r);
            }
            if constexpr (MV) {  // the decoded chunk, once per view that is left
                for (uint32_t m = vmask; m; m &= m - 1u) {
                    use_view((uint32_t)__builtin_ctz(m));
                    project_rows(X, Y, Z, r);
                    do_quad(i_c, live_c, r);
                }
                return;
            }
#ifdef RTR_EXPERIMENT
            if (RTR_XP(256)) {  // ... + decode + the three matrix rows
                xp_sink ^= __float_as_uint(r.rz[0]) ^ __float_as_uint(r.rz[1]) ^ __float_as_uint(r.rz[2]) ^ __float_as_uint(r.rz[3]);
                return;
            }
#endif
            do_quad(i_c, live_c, r);
        };
        if constexpr (CTEST) {
            // THE CHUNK TEST (round 5).  Nine chunks in ten hold no point inside the frustum, and the lane test above found
            // that out only after the ring had brought the chunk's A streams and the wave had decoded and projected a point
            // per lane: ~135 instructions a chunk, about 60 % of what the launch issued.  Every header already gives a box
            // for its chunk (chunk_box), so the wave tests 64 of its chunks at once, one per lane -- a 32-byte header load
            // and the five half-spaces of CULL -- and only the survivors enter the ring; the next 64 headers are in flight
            // meanwhile.  The lane test and the long path run on the survivors as before (the header boxes are up to twice
            // a chunk's extent: the lane test still rejects the chunks whose loose box reached the frustum).
            // Survivor k of the wave goes into slot k & kRing: its header words from the lane that tested it (an ordinary
            // LDS store; word 7 = its chunk, ~0 past the wave's last survivor) and its A streams by LDS-DMA, kRing
            // survivors ahead.  Every call of req issues exactly ONE request (past the last survivor: a dummy one of
            // the A array's first bytes), so "data k has landed" is vmcnt(kRing) with no drain in the prologue; the
            // header loads (the compiler's) only ever add requests behind it, which makes that count conservative.
            uint4 cur0, cur1;  // lane l: the header of position qb + l of the current batch
            uint32_t ksum = 0u;  // (KEEP) lane l: its chunk's keep summary
            uint32_t qb = 0;
            unsigned long long pmask = 0ull;  // survivors of the current batch not requested yet
            auto load_batch = [&](uint32_t q0, uint4 &h0, uint4 &h1) {
                const uint32_t c = chunk_of(q0 + (uint32_t)lane);
                const uint32_t cc = c < nchunks ? c : nchunks - 1u;
                h0 = pk_hdr[2 * (size_t)cc];
                h1 = pk_hdr[2 * (size_t)cc + 1];
                if constexpr (KEEP) ksum = kmask.sum[cc];
            };
            auto test_batch = [&]() {
                const uint32_t c = chunk_of(qb + (uint32_t)lane);
                bool keep = c < nchunks;
                float lo[3], hi[3];
                uint32_t vm = MV ? (1u << vt->count) - 1u : 0u;  // (MV: the views that keep the chunk; no box: all of them)
                if (MV && keep && chunk_box(cur0.x, cur0.y, cur0.z, cur0.w, lo, hi)) {
                    vm = 0u;
                    for (int v = 0; v < vt->count; ++v) {
                        float m[12];
#pragma unroll
                        for (int k = 0; k < 12; ++k) {
                            m[k] = vt->P[v].m[k];
                            asm volatile("" : "+v"(m[k]));
                        }
                        if (!box_outside(frustum_planes(m, fW, fH), lo, hi)) vm |= 1u << v;
                    }
                    if (CLIP && clip_box_outside(clip, lo, hi)) vm = 0u;  // (the planes are shared by every view)
                    keep = vm != 0u;
                } else if (!MV && keep && chunk_box(cur0.x, cur0.y, cur0.z, cur0.w, lo, hi)) {
                    // (the planes from the matrix in vector registers, once per batch: the barrier keeps the compiler
                    // from holding forty of them through the loop)
                    float m[12];
#pragma unroll
                    for (int k = 0; k < 12; ++k) {
                        m[k] = mv[k];
                        asm volatile("" : "+v"(m[k]));
                    }
                    keep = !box_outside(frustum_planes(m, fW, fH), lo, hi);
                    if (CLIP) keep = keep && !clip_box_outside(clip, lo, hi);
                }
                if constexpr (KEEP) keep = keep && ksum != kKeepNone;  // (a chunk the mask hides entirely: never requested)
                // (KEEP, one view: the chunk's summary travels in the top two bits of its chunk word, chunks < 2^25)
                cur1.w = MV ? (c | vm << 24) : (KEEP ? (c | ksum << 30) : c);
                // (every header word is consumed HERE, where the batch is tested: a word whose load is still pending when
                // the survivor's header is written would make the compiler wait for it there -- with a vmcnt(0), which
                // drains the ring's requests on every survivor)
                asm volatile("" : "+v"(cur0.x), "+v"(cur0.y), "+v"(cur0.z), "+v"(cur0.w), "+v"(cur1.x), "+v"(cur1.y), "+v"(cur1.z));
                pmask = __ballot(keep);
            };
            auto req = [&](uint32_t k) {
                while (pmask == 0ull && qb + 64u < R) {  // (wave-uniform) the next batch
                    qb += 64u;
                    load_batch(qb, cur0, cur1);
                    test_batch();
                }
                const uint32_t hs = rhdr_lds + 32u * (k & (uint32_t)kRing), lds = ring_lds + 4u * (uint32_t)kSlotDw * (k & (uint32_t)kRing);
                if (pmask != 0ull) {
                    const int l = __ffsll((long long)pmask) - 1;
                    pmask &= pmask - 1ull;
                    if (lane == l) {
                        *(lds_u32x4 *)(uintptr_t)hs = u32x4_l{cur0.x, cur0.y, cur0.z, cur0.w};
                        *(lds_u32x4 *)(uintptr_t)(hs + 16u) = u32x4_l{cur1.x, cur1.y, cur1.z, cur1.w};
                    }
                    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)cur1.x, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)cur1.y, l);
                    const uint8_t *src = reinterpret_cast<const uint8_t *>(pk_planes) + (((((uint64_t)hi) << 32) | (uint64_t)lo) << 3);
                    if (lane < 48) asm volatile("s_mov_b32 m0, %2\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(lane16), "s"(src), "s"(lds) : "memory", "m0");
                } else {
                    if (lane == 0) *(lds_u32 *)(uintptr_t)(hs + 28u) = ~0u;
                    if (lane < 48) asm volatile("s_mov_b32 m0, %2\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(lane16), "s"(pk_planes), "s"(lds) : "memory", "m0");
                }
            };
            load_batch(0u, cur0, cur1);
            test_batch();
#pragma unroll
            for (int k = 0; k < kRing; ++k) req((uint32_t)k);
            for (uint32_t k = 0;; ++k) {
                req(k + (uint32_t)kRing);
                asm volatile("s_waitcnt vmcnt(%0)" : : "n"(kRing) : "memory");  // data k: kRing requests behind it
                const lds_u32 *const slot = (const lds_u32 *)(uintptr_t)(ring_lds + 4u * (uint32_t)kSlotDw * (k & (uint32_t)kRing));
                const lds_u32 *const hs = (const lds_u32 *)(uintptr_t)(rhdr_lds + 32u * (k & (uint32_t)kRing));
                const u32x4_l g0 = *reinterpret_cast<const lds_u32x4 *>(hs);
                const u32x4_l g1 = *reinterpret_cast<const lds_u32x4 *>(hs + 4);
                const uint32_t cw = (uint32_t)__builtin_amdgcn_readfirstlane((int)g1.w);
                if constexpr (KEEP && !MV) {
                    if ((cw & 0x3FFFFFFFu) >= nchunks) break;  // (wave-uniform) past the wave's last survivor
                    kst = cw >> 30;
                    chunk_body(slot, g0, g1, cw & 0x3FFFFFFFu, 0u);
                    continue;
                }
                if (MV ? cw == ~0u : cw >= nchunks) break;  // (wave-uniform) past the wave's last survivor
                chunk_body(slot, g0, g1, MV ? (cw & 0xFFFFFFu) : cw, cw >> 24);
            }
        } else {
            // (option chunk_test = 0: every chunk of the wave through the ring, the loop of round 4)
            // (prologue: one drain, ~1.5 us once per launch, so that every wait below may count two requests per iteration)
            uint32_t c_req = c_first;
#pragma unroll
            for (int k = 0; k < kRingH; ++k) {
                req_hdr((uint32_t)k, (uint32_t)k < R ? c_req : nchunks);
                c_req = next_chunk(c_req);
            }
#pragma unroll
            for (int k = 0; k < kRing; ++k) {
                asm volatile("s_waitcnt vmcnt(%0)" : : "n"(kRingH - 1) : "memory");  // header k: kRingH - 1 requests behind it
                req_data((uint32_t)k);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            uint32_t c_use = c_first;
            for (uint32_t q = 0; q < R; ++q) {
                req_hdr(q + (uint32_t)kRingH, q + (uint32_t)kRingH < R ? c_req : nchunks);
                c_req = next_chunk(c_req);
                asm volatile("s_waitcnt vmcnt(%0)" : : "n"(2 * kLead) : "memory");  // header q + kRing (requested kLead iterations ago, or drained)
                req_data(q + (uint32_t)kRing);
                asm volatile("s_waitcnt vmcnt(%0)" : : "n"(2 * kRing) : "memory");  // data q (requested kRing iterations ago, or drained)
                const lds_u32 *const slot = (const lds_u32 *)(uintptr_t)(ring_lds + 4u * (uint32_t)kSlotDw * (q & (uint32_t)kRing));
                const lds_u32 *const hs = (const lds_u32 *)(uintptr_t)(rhdr_lds + 32u * (q & (uint32_t)kRingH));
                const u32x4_l g0 = *reinterpret_cast<const lds_u32x4 *>(hs);
                const u32x4_l g1 = *reinterpret_cast<const lds_u32x4 *>(hs + 4);
                const uint32_t c = c_use;
                c_use = next_chunk(c_use);
                if (c >= nchunks) continue;  // (wave-uniform) past the wave's last chunk
                chunk_body(slot, g0, g1, c, 0u);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the requests past the wave's last chunk: into LDS, before it is left)
#ifdef RTR_EXPERIMENT
        if (xp_sink == 0x12345678u) fill[0] = 0u;  // practically never; keeps the work alive
#endif

    } else if (!CULL) {
        // Software pipeline: the coordinates of the wave's NEXT quad are requested as soon as the current
        // ones have gone through the matrix rows, i.e. before the long part of an in-frustum quad (claims,
        // colour load, stores).  A wave waiting for its claims then still has three kilobyte-loads in
        // flight, which is what keeps HBM busy with only 4 waves per SIMD.  Lanes past the end of the cloud
        // re-read its last quad and are masked (`live`).
        float4 X = make_float4(0.f, 0.f, 0.f, 0.f), Y = X, Z = X;
        uint32_t i = 0, spb = 0x7F800000u, kst_f = kKeepAll;
        bool have = false, live = false;
        auto fetch = [&](uint32_t q) {
            const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)(q < R ? chunk_of(q) : nchunks));
            have = c < nchunks;  // wave-uniform
            if constexpr (KEEP) {  // (a chunk the mask hides entirely: its coordinates are never read)
                kst_f = have ? keep_state(kmask, c) : kKeepAll;
                if (kst_f == kKeepNone) have = false;
            }
            if (have) {
                i = c * 64u + (uint32_t)lane;
                live = i < n4;
                const uint32_t ic = live ? i : n4 - 1u;
                if (spread) spb = __float_as_uint(spread[c]);  // (a scalar load, in flight with the coordinates)
                X = ld_stream(x4 + ic);
                Y = ld_stream(y4 + ic);
                Z = ld_stream(z4 + ic);
            }
        };
        fetch(0);
        if constexpr (MV) {
            for (uint32_t q = 0; q < R; ++q) {
                Rows r;
                const bool have_c = have, live_c = live;
                const uint32_t i_c = i < n4 ? i : n4 - 1u;
                const float4 Xc = X, Yc = Y, Zc = Z;  // (the quad is served to every view; the next one is on its way)
                const uint32_t spc = spb;
                if constexpr (KEEP) kst = kst_f;
                fetch(q + 1);
                if (!have_c) continue;
                for (int v = 0; v < vt->count; ++v) {
                    use_view((uint32_t)v);
                    bool cand = true;
                    if (lane_test && spread && spc < 0x7F000000u) cand = lane_maybe(Xc.x, Yc.x, Zc.x, __uint_as_float(spc), live_c);
                    if (!cand) continue;
                    project_rows(Xc, Yc, Zc, r);
                    do_quad(i_c, live_c, r);
                }
            }
        } else
        for (uint32_t q = 0; q < R; ++q) {
            Rows r;
            const bool have_c = have, live_c = live;
            const uint32_t i_c = i < n4 ? i : n4 - 1u;  // (masked lanes past the end: any valid address for the colour load)
            bool cand = have_c;
            if (have_c && lane_test && spread && spb < 0x7F000000u)
                cand = lane_maybe(X.x, Y.x, Z.x, __uint_as_float(spb), live_c);  // (the lane test: one point per lane)
            if (cand) project_rows(X, Y, Z, r);
            if constexpr (KEEP) kst = kst_f;
            fetch(q + 1);
            if (cand) do_quad(i_c, live_c, r);
        }
    } else {
        // 64 of the wave's chunks are tested at once, one per lane, then only the survivors are
        // streamed: the box test costs 1/64 and its load latency is paid once per 64 chunks.
        const FrustumPlanes fpl = frustum_planes(P.m, fW, fH);
        for (uint32_t g0 = 0; g0 < R; g0 += 64) {
            const uint32_t chunk = chunk_of(g0 + (uint32_t)lane);
            const bool valid = chunk < nchunks;
            if (__ballot(valid) == 0ull) continue;
            bool keep = false;
            if (valid) {
                const float *b = bounds + 6 * (size_t)chunk;
                const float lo[3] = {b[0], b[1], b[2]}, hi[3] = {b[3], b[4], b[5]};
                keep = !box_outside(fpl, lo, hi);  // NaN / inf boxes compare false: never culled
                if (CLIP) keep = keep && !clip_box_outside(clip, lo, hi);
                if constexpr (KEEP) keep = keep && kmask.sum[chunk] != kKeepNone;
            }
            unsigned long long mask = __ballot(keep);
            while (mask) {
                const int l = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const uint32_t i = chunk_of(g0 + (uint32_t)l) * 64u + (uint32_t)lane;
                const bool live = i < n4;  // (lanes past the end of the cloud re-read its last quad, masked)
                if constexpr (KEEP) kst = keep_state(kmask, (uint32_t)__builtin_amdgcn_readfirstlane((int)(i >> 6)));
                const uint32_t ic = live ? i : n4 - 1u;
                float4 X, Y, Z;
                if (PACKED) {
                    const uint32_t cc = (uint32_t)__builtin_amdgcn_readfirstlane((int)(i >> 6));
                    const uint4 h0 = pk_hdr[2 * (size_t)cc], h1 = pk_hdr[2 * (size_t)cc + 1];
                    const ChunkRawA raw_a = load_chunk_a(pk_planes, h0, h1, lane);
                    const ChunkRaw raw = load_chunk_b(pk_planes_b, h0, h1, lane);
                    unpack_chunk(raw_a, raw, h0.w, h0.x, h0.y, h0.z, X, Y, Z, lane);
                } else {
                    X = ld_stream(x4 + ic), Y = ld_stream(y4 + ic), Z = ld_stream(z4 + ic);
                }
                Rows r;
                project_rows(X, Y, Z, r);
                do_quad(ic, live, r);
            }
        }
    }
#ifdef RTR_EXPERIMENT
    if (lane == 0) {
        const unsigned long long t_end = wall_clock64();
        // (same-address atomics serialise, ~90 per us, and hold up the claims behind them: a SAMPLE of the waves reports)
        if ((blockIdx.x & 7u) == 0u) {  // histogram of the waves' own durations, 10 us bins from 40 us
            const unsigned long long us = (t_end - t_wave0) / 100ull;
            const int bin = us < 60ull ? 0 : (us >= 200ull ? 7 : (int)((us - 60ull) / 20ull));
            atomicAdd(ts_dbg(S) + 40 + bin, 1ull);
        }
        if ((wave & 63u) == 0u) {
            atomicMax(ts_dbg(S) + 57, t_end);
            atomicMax(ts_dbg(S) + 61, (unsigned long long)n_colour);
            atomicMax(ts_dbg(S) + 56, ~t_end);
            atomicAdd(ts_dbg(S) + 58, t_end);
            atomicAdd(ts_dbg(S) + 60, 1ull);
            atomicAdd(ts_dbg(S) + 62, (unsigned long long)n_colour);
        }
    }
#endif
    if (MV || (clear_split & 8)) {
        // a LEAN frame (lean_frame_end): no ticket, no epilogue -- the tile kernel's workgroups read the stream counters
        // themselves.  Only the colour-chunk statistic leaves, one fire-and-forget add per wave that has any (not for a
        // batch of views: its chunks are not one frame's).
        if (!MV && lane == 0 && n_colour) atomicAdd(ts_sub_colour(S, wave & (uint32_t)(kSubTickets - 1)), (unsigned long long)n_colour);
        return;
    }
    // every claim of this workgroup has returned (its value was used); the workgroup that takes the
    // last ticket sees every stream length final
    // The ticket is the low word of a 64-bit counter whose high word sums the workgroups' colour-chunk counts
    // (frame statistics: bench.py prices the kernel by the bytes it moves) -- one atomic per workgroup for both.
    __shared__ uint32_t s_last, s_colour_total;
    __shared__ uint32_t s_colour[kBlock / 64];
#ifdef RTR_EXPERIMENT
    const unsigned long long t_done = wall_clock64();
#endif
    if (lane == 0) s_colour[threadIdx.x >> 6] = n_colour;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t mine = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) mine += s_colour[w];
        // two levels (rtr_kernels.h, sub[]): workgroup b arrives at word b % 32; the last arrival there zeroes the word
        // for the next frame and carries the group's colour count to the ticket proper
        const uint32_t ng = gridDim.x < (uint32_t)kSubTickets ? gridDim.x : (uint32_t)kSubTickets, grp = blockIdx.x % ng;
        const uint32_t gsize = (gridDim.x - grp + ng - 1u) / ng;
        unsigned long long *const sub = ts_sub(S, grp);
        const unsigned long long old = atomicAdd(sub, 1ull | ((unsigned long long)mine << 32));
        uint32_t last = 0u;
        if ((uint32_t)old == gsize - 1u) {
            __hip_atomic_store(sub, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long group_colour = (old >> 32) + mine;
            const unsigned long long old2 = atomicAdd(reinterpret_cast<unsigned long long *>(ts_ticket(S)), 1ull | (group_colour << 32));
            last = (uint32_t)old2 == ng - 1u ? 1u : 0u;
            s_colour_total = (uint32_t)(old2 >> 32) + (uint32_t)group_colour;
        }
        s_last = last;
    }
    __syncthreads();
#ifdef RTR_EXPERIMENT
    if (s_last && threadIdx.x == 0) ts_dbg(S)[0] = t_done;
#endif
    if (s_last && !RTR_XP(32)) bin_epilogue(S, W, H, clear_split, s_colour_total);
    if (s_last && RTR_XP(32) && threadIdx.x == 0) *reinterpret_cast<unsigned long long *>(ts_ticket(S)) = 0ull;  // (only together with xp 8: nothing was claimed)
