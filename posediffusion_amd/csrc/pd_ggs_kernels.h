// pd_ggs_kernels.h -- the wave-per-item GGS kernels: pd_ggs_kernel (one exchange hop per iteration; every workgroup of a sequence runs the whole
// backward), pd_ggs2_kernel (two hops, the backward distributed: many frames) and pd_ggs_zero_kernel (clears the exchange granules before a launch).
// The lane-per-item kernel is pd_ggs_lane.inc.  Statement fragments shared by the kernels: pd_ggs_pairbwd.inc, pd_ggs_p3b.inc, pd_ggs_p4.inc, pd_ggs_p4_long.inc, pd_ggs_long_hop2.inc, pd_ggs_p4q.inc.
// Textually part of pd_ggs.hip, which holds the development switches read here (PD_GGS_PROF12, PD_GGS_ABLATE, PD_GGS_MIN_WAVES_PER_SIMD, PD_GGS_PROF2).
#pragma once
#include "pd_ggs_sampson.h"

// --------------------------------------------------------------------------------------------
// the kernel
// --------------------------------------------------------------------------------------------
// STAGE_P > 0: waves that own several items stream them through a per-wave double buffer in LDS filled by LDS-DMA
// (STAGE_P pieces of 1 KiB = up to 64 STAGE_P matches per item), the next item in flight while the current one is computed,
// the first item of the next iteration in flight across the serial phases.  STAGE_P = 0: through registers (any item size).
// RESIDENT: every wave owns at most one item (n_slots == 8, the k = ceil(items / 8) regime): its matches stay in registers for
// the whole launch -- a compile-time variant, so the other variants do not carry those 32 registers.
// NW: waves per workgroup.  8 (two per SIMD, up to 256 VGPRs) everywhere; 12 (three per SIMD, 168 VGPRs: the compiler spills launch
// constants of the serial phases, the match pass itself stays in registers) for the staged k = 1 shape, where the match pass is bound
// by VALU cycles two waves per SIMD leave unused.  Slots, chunks of pairs and the P3 thread roles keep their 8-wave / 512-thread
// geometry (the extra waves only take part in the match pass and the strided loops), so every sum is the one the 8-wave kernel forms;
// with 12 waves a wave has ONE staging buffer: the item is read out of LDS whole, after which the buffer takes the next item.
template <int STAGE_P, bool RESIDENT, int NW = PD_GGS_WAVES>
__global__ __launch_bounds__(NW * 64, NW > PD_GGS_WAVES ? 3 : PD_GGS_MIN_WAVES_PER_SIMD) void pd_ggs_kernel(PdGgsParams P, int B, int n_slots, int pinc_rows, int items_cap) {
    constexpr int NT = NW * 64;                       // threads of this instantiation
    constexpr bool SINGLE = NW > PD_GGS_WAVES;        // one staging buffer per wave
    static_assert(!(RESIDENT && SINGLE) && (NW == PD_GGS_WAVES || STAGE_P > 0), "12 waves: the staged variants only");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = tid >> 6;       // (kept a vector value: readfirstlane would move what derives from it to SGPRs, of which the kernel has
                                     //  none to spare -- measured 0.1 us per iteration slower at several workgroups per sequence, equal at one)
    const int b = blockIdx.x % B, wg = blockIdx.x / B;   // XCD-aware: see header comment (B: the launch's sequences, padded to 8 if P.xchg_local)
    if (b >= P.n_seqs) return;                           // (padding blocks of the XCD-local placement)
    const PdSeqDesc D = P.seqs[b];
    const int N = D.n_frames, k = P.k;   // this sequence's own frame count (pd_ggs_plan checked it: P.N, or its entry of pd_engine_set_frame_counts); rows of x stay P.N apart
    const int nW = k * PD_GGS_WAVES;
    const int n_items = D.n_items;
    const Lds L = carve(smem, n_slots, pinc_rows, items_cap);
    const bool p3t = tid < PD_GGS_THREADS;            // takes part in the 512-thread roles of P3
    float *xg = P.x + (size_t)b * P.N * PD_POSE_DIM;
    u64 *xchg = P.xchg ? P.xchg + (size_t)b * 2 * P.xchg_stride : nullptr;

    // wave 0, lane n owns frame n: parameters + momentum live in LDS (L.xst / L.mst) and visit registers only inside P4
    const bool own = (wave == 0 && lane < N);
    if (wave == 0) {
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            L.xst[lane * PD_XS_STRIDE + c] = own ? xg[lane * 9 + c] : 0.0f;
            L.mst[lane * PD_XS_STRIDE + c] = 0.0f;
        }
    }
    // local item table -> LDS (slot = wave + 8 * round <-> item = wg*8 + wave + round * nW)
    for (int s = tid; s < n_slots; s += NT) {
        const int item = wg * PD_GGS_WAVES + (s & 7) + (s >> 3) * nW;
        int4 e = make_int4(0, 0, 0, 0);
        if (item < n_items) {
            const int4 it = D.items[item];
            const int2 ij = D.pair_ij[it.x];
            e = make_int4(it.y, it.z, ij.x, ij.y);
        }
        L.itab[s] = e;
    }
    for (int q = tid; q < D.n_pchunks * (N + 1); q += NT) L.incoff[(q / (N + 1)) * 68 + q % (N + 1)] = D.pchunk_off[q];
    if (tid == 0) {
        L.ctl[0] = 0.0f;
        L.ctl[1] = 0.0f;
        L.ctl[3] = 0.0f;
    }
    if (wave == 0) {
        float xr0[9];
        params_load(L.xst, lane, xr0);
        decode_all(L, xr0, lane, N, D);
    }
    __syncthreads();
    // k > 1, XCD-local placement (P.xchg_local: the launch maps block -> (sequence, workgroup) so that the dispatcher's round-robin puts
    // all workgroups of a sequence on one XCD): the per-iteration exchange can then stay in that XCD's L2 -- plain stores instead of
    // write-through agent-scope ones, 1.1 us instead of 1.9 us per exchange of 24 workgroups (tools/xchg_probe.hip).  The placement is
    // the dispatcher's habit, not a guarantee, so it is VERIFIED once per launch: every workgroup publishes its XCC_ID the safe way
    // (agent scope) and all of them read all of them; only if they agree do the stores stay local.  Same answer in every workgroup.
    bool xl = false;
    if (k > 1 && P.xchg_local) {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        xcc &= 15u;
        u64 *ids = xchg + (size_t)P.xchg_stride - 256;          // the last 256 granules of the sequence's first slot (pd_ggs_plan keeps them free)
        if (tid == 0) __hip_atomic_store(ids + wg, (0x7fffffffull << 32) | (u64)(xcc + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bool same = true, fail = false;
        if (tid < k) {
            unsigned spins = 0;
            u64 v;
            for (;;) {
                v = __hip_atomic_load(ids + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if ((v >> 32) == 0x7fffffffull) break;
                if (++spins > (1u << 20)) {
                    fail = true;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            same = !fail && (unsigned)(v & 0xffffffffull) == xcc + 1;
        }
        if (fail) atomicOr(P.err_flag, 1u);
        if (!same) L.ctl[3] = 1.0f;                              // (zeroed before the barrier above; no static LDS: the dynamic region is the whole 160 KiB)
        __syncthreads();
        xl = L.ctl[3] == 0.0f;
    }
    // matches of this wave's first item stay in registers for the whole launch when every wave owns
    // at most one item (the k = ceil(items/8) regime): no per-iteration match traffic at all
    constexpr bool resident = RESIDENT;
    float4 mres[RESIDENT ? 8 : 1];
    if (RESIDENT) {
        const int4 e = L.itab[wave];
        const int last = e.y > 0 ? e.y - 1 : 0;
        const float4 *pts = D.pts + e.x;
#pragma unroll
        for (int st = 0; st < (RESIDENT ? 8 : 1); ++st) {
            const int m = lane + 64 * st;
            mres[st] = (e.y > 0) ? pts[m < e.y ? m : last] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }

    // LDS staging of the match pass (STAGE_P > 0, several items per wave): this wave's items, its double buffer, and the
    // first item already on its way
    // Items of this workgroup are slots 0 .. n_local-1 (slot q <-> item wg*8 + (q & 7) + (q >> 3) * nW, increasing in q).
    // A wave starts every iteration with its own slot `wave` and then PULLS further slots from a workgroup-wide counter:
    // the two waves that share a SIMD do not issue at the same rate (the older one gets the VALU first), and a static
    // round-robin leaves the faster half idle for the last quarter of the match pass.  Which wave computes an item does
    // not enter its sums, so results stay bitwise reproducible.
    int n_local = 0;
    if (n_items > wg * PD_GGS_WAVES) {
        const int d = n_items - wg * PD_GGS_WAVES, r0 = d / nW;
        n_local = r0 * PD_GGS_WAVES + min(d - r0 * nW, PD_GGS_WAVES);
    }
    int *q_ctr = (int *)&L.ctl[4];
#ifdef PD_GGS_PROF2
    if (P.prof_wave & 0x100) {                   // experiment: only one wave per SIMD works in the match pass
        if (wave >= 4) n_local = 0;
    }
#endif
    const bool staged = STAGE_P > 0 && !resident && wave < n_local;
    const unsigned stage_lds = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(L.stage + wave * ((SINGLE ? 1 : 2) * STAGE_P * 256)));
    const float4 *stage_ptr = (const float4 *)(L.stage + wave * ((SINGLE ? 1 : 2) * STAGE_P * 256));
    int pb = 0;                                   // buffer that holds (or is receiving) the item computed next
    // byte offsets of this lane's match in each piece (lane + 64 q), clamped per item to its last match
    // (the byte offsets lane * 16 + 1024 q are formed where they are used: six registers held across the whole launch are six spills in the
    // 168-register variants, whose reloads from scratch land in the serial phases)
    auto stage_item = [&](int slot, int buf) {
        int4 e = L.itab[slot];
        const int first = __builtin_amdgcn_readfirstlane(e.x);
        const unsigned last16 = (unsigned)(__builtin_amdgcn_readfirstlane(e.y) - 1) * 16u;
        if constexpr (STAGE_P > 0) {
            unsigned off[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) off[q] = min((unsigned)lane * 16u + 1024u * q, last16);     // no predicated loads: a clamped copy of the last match
            pd_glds_item<STAGE_P>(D.pts + first, off, stage_lds + (unsigned)(buf * STAGE_P) * 1024u);
        }
    };
    if (staged) stage_item(wave, 0);

    // ---- geometry of the serial phases ------------------------------------------------------------------------------------------
    // FAST (<= PD_GGS_FAST_FRAMES frames, one chunk of pairs -- every BASELINE config of this kernel): the rows of the pair backward are
    // laid out per frame at a FIXED stride `cap` (the largest number of pairs incident to a frame, rounded up to 4; unused rows stay
    // zero for the whole launch), thread (fb_n, fb_c) = (frame, component) of the first 16 N threads sums its column without index
    // clamps or selects, turns the nine dL/dR sums into dL/dq inside its 16-lane row (row_bcast + the Jacobian of jac_all) and hands P4
    // seven numbers per frame; waves 6 and 7 form the dL/dA and loss totals beside them.
    // GENERAL (more frames or several chunks of pairs): CSR rows, partial sums carried across chunks in LDS, as before.
    const int fb_n = tid >> 4, fb_c = tid & 15;
    const float fb_sign = (fb_c < 9) ? (fb_c < 6 ? -1.0f : 1.0f) : ((fb_c < 11) ? -1.0f : 1.0f);   // D = diag(-1,-1,1): rows a < 2 of dL/dRc, entries < 2 of dL/dtc
    int cap = 0;
    if (D.n_pchunks == 1 && N <= PD_GGS_FAST_FRAMES) {
        int dmax = 0;
        for (int n = 0; n < N; ++n) dmax = max(dmax, L.incoff[n + 1] - L.incoff[n]);
        cap = (dmax + 3) & ~3;
    }
    // a frame's rows start `rstride` = cap + 1 rows apart: with cap % 4 == 0 the four frames a wave sums then sit 16 banks apart -- 64 lanes
    // on 64 distinct LDS banks (at a stride of cap rows all four would share 16 banks: every column load a four-way conflict)
    const int rstride = cap + 1;
    const bool fast34 = cap > 0 && N * rstride <= pinc_rows;    // (block-uniform)
    const int n_row_waves = (N * 16 + 63) >> 6;                 // waves that hold (frame, component) threads in the fast path (<= 6)
    const int ga_parts = fast34 ? n_row_waves : 1;              // dL/dA partials P4 adds up (fast: one per row wave; general: the totals)
    constexpr int W_LOSS = PD_GGS_WAVES - 1;                    // idle in the fast backward phase: forms the loss totals meanwhile
    // pair-level backward in chunks of PD_GGS_THREADS pairs (one chunk up to N = 32); chunk 0's table entry is hoisted
    // (held for the whole launch in THREE registers: frames i | j << 8 and the item count share one -- pd_ggs_set_matches bounds both to 16 bits)
    int4 my_pair = (p3t && tid < D.n_pairs) ? D.ptab[tid] : make_int4(0, 0, 0, 0);
    if (fast34) {
        if (p3t && tid < D.n_pairs) {       // CSR positions -> fixed-stride rows
            const int pi = my_pair.x & 0xff, pj = my_pair.x >> 8;
            const int r0 = pi * rstride + ((my_pair.w & 0xffff) - L.incoff[pi]), r1 = pj * rstride + ((my_pair.w >> 16) - L.incoff[pj]);
            my_pair.w = r0 | (r1 << 16);
        }
        for (int q = tid; q < N * rstride * 4; q += NT) ((float4 *)L.pinc)[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    const int my_pair_xz = (my_pair.x & 0xffff) | (my_pair.z << 16), my_pair_y = my_pair.y, my_pair_w = my_pair.w;
    unsigned epoch = 0;
    int trace_row = 0;
    // the in-kernel cycle counters cost 24 VGPRs for the whole launch: compiled out of the 12-wave variants, which run at the
    // 168-register limit (build with -DPD_GGS_PROF12 to study those; pd_ggs_plan keeps 8 waves while profiling is on otherwise)
    constexpr bool HAS_PROF = !SINGLE || PD_GGS_PROF12;
    const bool prof = HAS_PROF && P.prof != nullptr && blockIdx.x == 0 && wave == (P.prof_wave & 7);   // one wave of WG 0
    // (build with -DPD_GGS_PROF2 for the timers INSIDE the match pass: claim / DMA issue / wait / pass / reduce -> counters 10..14)
    long long pc = 0, pq = 0;
    if (prof && lane == 0) {
        for (int i = 0; i < 16; ++i) L.prof[i] = 0;
    }
#define PD_PROF(i) do { if (prof) { const long long _n = __builtin_readcyclecounter(); if (lane == 0) L.prof[i] += _n - pc; pc = _n; } } while (0)
    const float inv_M = 1.0f / (float)D.M;
    for (int st = 0; st < P.n_stages; ++st) {
        const PdGgsStage S = P.stages[st];
        int stepped = 0;
        // {printed statistic, valid count, loss} of the stage's last iteration: LDS (L.ctl[5..7], written by P4's lane 0), not three registers
        if (tid == 0) {
            L.ctl[5] = __int_as_float(0x7fc00000);
            L.ctl[6] = 0.0f;
            L.ctl[7] = __int_as_float(0x7fc00000);
        }
        for (int it = 0; it < S.iters; ++it) {
            if (prof) pc = __builtin_readcyclecounter();
            // ---- P1: F for the pairs of this workgroup's items -------------------------------
            const Cam cam = {L.cam[0], L.cam[1], L.cam[2], L.cam[3]};
            if (tid == 0) *q_ctr = NW;                    // first slot the match pass hands out dynamically
            for (int s = tid; s < n_slots && !(PD_GGS_ABLATE & 1); s += NT) {
                const int4 e = L.itab[s];
                if (e.y > 0) {
                    float Ri[9], Rj[9], ti[3], tj[3];
                    frame_load(L, e.z, Ri, ti);
                    frame_load(L, e.w, Rj, tj);
                    PairFwd f;
                    pair_forward(Ri, ti, Rj, tj, f);
                    float F[9];
                    fundamental_from_E(f.E, cam, F);
#pragma unroll
                    for (int c = 0; c < 9; ++c) L.F[s * PD_F_STRIDE + c] = F[c];
                }
            }
            __syncthreads();
            PD_PROF(0);

            // ---- P2: per-match Sampson residual + dL/dF, one (pair, chunk) item per wave ------
            ++epoch;
            // slot claims run one item ahead: the LDS atomic for the item after the next one is issued before the pass and
            // consumed after it, so its latency is never exposed (a wave over-claims one slot per iteration: harmless)
            int s_next = n_local;
            if constexpr (!RESIDENT) {
                int t0 = 0;
                if (lane == 0 && wave < n_local) t0 = atomicAdd(q_ctr, 1);
                s_next = __builtin_amdgcn_readfirstlane(t0);
            }
            for (int s = wave; s < n_local && !(PD_GGS_ABLATE & 16);) {
                const int item = wg * PD_GGS_WAVES + (s & 7) + (s >> 3) * nW;
#ifdef PD_GGS_PROF2
#define PD_PROF2(i) do { if (prof) { const long long _n = __builtin_readcyclecounter(); if (lane == 0) L.prof[i] += _n - pq; pq = _n; } } while (0)
                if (prof) pq = __builtin_readcyclecounter();
#else
#define PD_PROF2(i) do { } while (0)
#endif
                int t_claim = 0;
                if constexpr (!RESIDENT) {
                    if (lane == 0) t_claim = atomicAdd(q_ctr, 1);
                }
                PD_PROF2(10);
                int4 e = L.itab[s];
                e.x = __builtin_amdgcn_readfirstlane(e.x);      // wave-uniform by construction: lets the step-count branches be scalar
                e.y = __builtin_amdgcn_readfirstlane(e.y);
                float Fm[9];
                {   // three LDS reads (slot stride 12 floats, 16-byte aligned) instead of nine 4-byte ones
                    const float4 f0 = *(const float4 *)(L.F + s * PD_F_STRIDE), f1 = *(const float4 *)(L.F + s * PD_F_STRIDE + 4);
                    Fm[0] = f0.x; Fm[1] = f0.y; Fm[2] = f0.z; Fm[3] = f0.w;
                    Fm[4] = f1.x; Fm[5] = f1.y; Fm[6] = f1.z; Fm[7] = f1.w;
                    Fm[8] = L.F[s * PD_F_STRIDE + 8];
                }
                // two 64-match steps per pass: lane handles matches lane + 64*(2j) and lane + 64*(2j+1) together
                v2f acc2[PD_ITEM_VALS];
                int nv;
                if constexpr (RESIDENT) {   // straight from the resident registers (no copies)
                    item_pass<false>(MatchRegs{mres}, e.y, lane, Fm, P.sampson_max, acc2, nv);
                } else if constexpr (STAGE_P > 0) {
                    // the slot this wave computes next (or its own first one, for the next iteration: the matches never
                    // change) goes into the other buffer while this one is computed; STAGE_P pieces stay in flight
                    if constexpr (!SINGLE) stage_item(s_next < n_local ? s_next : wave, pb ^ 1);
                    PD_PROF2(11);
                    pd_vmcnt<SINGLE ? 0 : STAGE_P>();
                    PD_PROF2(12);
                    // the whole item out of LDS at once (one exposed LDS latency instead of one per step)
                    float4 mb[8];
                    {
                        const float4 *Bp = stage_ptr + (SINGLE ? 0 : pb) * (STAGE_P * 64) + lane;
#pragma unroll
                        for (int q = 0; q < 8; ++q) mb[q] = q < STAGE_P ? Bp[64 * q] : make_float4(0.f, 0.f, 0.f, 0.f);
                    }
                    if constexpr (SINGLE) {     // the item is in registers: its buffer takes the next one while this one is computed
                        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(mb[0].x), "+v"(mb[1].x), "+v"(mb[2].x), "+v"(mb[3].x), "+v"(mb[4].x), "+v"(mb[5].x) :: "memory");
                        stage_item(s_next < n_local ? s_next : wave, 0);
                    }
                    item_pass<true>(MatchRegs{mb}, e.y, lane, Fm, P.sampson_max, acc2, nv);
                    pb ^= 1;
                } else {
                    // stream this item: all (<= 8) lines in flight at once, indices clamped (no
                    // predicated loads), out-of-range lanes are masked in the arithmetic instead
                    float4 mb[8];
                    const float4 *pts = D.pts + e.x;
                    const int last = e.y - 1;
#pragma unroll
                    for (int st = 0; st < 8; ++st) {
                        const int m = lane + 64 * st;
                        mb[st] = pts[m < e.y ? m : last];
                    }
                    item_pass<false>(MatchRegs{mb}, e.y, lane, Fm, P.sampson_max, acc2, nv);
                }
#ifdef PD_GGS_PROF2
                if (prof) { acc2[0].x += 0.0f * (float)__builtin_amdgcn_readfirstlane(__float_as_int(acc2[9].y)); }   // (keeps the pass before the timer)
#endif
                PD_PROF2(13);
                int slot;
                const float tot = item_totals(acc2, nv, e.y, P.sampson_max, lane, slot);   // this lane holds the item total of `slot`
                if (lane < 16 && slot < PD_ITEM_VALS) {
                    if (k == 1) {
                        L.item[item * PD_ITEM_VALS + slot] = tot;
                    } else {
                        u64 *g = xchg + (size_t)(epoch & 1) * P.xchg_stride + (size_t)item * PD_XCHG_LINE + slot;
                        const u64 gv = ((u64)epoch << 32) | (u64)__float_as_uint(tot);
                        if (xl) asm volatile("global_store_dwordx2 %0, %1, off" ::"v"(g), "v"(gv) : "memory");   // stays in this XCD's L2 (the readers' sc1 loads find it there)
                        else __hip_atomic_store(g, gv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
                PD_PROF2(14);
                s = s_next;
                s_next = RESIDENT ? n_local : __builtin_amdgcn_readfirstlane(t_claim);
            }
            PD_PROF(1);
            if (k > 1) {
                // all-gather of every item's 12 sums: the data IS the flag (tag == epoch)
                const u64 *slot = xchg + (size_t)(epoch & 1) * P.xchg_stride;
                bool fail = false;
                // each item is one 128-byte line of 16 granules (12 used); a thread fetches 16-byte pieces
                // (2 granules) with write-through-coherent (sc1) loads, up to 3 pieces in flight per pass
                const int n_piece = (PD_GGS_ABLATE & 32) ? 0 : n_items * 6;
                for (int p0 = tid; p0 < n_piece; p0 += 3 * NT) {
                    const u64 *a[3];
                    int pi_[3];
#pragma unroll
                    for (int u = 0; u < 3; ++u) {
                        const int pc = p0 + u * NT;
                        pi_[u] = pc < n_piece ? pc : p0;
                        a[u] = slot + (size_t)(pi_[u] / 6) * PD_XCHG_LINE + (pi_[u] % 6) * 2;
                    }
                    u32x4 v0, v1, v2;
                    unsigned spins = 0;
                    for (;;) {
                        asm volatile("global_load_dwordx4 %0, %3, off sc1\n\t"
                                     "global_load_dwordx4 %1, %4, off sc1\n\t"
                                     "global_load_dwordx4 %2, %5, off sc1\n\t"
                                     "s_waitcnt vmcnt(0)"
                                     : "=&v"(v0), "=&v"(v1), "=&v"(v2)
                                     : "v"(a[0]), "v"(a[1]), "v"(a[2])
                                     : "memory");
                        const bool ok = v0[1] == epoch && v0[3] == epoch && v1[1] == epoch && v1[3] == epoch &&
                                        v2[1] == epoch && v2[3] == epoch;
                        if (ok) break;
                        if (++spins > (1u << 20) ||
                            ((spins & 255u) == 0 &&
                             __hip_atomic_load(P.err_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
                            fail = true;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(1);
                    }
                    const u32x4 vv[3] = {v0, v1, v2};
#pragma unroll
                    for (int u = 0; u < 3; ++u) {
                        if (p0 + u * NT < n_piece) {
                            const int g = (pi_[u] / 6) * PD_ITEM_VALS + (pi_[u] % 6) * 2;
                            L.item[g] = __uint_as_float(vv[u][0]);
                            L.item[g + 1] = __uint_as_float(vv[u][2]);
                        }
                    }
                }
                if (fail) {
                    atomicOr(P.err_flag, 1u);
                    L.ctl[1] = 1.0f;
                }
            }
            __syncthreads();
            if (L.ctl[1] != 0.0f) {   // a bounded spin gave up: abort the whole workgroup
                if (STAGE_P > 0) pd_vmcnt<0>();
                return;
            }
            PD_PROF(2);

            // ---- P3a: pair backward, one thread per frame pair, in chunks of PD_GGS_THREADS pairs (one chunk up to 32 frames) ----
            // results go to LDS rows of 16 floats per (pair, side): 9 dL/dRc_side + 3 dL/dtc_side + the pair's 4 dL/dA partials (side 0;
            // zeros on side 1).  P3b sums the first twelve per frame in fixed order; of the last four only the sum over ALL rows is needed
            // (the focal length is the mean over frames, geometry_guided_sampling.py:142): an idle wave forms it
            const bool need_rt = S.update_R || S.update_T;
            // totals over all items by one wave: one 16-byte read per item gets {dF22, sum(s valid), n_valid, sum(min(s, max))}
            auto loss_totals = [&]() {
                float s_sum = 0.0f, s_cnt = 0.0f, s_cl = 0.0f;
                for (int q2 = lane; q2 < n_items; q2 += 64) {
                    const float4 v4 = *(const float4 *)&L.item[q2 * PD_ITEM_VALS + 8];
                    s_sum += v4.y;
                    s_cnt += v4.z;
                    s_cl += v4.w;
                }
                s_sum = wave_allsum(s_sum);
                s_cnt = wave_allsum(s_cnt);
                s_cl = wave_allsum(s_cl);
                if (lane == 0) {
                    L.cam[6] = s_sum;
                    L.cam[7] = s_cnt;
                    L.ctl[2] = s_cl;
                }
            };
            for (int ck = 0; ck < D.n_pchunks; ++ck) {
                const int *coff = L.incoff + ck * 68;   // this chunk's incidences by frame (CSR positions within L.pinc; general path)
                {
                    // ONE thread per frame pair runs the shared backward chain once and writes both sides' results straight into
                    // their rows.  190 threads = 3 waves, one per SIMD: the cost is per wave-instruction.
                    const int pair = ck * PD_GGS_THREADS + tid;
                    if (p3t && pair < D.n_pairs && !(PD_GGS_ABLATE & 2)) {
                        const int4 mp = (ck == 0) ? make_int4(my_pair_xz & 0xffff, my_pair_y, (int)((unsigned)my_pair_xz >> 16), my_pair_w) : D.ptab[pair];
                        const int pi = mp.x & 0xff, pj = mp.x >> 8, nit = mp.z;
                        float G[9];
#pragma unroll
                        for (int c = 0; c < 9; ++c) G[c] = 0.0f;
                        for (int u = 0; u < nit; ++u)
#pragma unroll
                            for (int c = 0; c < 9; ++c) G[c] += L.item[(mp.y + u) * PD_ITEM_VALS + c];
#include "pd_ggs_pairbwd.inc"
                    }
                    // the quaternion Jacobian of this iteration's parameters, on a wave the pair backward leaves idle (<= 276 pairs: waves 0 .. 4), read by P3b behind the
                    // barrier below.  (Round 6: until here it ran at the top of the iteration, where a one-item-per-wave sequence -- B = 1, k = 24 -- has nothing to hide it
                    // behind: every wave waited at P1's barrier for this one.)
                    if (ck == 0 && wave == PD_GGS_WAVES - 1 && S.update_R && fast34) jac_all(L, lane, N);
                }
                if (prof) { pq = __builtin_readcyclecounter(); if (lane == 0) L.prof[6] += pq - pc; }
                __syncthreads();
                if (prof) { const long long n_ = __builtin_readcyclecounter(); if (lane == 0) L.prof[7] += n_ - pq; pq = n_; }
                // ---- P3b: per-frame sums over the rows of this chunk, fixed (ascending) order ----
                if (PD_GGS_ABLATE & 4) {
                } else if (fast34) {
#include "pd_ggs_p3b.inc"
                    if (wave >= n_row_waves && wave == W_LOSS) {
                        loss_totals();
                    }
                } else {         // several passes over the frames, partial sums carried across chunks in LDS
                    for (int n0 = 0; n0 < N; n0 += PD_GGS_THREADS / 16) {
                        const int n = n0 + fb_n;
                        if (p3t && n < N) {
                            const int lo = coff[n], hi = coff[n + 1];
                            float acc2 = (ck == 0) ? 0.0f : L.psum[n * 16 + fb_c];
                            for (int e = lo; e < hi; e += 16) {   // 16 LDS loads in flight, summed in order
                                float t16[16];
#pragma unroll
                                for (int u = 0; u < 16; ++u) t16[u] = L.pinc[min(e + u, hi - 1) * 16 + fb_c];
#pragma unroll
                                for (int u = 0; u < 16; ++u) acc2 += (e + u < hi) ? t16[u] : 0.0f;
                            }
                            L.psum[n * 16 + fb_c] = acc2;
                        }
                    }
                }
                if (prof) { const long long n_ = __builtin_readcyclecounter(); if (lane == 0) L.prof[8] += n_ - pq; pq = n_; }
                if (ck + 1 < D.n_pchunks) __syncthreads();   // the rows (and the dL/dA slots) are rewritten by the next chunk
            }
            if (!fast34) {
                if (wave == W_LOSS) loss_totals();
                __syncthreads();                         // every frame's sums are complete
                // the same seven numbers per frame as the fast path hands to P4: dL/dq through the Jacobian, dL/dT (signs: D = diag(-1,-1,1))
                for (int q = tid; q < N * 8; q += NT) {
                    const int n = q >> 3, x = q & 7;
                    float v = 0.0f;
                    if (x < 4) {
                        if (S.update_R) {
                            const float qn[4] = {L.xst[n * PD_XS_STRIDE + 3], L.xst[n * PD_XS_STRIDE + 4], L.xst[n * PD_XS_STRIDE + 5], L.xst[n * PD_XS_STRIDE + 6]};
                            float Wr[9];
                            jac_row_x(qn, x, Wr);
                            const float *ps = L.psum + n * 16;
#pragma unroll
                            for (int m = 0; m < 9; ++m) v = __builtin_fmaf(m < 6 ? -ps[m] : ps[m], Wr[m], v);
                        }
                    } else if (x < 7) {
                        if (S.update_T) {
                            const float t = L.psum[n * 16 + 9 + (x - 4)];
                            v = (x - 4 < 2) ? -t : t;
                        }
                    }
                    L.gq[q] = v;
                }
                // dL/dA totals over the frames, in frame order
                if (tid < 4) {
                    float v = 0.0f;
                    for (int n = 0; n < N; ++n) v += L.psum[n * 16 + 12 + tid];
                    L.gA[tid] = v;
                }
            }
            __syncthreads();
            PD_PROF(3);

#include "pd_ggs_p4q.inc"
            __syncthreads();
            PD_PROF(4);
            if (prof && lane == 0) L.prof[5] += 1;
            if (L.ctl[0] != 0.0f) break;
        }
        if (wave == 0 && lane == 0 && wg == 0 && P.stats) {
            float *so = P.stats + ((size_t)b * P.n_stages + st) * 4;
            so[0] = L.ctl[5];
            so[1] = (float)stepped;
            so[2] = L.ctl[6];
            so[3] = L.ctl[7];
        }
        if (P.eval_only) break;
    }
    if (prof && lane == 0) {
        for (int i = 0; i < 16; ++i) P.prof[i] = L.prof[i];
    }
    if (own && wg == 0 && !P.eval_only) {
#pragma unroll
        for (int c = 0; c < 9; ++c) xg[lane * 9 + c] = L.xst[lane * PD_XS_STRIDE + c];
    }
    if (STAGE_P > 0) pd_vmcnt<0>();   // the look-ahead LDS-DMA of the last item must land before the LDS is handed on
}

// --------------------------------------------------------------------------------------------
// the two-hop kernel for many frames (N > 32: several chunks of pairs)
//
// pd_ggs_kernel lets EVERY workgroup of a sequence gather all item sums and back-propagate all pairs;
// that replication is cheap at N = 20 (190 pairs) and dominates at N = 50 (1 225 pairs: 18 MB of
// exchange reads and 3 chunks of pair backward per iteration and workgroup).  Here the backward is
// distributed instead -- same arithmetic per pair and per frame, two small exchanges per iteration:
//   P1/P2  as before, but a workgroup keeps its items' sums to itself (needs one item per pair);
//   P3a    it back-propagates only ITS pairs and publishes the two 16-float results of each pair as
//          one exchange line per (pair, side), at the row the frame-sorted order gives it   (hop 1)
//   P3b    the owner of frame n (workgroup n % k) gathers that frame's rows, sums them in row order and
//          publishes the frame's 16 gradient sums; every workgroup also publishes its loss totals   (hop 2)
//   P4     every workgroup gathers the N frame lines + k total lines (a few KB) and runs the update.
// Exchange lines live in the sequence's slot of the same tagged-granule buffer:
//   [0, n_inc) (pair, side) rows | [n_inc, n_inc + k) per-workgroup totals | [n_inc + k, + N) per-frame sums.
// --------------------------------------------------------------------------------------------
template <int U>
__device__ __forceinline__ bool ggs2_gather(const u64 *src_lines, int piece0, int n_piece, int pieces_per_line, unsigned epoch,
                                            float *dst, int dst_stride, unsigned *err_flag) {
    // piece p = (line p / pieces_per_line, 16-byte part p % pieces_per_line) -> dst[line * dst_stride + 2 * part .. + 1]
    bool fail = false;
    for (int p0 = piece0; p0 < n_piece; p0 += U * PD_GGS_THREADS) {
        unsigned spins = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int p = p0 + u * PD_GGS_THREADS;
            if (p < n_piece) {
                const int line = p / pieces_per_line, part = p - line * pieces_per_line;
                const u64 *a = src_lines + (size_t)line * PD_XCHG_LINE + part * 2;
                u32x4 v;
                for (;;) {
                    asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"(a) : "memory");
                    if (v[1] == epoch && v[3] == epoch) break;
                    if (++spins > (1u << 20) ||
                        ((spins & 255u) == 0 && __hip_atomic_load(err_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
                        fail = true;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
                dst[line * dst_stride + part * 2] = __uint_as_float(v[0]);
                dst[line * dst_stride + part * 2 + 1] = __uint_as_float(v[2]);
            }
        }
    }
    return !fail;
}

__global__ __launch_bounds__(PD_GGS_THREADS) void pd_ggs2_kernel(PdGgsParams P, int B, int n_slots) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x % B, wg = blockIdx.x / B;
    if (b >= P.n_seqs) return;
    const PdSeqDesc D = P.seqs[b];
    const int N = D.n_frames, k = P.k;   // this sequence's own frame count (pd_ggs_plan checked it: P.N, or its entry of pd_engine_set_frame_counts); rows of x stay P.N apart
    const int nW = k * PD_GGS_WAVES;
    const int n_items = D.n_items;          // == D.n_pairs (one item per pair)
    const int n_inc = 2 * D.n_pairs;
    const Lds L = carve(smem, n_slots, PD_GGS_PINC_ROWS, n_slots);
    float *xg = P.x + (size_t)b * P.N * PD_POSE_DIM;
    u64 *xbase = P.xchg + (size_t)b * 2 * P.xchg_stride;
    // LDS reuse: L.item holds this workgroup's item sums [n_slots][12]; L.pinc rows [0, 2 n_slots <= 512) the results of
    // its pairs, rows [512, 576) the gathered rows of an owned frame, rows [640, 704) the gathered totals [k <= 256][4],
    // rows [768, 800) the exchange row of each local (pair, side); L.psum the gathered frame sums [N][16]
    float *own_rows = L.pinc;
    float *frame_rows = L.pinc + 512 * 16;
    float *tot_rows = L.pinc + 640 * 16;
    int *grow = (int *)(L.pinc + 768 * 16);

    const bool own = (wave == 0 && lane < N);
    if (wave == 0) {
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            L.xst[lane * PD_XS_STRIDE + c] = own ? xg[lane * 9 + c] : 0.0f;
            L.mst[lane * PD_XS_STRIDE + c] = 0.0f;
        }
    }
    for (int s = tid; s < n_slots; s += PD_GGS_THREADS) {
        const int item = wg * PD_GGS_WAVES + (s & 7) + (s >> 3) * nW;
        int4 e = make_int4(0, 0, 0, 0);
        int2 gp = make_int2(0, 0);
        if (item < n_items) {
            const int4 it = D.items[item];
            const int2 ij = D.pair_ij[it.x];
            e = make_int4(it.y, it.z, ij.x, ij.y);
            gp = D.gpos[it.x];
        }
        L.itab[s] = e;
        grow[2 * s] = gp.x;
        grow[2 * s + 1] = gp.y;
    }
    for (int q = tid; q <= N; q += PD_GGS_THREADS) L.incoff[q] = D.ginc_off[q];
    if (tid == 0) {
        L.ctl[0] = 0.0f;
        L.ctl[1] = 0.0f;
    }
    if (wave == 0) {
        float xr0[9];
        params_load(L.xst, lane, xr0);
        decode_all(L, xr0, lane, N, D);
    }
    __syncthreads();
    // one item per wave (the usual case here: k = ceil(pairs / 8)): its matches stay in registers for the whole launch
    const bool resident = (n_slots == PD_GGS_WAVES);
    float4 mres[8];
    {
        const int4 e = L.itab[wave];
        const int last = e.y > 0 ? e.y - 1 : 0;
        const float4 *pts = D.pts + e.x;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int m = lane + 64 * q;
            mres[q] = (resident && e.y > 0) ? pts[m < e.y ? m : last] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    unsigned epoch = 0;
    int trace_row = 0;
    const float inv_M = 1.0f / (float)D.M;
    // phase clocks (pd_debug_ggs_prof; round 5): wave 0 of workgroup 0 (owner of frame 0) -> prof[0..7], of the last workgroup (owns no frame when
    // k > N) -> prof[8..15]: {P1, P2, P3a, hop-1 publish + totals, P3b owner loop, hop-2 gathers, frame gradients + totals, P4}, shader cycles
    const bool prof2 = P.prof != nullptr && b == 0 && wave == 0 && (wg == 0 || wg == k - 1);
    long long q0 = 0, q1 = 0, q2 = 0, q3 = 0, q4 = 0, q5 = 0, q6 = 0, q7 = 0, qc = 0;
#define PD_PROF2H(acc) do { if (prof2) { const long long n_ = __builtin_amdgcn_s_memtime(); acc += n_ - qc; qc = n_; } } while (0)
    for (int st = 0; st < P.n_stages; ++st) {
        const PdGgsStage S = P.stages[st];
        int stepped = 0;
        float last_print = __int_as_float(0x7fc00000), last_cnt = 0.0f, last_loss = __int_as_float(0x7fc00000);
        const bool need_rt = S.update_R || S.update_T;
        for (int it = 0; it < S.iters; ++it) {
            if (prof2) qc = __builtin_amdgcn_s_memtime();
            // ---- P1: F for the pairs of this workgroup's items
            const Cam cam = {L.cam[0], L.cam[1], L.cam[2], L.cam[3]};
            for (int s = tid; s < n_slots; s += PD_GGS_THREADS) {
                const int4 e = L.itab[s];
                if (e.y > 0) {
                    float Ri[9], Rj[9], ti[3], tj[3];
                    frame_load(L, e.z, Ri, ti);
                    frame_load(L, e.w, Rj, tj);
                    PairFwd f;
                    pair_forward(Ri, ti, Rj, tj, f);
                    float F[9];
                    fundamental_from_E(f.E, cam, F);
#pragma unroll
                    for (int c = 0; c < 9; ++c) L.F[s * PD_F_STRIDE + c] = F[c];
                }
            }
            __syncthreads();
            PD_PROF2H(q0);
            // ---- P2: per-match Sampson residual + dL/dF, a wave per item; the 12 sums stay in this workgroup's LDS
            ++epoch;
            u64 *xs = xbase + (size_t)(epoch & 1) * P.xchg_stride;
            for (int r = 0; r * PD_GGS_WAVES < n_slots; ++r) {
                const int s = wave + PD_GGS_WAVES * r;
                const int4 e = L.itab[s];
                if (e.y > 0) {
                    float Fm[9];
                    {   // three LDS reads (slot stride 12 floats, 16-byte aligned) instead of nine 4-byte ones
                    const float4 f0 = *(const float4 *)(L.F + s * PD_F_STRIDE), f1 = *(const float4 *)(L.F + s * PD_F_STRIDE + 4);
                    Fm[0] = f0.x; Fm[1] = f0.y; Fm[2] = f0.z; Fm[3] = f0.w;
                    Fm[4] = f1.x; Fm[5] = f1.y; Fm[6] = f1.z; Fm[7] = f1.w;
                    Fm[8] = L.F[s * PD_F_STRIDE + 8];
                }
                    v2f acc2[PD_ITEM_VALS];
                    int nv;
                    if (resident) {
                        item_pass<false>(MatchRegs{mres}, e.y, lane, Fm, P.sampson_max, acc2, nv);
                    } else {
                        float4 mb[8];
                        const float4 *pts = D.pts + e.x;
                        const int last = e.y - 1;
#pragma unroll
                        for (int q = 0; q < 8; ++q) {
                            const int m = lane + 64 * q;
                            mb[q] = pts[m < e.y ? m : last];
                        }
                        item_pass<false>(MatchRegs{mb}, e.y, lane, Fm, P.sampson_max, acc2, nv);
                    }
                    int slot;
                    const float tot = item_totals(acc2, nv, e.y, P.sampson_max, lane, slot);
                    if (lane < 16 && slot < PD_ITEM_VALS) L.item[s * PD_ITEM_VALS + slot] = tot;
                }
            }
            __syncthreads();
            PD_PROF2H(q1);
            // ---- P3a: backward of this workgroup's pairs (thread per local item), rows 2s (side 0), 2s + 1 (side 1)
            if (tid < n_slots && L.itab[tid].y > 0) {
                const int4 e = L.itab[tid];
                const int pi = e.z, pj = e.w;
                const int4 mp = make_int4(0, 0, 1, (2 * tid) | ((2 * tid + 1) << 16));
                float G[9];
#pragma unroll
                for (int c = 0; c < 9; ++c) G[c] = L.item[tid * PD_ITEM_VALS + c];
#include "pd_ggs_pairbwd.inc"
            }
            __syncthreads();
            PD_PROF2H(q2);
            // ---- hop 1: publish the (pair, side) rows; thread (row = tid / 16, component = tid % 16), 32 rows per pass
            for (int r0 = 0; r0 < 2 * n_slots; r0 += PD_GGS_THREADS / 16) {
                const int row = r0 + (tid >> 4);
                if (row < 2 * n_slots && L.itab[row >> 1].y > 0) {
                    u64 *g = xs + (size_t)grow[row] * PD_XCHG_LINE + (tid & 15);
                    __hip_atomic_store(g, ((u64)epoch << 32) | (u64)__float_as_uint(own_rows[row * 16 + (tid & 15)]), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            // this workgroup's loss totals {sum s valid, n valid, sum min(s, max)} -> its totals line
            if (wave == PD_GGS_WAVES - 1) {
                float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;
                for (int s = lane; s < n_slots; s += 64) {
                    if (L.itab[s].y > 0) {
                        t0 += L.item[s * PD_ITEM_VALS + 9];
                        t1 += L.item[s * PD_ITEM_VALS + 10];
                        t2 += L.item[s * PD_ITEM_VALS + 11];
                    }
                }
                t0 = wave_allsum(t0);
                t1 = wave_allsum(t1);
                t2 = wave_allsum(t2);
                if (lane < 4) {
                    const float v = lane == 0 ? t0 : (lane == 1 ? t1 : (lane == 2 ? t2 : 0.0f));
                    __hip_atomic_store(xs + (size_t)(n_inc + wg) * PD_XCHG_LINE + lane, ((u64)epoch << 32) | (u64)__float_as_uint(v),
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            PD_PROF2H(q3);
            // ---- P3b: the owner of frame n sums that frame's rows in row order and publishes the frame line
            bool ok = true;
            for (int n = wg; n < N; n += k) {
                const int lo = L.incoff[n], cn = L.incoff[n + 1] - lo;   // <= 2 (N - 1) <= 126 rows
                ok = ggs2_gather<1>(xs + (size_t)lo * PD_XCHG_LINE, tid, cn * 8, 8, epoch, frame_rows, 16, P.err_flag) && ok;
                __syncthreads();
                if (tid < 64) {
                    // the frame's rows summed in a FIXED order that does not depend on the workgroup count: the four 16-lane rows of wave 0 each sum
                    // every fourth row (rows p, p + 4, ...: eight LDS reads in flight at a time), then (p0 + p1) + (p2 + p3) on the permlane swaps.
                    // History (tools/ggs_prof_n50.py, round 5): a plain loop over the rows was a chain of <= 63 dependent LDS round trips -- 5 700 of the
                    // 22 100 cycles of an iteration at 50 frames; eight reads in flight on 16 lanes: 3 300; this form: see profiles/round5_ggs_n50_phase_clocks.txt
                    const int c16 = tid & 15, part = tid >> 4;
                    float a = 0.0f;
                    for (int e0 = part; e0 < cn; e0 += 32) {              // (cn <= 2 (N - 1) rows; the loop bound differs between the four parts: no cross-lane operation inside)
                        float r[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) r[u] = e0 + 4 * u < cn ? frame_rows[(e0 + 4 * u) * 16 + c16] : 0.0f;
#pragma unroll
                        for (int u = 0; u < 8; ++u) a += r[u];
                    }
                    a = add_xor16(a);
                    a = add_xor32(a);
                    if (tid < 16)
                        __hip_atomic_store(xs + (size_t)(n_inc + k + n) * PD_XCHG_LINE + tid, ((u64)epoch << 32) | (u64)__float_as_uint(a),
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                __syncthreads();
            }
            PD_PROF2H(q4);
            // ---- hop 2: everybody gathers the N frame lines and the k totals lines
            ok = ggs2_gather<2>(xs + (size_t)(n_inc + k) * PD_XCHG_LINE, tid, N * 8, 8, epoch, L.psum, 16, P.err_flag) && ok;
            ok = ggs2_gather<1>(xs + (size_t)n_inc * PD_XCHG_LINE, tid, k * 2, 2, epoch, tot_rows, 4, P.err_flag) && ok;
            if (!ok) {
                atomicOr(P.err_flag, 1u);
                L.ctl[1] = 1.0f;
            }
            __syncthreads();
            if (L.ctl[1] != 0.0f) return;
            PD_PROF2H(q5);
            // per-frame gradients back through tc = D T and Rc[a][b] = D[a] R[b][a]; totals in workgroup order
            for (int q = tid; q < N * 16; q += PD_GGS_THREADS) {
                const int n = q >> 4, c = q & 15;
                const float v = L.psum[n * 16 + c];
                if (c < 9) {
                    const int aa = c / 3, bb = c % 3;
                    L.gR[n * 9 + bb * 3 + aa] = (aa < 2 ? -v : v);
                } else if (c < 12) {
                    L.gT[n * 3 + (c - 9)] = (c - 9 < 2 ? -v : v);
                } else {
                    L.gA[n * 4 + (c - 12)] = v;
                }
            }
            if (wave >= PD_GGS_WAVES - 3) {                 // one wave per total (round 5: one wave ran the 3 x ceil(k / 64) reductions back to back)
                const int c = wave - (PD_GGS_WAVES - 3);
                float t = 0.0f;
                for (int w0 = 0; w0 < k; w0 += 64) {      // fixed order: 64 workgroups at a time, tree inside
                    const int w = w0 + lane;
                    t += wave_allsum(w < k ? tot_rows[w * 4 + c] : 0.0f);
                }
                if (lane == 0) *(c == 0 ? &L.cam[6] : (c == 1 ? &L.cam[7] : &L.ctl[2])) = t;
            }
            __syncthreads();
            PD_PROF2H(q6);
#include "pd_ggs_p4.inc"
            __syncthreads();
            PD_PROF2H(q7);
            if (L.ctl[0] != 0.0f) break;
        }
        if (wave == 0 && lane == 0 && wg == 0 && P.stats) {
            float *so = P.stats + ((size_t)b * P.n_stages + st) * 4;
            so[0] = last_print;
            so[1] = (float)stepped;
            so[2] = last_cnt;
            so[3] = last_loss;
        }
        if (P.eval_only) break;
    }
    if (prof2 && lane == 0) {
        long long *o = P.prof + (wg == 0 ? 0 : 8);
        o[0] = q0; o[1] = q1; o[2] = q2; o[3] = q3; o[4] = q4; o[5] = q5; o[6] = q6; o[7] = q7;
    }
#undef PD_PROF2H
    if (own && wg == 0 && !P.eval_only) {
#pragma unroll
        for (int c = 0; c < 9; ++c) xg[lane * 9 + c] = L.xst[lane * PD_XS_STRIDE + c];
    }
}

// --------------------------------------------------------------------------------------------
// the two-hop scheme for up to 256 frames (PD_OPT_GGS_MAX_FRAMES above 64; PD_GGS_CFG_LONG_FRAMES at any N)
//
// pd_ggs2_kernel's structure, exchange and arithmetic -- P1, P2, P3a, hop 1, P3b, hop 2, P4; the same tagged granules, bounded spins and
// fixed summation orders -- on the LDS image of carve_long (pd_ggs_lds.h): frame tables for 256 frames and a 512-row window for the
// gathered rows of a frame.  What was "lane = frame on wave 0" there (the parameter load, decode_all, P4, the final store) is
// "thread = frame on waves 0 .. 3" here; the sums over the frames inside those phases go wave_allsum per wave, then (w0 + w1) + (w2 + w3)
// through L.red.  At N <= 64 waves 1 .. 3 add +0 and every result is bitwise pd_ggs2_kernel's (tests/test_gpu_ggs_long.py).
// --------------------------------------------------------------------------------------------
// decode_all for thread = frame: called by ALL threads of the workgroup (one workgroup barrier inside when do_fl; do_* are block-uniform)
__device__ __forceinline__ void decode_all_long(const LdsLong &L, const float *xr, int tid, int N, const PdSeqDesc &D, bool do_r = true,
                                                bool do_t = true, bool do_fl = true) {
    const int lane = tid & 63, wave = tid >> 6;
    if (tid < N) {
        float *dst = L.Rc + tid * PD_FR_STRIDE;
        if (do_r) {
            float Rc[9];
            decode_frame_r(xr, Rc);
            ((float4 *)dst)[0] = make_float4(Rc[0], Rc[1], Rc[2], Rc[3]);
            ((float4 *)dst)[1] = make_float4(Rc[4], Rc[5], Rc[6], Rc[7]);
            dst[8] = Rc[8];
        }
        if (do_t) decode_frame_t(xr, dst + 9);
    }
    if (!do_fl) return;                               // (block-uniform)
    float flx = 0.f, fly = 0.f, px = 0.f, py = 0.f;
    if (tid < N) {
        decode_frame_fl(xr, flx, fly, px, py);
        *(float4 *)&L.fl[tid * 4] = make_float4(flx, fly, px, py);
    }
    // focal_length.mean(dim=0) over all cameras (geometry_guided_sampling.py:142): decode_all's tree per wave, then the four waves
    int n_op = N;
    asm volatile("" : "+s"(n_op));
    const float rN = pd_rcp((float)n_op);
    float fbx, fby;
    wave_allsum2(flx, fly, fbx, fby);
    if (wave < 4 && lane == 0) {
        L.red[24 + wave] = fbx;
        L.red[28 + wave] = fby;
    }
    __syncthreads();
    if (tid == 0) {
        fbx = (L.red[24] + L.red[25]) + (L.red[26] + L.red[27]);
        fby = (L.red[28] + L.red[29]) + (L.red[30] + L.red[31]);
        fbx *= rN;
        fby *= rN;
        const float a0 = pd_rcp(fbx * D.sc), a1 = pd_rcp(fby * D.sc);
        L.cam[0] = a0;
        L.cam[1] = a1;
        L.cam[2] = -D.cx * a0;
        L.cam[3] = -D.cy * a1;
        L.cam[4] = fbx;
        L.cam[5] = fby;
    }
}

__global__ __launch_bounds__(PD_GGS_THREADS) void pd_ggs_long_kernel(PdGgsParams P, int B, int n_slots, int n_batch) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x % B, wg = blockIdx.x / B;
    if (b >= P.n_seqs) return;
    const PdSeqDesc D = P.seqs[b];
    const int N = D.n_frames, k = P.k;   // this sequence's own frame count (pd_ggs_plan checked it: P.N, or its entry of pd_engine_set_frame_counts); rows of x stay P.N apart
    const int nW = k * PD_GGS_WAVES;
    const int n_items = D.n_items;          // == D.n_pairs (one item per pair)
    const int n_inc = 2 * D.n_pairs;
    const LdsLong L = carve_long(smem, n_slots, n_batch);
    float *xg = P.x + (size_t)b * P.N * PD_POSE_DIM;
    u64 *xbase = P.xchg + (size_t)b * 2 * P.xchg_stride;
    // the hop windows of the image (carve_long): L.item the item sums of a batch of this workgroup's slots [n_batch][12]; own_rows the results
    // of its pairs [2 n_batch][16]; frame_rows the gathered rows of an owned frame (<= 2 (N - 1) <= 510); tot_rows the gathered totals [k <= 256][4];
    // grow the exchange row of each local (pair, side); L.psum the gathered frame sums [N][16]
    float *own_rows = L.own_rows;
    float *frame_rows = L.frame_rows;
    float *tot_rows = L.tot_rows;
    int *grow = L.grow;

    // thread tid < 256 (waves 0 .. 3) owns frame tid: parameters + momentum live in LDS (L.xst / L.mst) and visit registers only inside P4
    const bool own = tid < N;
    if (tid < PD_GGS_LONG_FRAMES) {
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            L.xst[tid * PD_XS_STRIDE + c] = own ? xg[tid * 9 + c] : 0.0f;
            L.mst[tid * PD_XS_STRIDE + c] = 0.0f;
        }
    }
    for (int s = tid; s < n_slots; s += PD_GGS_THREADS) {
        const int item = wg * PD_GGS_WAVES + (s & 7) + (s >> 3) * nW;
        int4 e = make_int4(0, 0, 0, 0);
        int2 gp = make_int2(0, 0);
        if (item < n_items) {
            const int4 it = D.items[item];
            const int2 ij = D.pair_ij[it.x];
            e = make_int4(it.y, it.z, ij.x, ij.y);
            gp = D.gpos[it.x];
        }
        L.itab[s] = e;
        grow[2 * s] = gp.x;
        grow[2 * s + 1] = gp.y;
    }
    for (int q = tid; q <= N; q += PD_GGS_THREADS) L.incoff[q] = D.ginc_off[q];
    if (tid == 0) {
        L.ctl[0] = 0.0f;
        L.ctl[1] = 0.0f;
    }
    {
        float xr0[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) xr0[c] = 0.0f;
        if (tid < PD_GGS_LONG_FRAMES) params_load(L.xst, tid, xr0);
        decode_all_long(L, xr0, tid, N, D);
    }
    __syncthreads();
    // one item per wave (the usual case here: k = ceil(pairs / 8)): its matches stay in registers for the whole launch
    const bool resident = (n_slots == PD_GGS_WAVES);
    float4 mres[8];
    {
        const int4 e = L.itab[wave];
        const int last = e.y > 0 ? e.y - 1 : 0;
        const float4 *pts = D.pts + e.x;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int m = lane + 64 * q;
            mres[q] = (resident && e.y > 0) ? pts[m < e.y ? m : last] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    unsigned epoch = 0;
    int trace_row = 0;
    const float inv_M = 1.0f / (float)D.M;
    // phase clocks (pd_debug_ggs_prof; round 5): wave 0 of workgroup 0 (owner of frame 0) -> prof[0..7], of the last workgroup (owns no frame when
    // k > N) -> prof[8..15]: {P1, P2, P3a, hop-1 publish + totals, P3b owner loop, hop-2 gathers, frame gradients + totals, P4}, shader cycles
    const bool prof2 = P.prof != nullptr && b == 0 && wave == 0 && (wg == 0 || wg == k - 1);
    long long q0 = 0, q1 = 0, q2 = 0, q3 = 0, q4 = 0, q5 = 0, q6 = 0, q7 = 0, qc = 0;
#define PD_PROF2H(acc) do { if (prof2) { const long long n_ = __builtin_amdgcn_s_memtime(); acc += n_ - qc; qc = n_; } } while (0)
    for (int st = 0; st < P.n_stages; ++st) {
        const PdGgsStage S = P.stages[st];
        int stepped = 0;
        float last_print = __int_as_float(0x7fc00000), last_cnt = 0.0f, last_loss = __int_as_float(0x7fc00000);
        const bool need_rt = S.update_R || S.update_T;
        for (int it = 0; it < S.iters; ++it) {
            if (prof2) qc = __builtin_amdgcn_s_memtime();
            // P1 .. hop 1 run over the workgroup's slots in batches of n_batch (pd_ggs_plan: all of them in one batch where the image has the
            // room; a multiple of 64 otherwise): F, the item sums and the own rows live in LDS for one batch at a time, indexed by the slot's
            // position in its batch.  Nothing a pair computes depends on its batch, and the lanes of the totals wave keep their slots
            // (s % 64) across batches: the results are those of one batch.
            const Cam cam = {L.cam[0], L.cam[1], L.cam[2], L.cam[3]};
            ++epoch;
            u64 *xs = xbase + (size_t)(epoch & 1) * P.xchg_stride;
            float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;      // (totals wave) this workgroup's loss totals, per lane until the last batch is in
            for (int s0 = 0; s0 < n_slots; s0 += n_batch) {
                const int nb = min(n_batch, n_slots - s0);
                // ---- P1: F for the pairs of this workgroup's items
                for (int sl = tid; sl < nb; sl += PD_GGS_THREADS) {
                    const int4 e = L.itab[s0 + sl];
                    if (e.y > 0) {
                        float Ri[9], Rj[9], ti[3], tj[3];
                        frame_load(L, e.z, Ri, ti);
                        frame_load(L, e.w, Rj, tj);
                        PairFwd f;
                        pair_forward(Ri, ti, Rj, tj, f);
                        float F[9];
                        fundamental_from_E(f.E, cam, F);
#pragma unroll
                        for (int c = 0; c < 9; ++c) L.F[sl * PD_F_STRIDE + c] = F[c];
                    }
                }
                __syncthreads();
                PD_PROF2H(q0);
                // ---- P2: per-match Sampson residual + dL/dF, a wave per item; the 12 sums stay in this workgroup's LDS
                for (int r = 0; r * PD_GGS_WAVES < nb; ++r) {
                    const int sl = wave + PD_GGS_WAVES * r;
                    const int4 e = L.itab[s0 + sl];
                    if (e.y > 0) {
                        float Fm[9];
                        {   // three LDS reads (slot stride 12 floats, 16-byte aligned) instead of nine 4-byte ones
                            const float4 f0 = *(const float4 *)(L.F + sl * PD_F_STRIDE), f1 = *(const float4 *)(L.F + sl * PD_F_STRIDE + 4);
                            Fm[0] = f0.x; Fm[1] = f0.y; Fm[2] = f0.z; Fm[3] = f0.w;
                            Fm[4] = f1.x; Fm[5] = f1.y; Fm[6] = f1.z; Fm[7] = f1.w;
                            Fm[8] = L.F[sl * PD_F_STRIDE + 8];
                        }
                        v2f acc2[PD_ITEM_VALS];
                        int nv;
                        if (resident) {
                            item_pass<false>(MatchRegs{mres}, e.y, lane, Fm, P.sampson_max, acc2, nv);
                        } else {
                            float4 mb[8];
                            const float4 *pts = D.pts + e.x;
                            const int last = e.y - 1;
#pragma unroll
                            for (int q = 0; q < 8; ++q) {
                                const int m = lane + 64 * q;
                                mb[q] = pts[m < e.y ? m : last];
                            }
                            item_pass<false>(MatchRegs{mb}, e.y, lane, Fm, P.sampson_max, acc2, nv);
                        }
                        int slot;
                        const float tot = item_totals(acc2, nv, e.y, P.sampson_max, lane, slot);
                        if (lane < 16 && slot < PD_ITEM_VALS) L.item[sl * PD_ITEM_VALS + slot] = tot;
                    }
                }
                __syncthreads();
                PD_PROF2H(q1);
                // ---- P3a: backward of this workgroup's pairs (thread per item of the batch), rows 2 sl (side 0), 2 sl + 1 (side 1)
                if (tid < nb && L.itab[s0 + tid].y > 0) {
                    const int4 e = L.itab[s0 + tid];
                    const int pi = e.z, pj = e.w;
                    const int4 mp = make_int4(0, 0, 1, (2 * tid) | ((2 * tid + 1) << 16));
                    float G[9];
#pragma unroll
                    for (int c = 0; c < 9; ++c) G[c] = L.item[tid * PD_ITEM_VALS + c];
#include "pd_ggs_pairbwd.inc"
                }
                __syncthreads();
                PD_PROF2H(q2);
                // ---- hop 1: publish the (pair, side) rows; thread (row = tid / 16, component = tid % 16), 32 rows per pass
                for (int r0 = 0; r0 < 2 * nb; r0 += PD_GGS_THREADS / 16) {
                    const int row = r0 + (tid >> 4);
                    if (row < 2 * nb && L.itab[s0 + (row >> 1)].y > 0) {
                        u64 *g = xs + (size_t)grow[2 * s0 + row] * PD_XCHG_LINE + (tid & 15);
                        __hip_atomic_store(g, ((u64)epoch << 32) | (u64)__float_as_uint(own_rows[row * 16 + (tid & 15)]), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
                // this workgroup's loss totals {sum s valid, n valid, sum min(s, max)}: lane l takes slots l, l + 64, ... (n_batch % 64 == 0
                // whenever there are several batches)
                if (wave == PD_GGS_WAVES - 1) {
                    for (int sl = lane; sl < nb; sl += 64) {
                        if (L.itab[s0 + sl].y > 0) {
                            t0 += L.item[sl * PD_ITEM_VALS + 9];
                            t1 += L.item[sl * PD_ITEM_VALS + 10];
                            t2 += L.item[sl * PD_ITEM_VALS + 11];
                        }
                    }
                }
                // (the next batch's P1 writes L.F only, and its barrier stands before anything overwrites L.item or the own rows)
            }
            // ... -> its totals line
            if (wave == PD_GGS_WAVES - 1) {
                t0 = wave_allsum(t0);
                t1 = wave_allsum(t1);
                t2 = wave_allsum(t2);
                if (lane < 4) {
                    const float v = lane == 0 ? t0 : (lane == 1 ? t1 : (lane == 2 ? t2 : 0.0f));
                    __hip_atomic_store(xs + (size_t)(n_inc + wg) * PD_XCHG_LINE + lane, ((u64)epoch << 32) | (u64)__float_as_uint(v),
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            PD_PROF2H(q3);
#include "pd_ggs_long_hop2.inc"
#include "pd_ggs_p4_long.inc"
            __syncthreads();
            PD_PROF2H(q7);
            if (L.ctl[0] != 0.0f) break;
        }
        if (tid == 0 && wg == 0 && P.stats) {
            float *so = P.stats + ((size_t)b * P.n_stages + st) * 4;
            so[0] = last_print;
            so[1] = (float)stepped;
            so[2] = last_cnt;
            so[3] = last_loss;
        }
        if (P.eval_only) break;
    }
    if (prof2 && lane == 0) {
        long long *o = P.prof + (wg == 0 ? 0 : 8);
        o[0] = q0; o[1] = q1; o[2] = q2; o[3] = q3; o[4] = q4; o[5] = q5; o[6] = q6; o[7] = q7;
    }
#undef PD_PROF2H
    if (own && wg == 0 && !P.eval_only) {
#pragma unroll
        for (int c = 0; c < 9; ++c) xg[tid * 9 + c] = L.xst[tid * PD_XS_STRIDE + c];
    }
}

// pd_ggs_long_kernel with a slot = a frame PAIR instead of a work item (PD_OPT_GGS_LONG_PAIR_ITEMS): for launches in which some pair holds more
// than PD_ITEM_MAX_MATCHES matches.  Slot s of workgroup wg owns pair wg * 8 + (s & 7) + (s >> 3) * nW; the wave that owns the slot runs the
// match pass once per work item of the pair (the balanced cuts both table builders write: items[pair_item_off[p] ..]), in item order, and
// adds the twelve item totals.  One wave forms a pair's sums in a fixed order, so -- as in pd_ggs_long_kernel -- nothing the update reads
// depends on the workgroup count or the slot batches; a pair of one item goes through that kernel's very operations (same bits).  Everything
// outside the slot table, the resident matches and P2 is that kernel's text.
__global__ __launch_bounds__(PD_GGS_THREADS) void pd_ggs_longm_kernel(PdGgsParams P, int B, int n_slots, int n_batch) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x % B, wg = blockIdx.x / B;
    if (b >= P.n_seqs) return;
    const PdSeqDesc D = P.seqs[b];
    const int N = D.n_frames, k = P.k;   // this sequence's own frame count (pd_ggs_plan checked it: P.N, or its entry of pd_engine_set_frame_counts); rows of x stay P.N apart
    const int nW = k * PD_GGS_WAVES;
    const int n_pairs = D.n_pairs;          // a slot is a PAIR here; its items are D.items[pair_item_off[p] .. pair_item_off[p + 1])
    const int n_inc = 2 * D.n_pairs;
    const LdsLong L = carve_long(smem, n_slots, n_batch);
    float *xg = P.x + (size_t)b * P.N * PD_POSE_DIM;
    u64 *xbase = P.xchg + (size_t)b * 2 * P.xchg_stride;
    // the hop windows of the image (carve_long): L.item the item sums of a batch of this workgroup's slots [n_batch][12]; own_rows the results
    // of its pairs [2 n_batch][16]; frame_rows the gathered rows of an owned frame (<= 2 (N - 1) <= 510); tot_rows the gathered totals [k <= 256][4];
    // grow the exchange row of each local (pair, side); L.psum the gathered frame sums [N][16]
    float *own_rows = L.own_rows;
    float *frame_rows = L.frame_rows;
    float *tot_rows = L.tot_rows;
    int *grow = L.grow;

    // thread tid < 256 (waves 0 .. 3) owns frame tid: parameters + momentum live in LDS (L.xst / L.mst) and visit registers only inside P4
    const bool own = tid < N;
    if (tid < PD_GGS_LONG_FRAMES) {
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            L.xst[tid * PD_XS_STRIDE + c] = own ? xg[tid * 9 + c] : 0.0f;
            L.mst[tid * PD_XS_STRIDE + c] = 0.0f;
        }
    }
    for (int s = tid; s < n_slots; s += PD_GGS_THREADS) {
        const int p = wg * PD_GGS_WAVES + (s & 7) + (s >> 3) * nW;
        int4 e = make_int4(0, 0, 0, 0);        // (first item, items, i, j): .y > 0 marks an active slot, as the item's match count does in pd_ggs_long_kernel
        int2 gp = make_int2(0, 0);
        if (p < n_pairs) {
            const int first = D.pair_item_off[p];
            const int2 ij = D.pair_ij[p];
            e = make_int4(first, D.pair_item_off[p + 1] - first, ij.x, ij.y);
            gp = D.gpos[p];
        }
        L.itab[s] = e;
        grow[2 * s] = gp.x;
        grow[2 * s + 1] = gp.y;
    }
    for (int q = tid; q <= N; q += PD_GGS_THREADS) L.incoff[q] = D.ginc_off[q];
    if (tid == 0) {
        L.ctl[0] = 0.0f;
        L.ctl[1] = 0.0f;
    }
    {
        float xr0[9];
#pragma unroll
        for (int c = 0; c < 9; ++c) xr0[c] = 0.0f;
        if (tid < PD_GGS_LONG_FRAMES) params_load(L.xst, tid, xr0);
        decode_all_long(L, xr0, tid, N, D);
    }
    __syncthreads();
    // one pair per wave (the usual case here: k = ceil(pairs / 8)) and that pair ONE item: its matches stay in registers for the whole launch
    // (wave-uniform); a pair of several items streams every item from memory
    const int4 it_res = L.itab[wave].y == 1 ? D.items[L.itab[wave].x] : make_int4(0, 0, 0, 0);     // (pair, first match, matches, 0)
    const bool resident = (n_slots == PD_GGS_WAVES) && it_res.z > 0;
    float4 mres[8];
    {
        const int last = it_res.z > 0 ? it_res.z - 1 : 0;
        const float4 *pts = D.pts + it_res.y;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int m = lane + 64 * q;
            mres[q] = resident ? pts[m < it_res.z ? m : last] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    unsigned epoch = 0;
    int trace_row = 0;
    const float inv_M = 1.0f / (float)D.M;
    // phase clocks (pd_debug_ggs_prof; round 5): wave 0 of workgroup 0 (owner of frame 0) -> prof[0..7], of the last workgroup (owns no frame when
    // k > N) -> prof[8..15]: {P1, P2, P3a, hop-1 publish + totals, P3b owner loop, hop-2 gathers, frame gradients + totals, P4}, shader cycles
    const bool prof2 = P.prof != nullptr && b == 0 && wave == 0 && (wg == 0 || wg == k - 1);
    long long q0 = 0, q1 = 0, q2 = 0, q3 = 0, q4 = 0, q5 = 0, q6 = 0, q7 = 0, qc = 0;
#define PD_PROF2H(acc) do { if (prof2) { const long long n_ = __builtin_amdgcn_s_memtime(); acc += n_ - qc; qc = n_; } } while (0)
    for (int st = 0; st < P.n_stages; ++st) {
        const PdGgsStage S = P.stages[st];
        int stepped = 0;
        float last_print = __int_as_float(0x7fc00000), last_cnt = 0.0f, last_loss = __int_as_float(0x7fc00000);
        const bool need_rt = S.update_R || S.update_T;
        for (int it = 0; it < S.iters; ++it) {
            if (prof2) qc = __builtin_amdgcn_s_memtime();
            // P1 .. hop 1 run over the workgroup's slots in batches of n_batch (pd_ggs_plan: all of them in one batch where the image has the
            // room; a multiple of 64 otherwise): F, the item sums and the own rows live in LDS for one batch at a time, indexed by the slot's
            // position in its batch.  Nothing a pair computes depends on its batch, and the lanes of the totals wave keep their slots
            // (s % 64) across batches: the results are those of one batch.
            const Cam cam = {L.cam[0], L.cam[1], L.cam[2], L.cam[3]};
            ++epoch;
            u64 *xs = xbase + (size_t)(epoch & 1) * P.xchg_stride;
            float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;      // (totals wave) this workgroup's loss totals, per lane until the last batch is in
            for (int s0 = 0; s0 < n_slots; s0 += n_batch) {
                const int nb = min(n_batch, n_slots - s0);
                // ---- P1: F for this workgroup's pairs
                for (int sl = tid; sl < nb; sl += PD_GGS_THREADS) {
                    const int4 e = L.itab[s0 + sl];
                    if (e.y > 0) {
                        float Ri[9], Rj[9], ti[3], tj[3];
                        frame_load(L, e.z, Ri, ti);
                        frame_load(L, e.w, Rj, tj);
                        PairFwd f;
                        pair_forward(Ri, ti, Rj, tj, f);
                        float F[9];
                        fundamental_from_E(f.E, cam, F);
#pragma unroll
                        for (int c = 0; c < 9; ++c) L.F[sl * PD_F_STRIDE + c] = F[c];
                    }
                }
                __syncthreads();
                PD_PROF2H(q0);
                // ---- P2: per-match Sampson residual + dL/dF, a wave per PAIR: the pair's items in ascending order, each the pass and the totals
                // of pd_ggs_long_kernel (the exact-threshold re-run stays per item); the 12 values are added on the lanes that hold them -- item
                // 0's as they are, so a pair of one item gets that kernel's bits -- and only the sums reach this workgroup's LDS
                for (int r = 0; r * PD_GGS_WAVES < nb; ++r) {
                    const int sl = wave + PD_GGS_WAVES * r;
                    const int4 e = L.itab[s0 + sl];
                    if (e.y > 0) {
                        float Fm[9];
                        {   // three LDS reads (slot stride 12 floats, 16-byte aligned) instead of nine 4-byte ones
                            const float4 f0 = *(const float4 *)(L.F + sl * PD_F_STRIDE), f1 = *(const float4 *)(L.F + sl * PD_F_STRIDE + 4);
                            Fm[0] = f0.x; Fm[1] = f0.y; Fm[2] = f0.z; Fm[3] = f0.w;
                            Fm[4] = f1.x; Fm[5] = f1.y; Fm[6] = f1.z; Fm[7] = f1.w;
                            Fm[8] = L.F[sl * PD_F_STRIDE + 8];
                        }
                        int slot = PD_ITEM_VALS;
                        float sum = 0.0f;
                        if (resident) {
                            v2f acc2[PD_ITEM_VALS];
                            int nv;
                            item_pass<false>(MatchRegs{mres}, it_res.z, lane, Fm, P.sampson_max, acc2, nv);
                            sum = item_totals(acc2, nv, it_res.z, P.sampson_max, lane, slot);
                        } else {
                            for (int c = 0; c < e.y; ++c) {
                                const int4 it = D.items[e.x + c];          // (pair, first match, matches, 0): the tables are the one definition of the cuts
                                v2f acc2[PD_ITEM_VALS];
                                int nv;
                                float4 mb[8];
                                const float4 *pts = D.pts + it.y;
                                const int last = it.z - 1;
#pragma unroll
                                for (int q = 0; q < 8; ++q) {
                                    const int m = lane + 64 * q;
                                    mb[q] = pts[m < it.z ? m : last];
                                }
                                item_pass<false>(MatchRegs{mb}, it.z, lane, Fm, P.sampson_max, acc2, nv);
                                const float tot = item_totals(acc2, nv, it.z, P.sampson_max, lane, slot);
                                sum = c == 0 ? tot : sum + tot;
                            }
                        }
                        if (lane < 16 && slot < PD_ITEM_VALS) L.item[sl * PD_ITEM_VALS + slot] = sum;
                    }
                }
                __syncthreads();
                PD_PROF2H(q1);
                // ---- P3a: backward of this workgroup's pairs (thread per pair of the batch), rows 2 sl (side 0), 2 sl + 1 (side 1)
                if (tid < nb && L.itab[s0 + tid].y > 0) {
                    const int4 e = L.itab[s0 + tid];
                    const int pi = e.z, pj = e.w;
                    const int4 mp = make_int4(0, 0, 1, (2 * tid) | ((2 * tid + 1) << 16));
                    float G[9];
#pragma unroll
                    for (int c = 0; c < 9; ++c) G[c] = L.item[tid * PD_ITEM_VALS + c];
#include "pd_ggs_pairbwd.inc"
                }
                __syncthreads();
                PD_PROF2H(q2);
                // ---- hop 1: publish the (pair, side) rows; thread (row = tid / 16, component = tid % 16), 32 rows per pass
                for (int r0 = 0; r0 < 2 * nb; r0 += PD_GGS_THREADS / 16) {
                    const int row = r0 + (tid >> 4);
                    if (row < 2 * nb && L.itab[s0 + (row >> 1)].y > 0) {
                        u64 *g = xs + (size_t)grow[2 * s0 + row] * PD_XCHG_LINE + (tid & 15);
                        __hip_atomic_store(g, ((u64)epoch << 32) | (u64)__float_as_uint(own_rows[row * 16 + (tid & 15)]), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
                // this workgroup's loss totals {sum s valid, n valid, sum min(s, max)}: lane l takes slots l, l + 64, ... (n_batch % 64 == 0
                // whenever there are several batches)
                if (wave == PD_GGS_WAVES - 1) {
                    for (int sl = lane; sl < nb; sl += 64) {
                        if (L.itab[s0 + sl].y > 0) {
                            t0 += L.item[sl * PD_ITEM_VALS + 9];
                            t1 += L.item[sl * PD_ITEM_VALS + 10];
                            t2 += L.item[sl * PD_ITEM_VALS + 11];
                        }
                    }
                }
                // (the next batch's P1 writes L.F only, and its barrier stands before anything overwrites L.item or the own rows)
            }
            // ... -> its totals line
            if (wave == PD_GGS_WAVES - 1) {
                t0 = wave_allsum(t0);
                t1 = wave_allsum(t1);
                t2 = wave_allsum(t2);
                if (lane < 4) {
                    const float v = lane == 0 ? t0 : (lane == 1 ? t1 : (lane == 2 ? t2 : 0.0f));
                    __hip_atomic_store(xs + (size_t)(n_inc + wg) * PD_XCHG_LINE + lane, ((u64)epoch << 32) | (u64)__float_as_uint(v),
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            PD_PROF2H(q3);
#include "pd_ggs_long_hop2.inc"
#include "pd_ggs_p4_long.inc"
            __syncthreads();
            PD_PROF2H(q7);
            if (L.ctl[0] != 0.0f) break;
        }
        if (tid == 0 && wg == 0 && P.stats) {
            float *so = P.stats + ((size_t)b * P.n_stages + st) * 4;
            so[0] = last_print;
            so[1] = (float)stepped;
            so[2] = last_cnt;
            so[3] = last_loss;
        }
        if (P.eval_only) break;
    }
    if (prof2 && lane == 0) {
        long long *o = P.prof + (wg == 0 ? 0 : 8);
        o[0] = q0; o[1] = q1; o[2] = q2; o[3] = q3; o[4] = q4; o[5] = q5; o[6] = q6; o[7] = q7;
    }
#undef PD_PROF2H
    if (own && wg == 0 && !P.eval_only) {
#pragma unroll
        for (int c = 0; c < 9; ++c) xg[tid * 9 + c] = L.xst[tid * PD_XS_STRIDE + c];
    }
}

// Zeroes the exchange granules before every launch (tags restart at 1 per launch).  A KERNEL rather than
// hipMemsetAsync: under hipGraph replay with a second graph running concurrently, the memset NODE was observed
// not to be ordered against the neighbouring kernel nodes (stale tags of the previous launch were accepted ->
// silently wrong sums; tests/test_gpu_parity.py::test_two_engines_overlapped...); kernel -> kernel edges are.
__global__ void pd_ggs_zero_kernel(unsigned long long *p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = 0ull;
}
