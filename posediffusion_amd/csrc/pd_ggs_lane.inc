// pd_ggs_lane.inc -- the lane-per-item GGS kernel (textually included by pd_ggs.hip after the helpers it shares with the other kernels:
// pd_ggs_dev.h, pd_ggs_sampson.h; its LDS image, carve_lane and lane_lds_bytes, is in pd_ggs_lds.h).
//
// Why another mapping (profiles/round3_valu_probe2.txt, round3_stream_probe.txt).  The wave-per-item kernel at one workgroup per
// sequence sits on two walls at once: (1) a gfx950 SIMD retires one packed-fp32 VALU instruction every ~2.0 ns whatever the number
// of resident waves (>= 2), and its 284 VALU instructions per 300-match item x 190 items are 86 % of that ceiling at the measured
// 22 ms per 256-sequence launch; (2) every CU re-reading a private 912 KB region gets 7.2 - 7.7 TB/s chip-wide from the Infinity
// Cache, and the launch moves exactly that.  Going faster needs FEWER INSTRUCTIONS and FEWER BYTES per iteration:
//   * a LANE owns a work item (<= l matches of one frame pair; how the pairs are cut into <= 512 items: pd_ggs_set_matches): the pair's F lives
//     in that lane's registers, the ten sums accumulate in the lane across its whole item, and there is no per-item prologue, no
//     64-lane reduction, no partly filled tail step: ~52 VALU instructions per two matches instead of ~121;
//   * the pair's F is computed by the lane itself (P1 merges into the match pass: one barrier less), the per-lane sums go to a
//     small LDS table and the pair backward sums a pair's items from there;
//   * the match table is laid out lane-major (a wave's step t = 2 x 1 KiB contiguous), and its first RV steps stay in REGISTERS for the whole
//     launch: only the rest is streamed, through a per-wave LDS ring fed by LDS-DMA (below).
// Arithmetic per match is sampson_step2 verbatim (same valid set, same fast / exact threshold rule); the order in which a pair's
// matches are summed differs from the wave-per-item kernels, so results agree to rounding, not bit for bit.
//
// One workgroup of 8 waves (<= 256 VGPRs each: two on every SIMD; waves w and w + 4 share one, which is why the items are ordered by length) per
// sequence and CU; needs <= PD_GGS_FAST_FRAMES (24) frames and <= 512 frame pairs (the serial phases are the fast ones of pd_ggs_kernel:
// pd_ggs_p3b.inc, pd_ggs_p4q.inc).

#ifndef PD_LANE_RV
#define PD_LANE_RV 14       // steps (two matches per lane each) of every lane item that stay in registers for the whole launch: the most that fit without a spill
                            //   (256 VGPRs; round 4 ran 12 -- 14 spilled 6 registers then; round 5 forms the P3b thread roles inside the iteration instead of holding
                            //   them across the match pass: 14 fit, 16 spill 13)
#endif
#ifndef PD_LANE_PAIRED
#define PD_LANE_PAIRED (PD_LANE_WAVES < 12)   // fewer than three waves per SIMD: run two steps in lockstep (sampson_stepW)
#endif
#ifndef PD_LANE_RING
#define PD_LANE_RING 3      // steps (2 KiB each) per wave in the LDS ring the rest of the stream is DMA'd through, in flight also ACROSS the serial phases
#endif                      //   (round 3's register ring let the stream stop there).  Round 4 ran 6; round 5 measured that 3 - 4 in flight sustain the stream
                            //   (2 do not: + 4 % at 256 sequences) and gave the other slots to RESIDENT steps (PD_LANE_RL)
#ifndef PD_LANE_RL
#define PD_LANE_RL 3        // steps RV .. RV + RL - 1 of every wave's stream that live in LDS for the whole launch (beside the ring: its depth is what the stream's
#endif                      //   latency needs, the rest of the LDS can HOLD matches; VERDICT round 4 item 4 b): 8 waves x (3 + 3) x 2 KiB = 96 KiB as before, 6.8 %
                            //   fewer streamed bytes, bitwise the same results; 256-sequence launch - 3.6 %, bench + 2.6 % (profiles/round5_lane_lds_resident.txt)
#define PD_LANE_SLOTS (PD_LANE_RING + PD_LANE_RL)     // 2 KiB slots per wave: the first RL resident, then the ring
#ifndef PD_LANE_ZIGZAG
#define PD_LANE_ZIGZAG 0    // round 6 (built, measured, OFF): the streamed steps are consumed forwards in one pass and BACKWARDS in the next, so what a pass touched last -- still in the
#endif                      //   XCD's L2 (4 MB per 32 CUs: ~ 64 steps of 2 KiB per CU) -- is what the next pass asks for first; the full-chip launch is bound by the
                            //   fabric behind the L2s (profiles/round6_zigzag_probe.txt: the ring pattern alone 6.6 -> 7.8 TB/s).  Every pass still sums every step
                            //   exactly once; the ORDER of a lane's sums alternates with the pass parity (deterministic: results stay bitwise reproducible and
                            //   independent of slot and launch shape, but differ in rounding from a forward-only build)

// the match stream is read through GLOBAL-address-space pointers (a pointer that came out of a descriptor in memory is generic to the
// compiler: flat loads, which count on the LDS counter too) with a wave-uniform base per step and the lane as a 32-bit offset
typedef float pd_f4v __attribute__((ext_vector_type(4)));
typedef const pd_f4v __attribute__((address_space(1))) *pd_gf4p;
__device__ __forceinline__ float4 pd_nt_load4(pd_gf4p p, unsigned lane) {
    const pd_f4v t = __builtin_nontemporal_load(p + lane);
    return make_float4(t.x, t.y, t.z, t.w);
}
__device__ __forceinline__ float4 pd_g_load4(pd_gf4p p, unsigned lane) {
    const pd_f4v t = p[lane];
    return make_float4(t.x, t.y, t.z, t.w);
}

// one two-match step of this lane's item: (q0, q1) = the two halves of step t; MASKED: the step may reach past the lane's item
#define PD_LANE_STEP(MASKED, q0, q1, t)                                                                                              \
    do {                                                                                                                             \
        const float4 a_ = (q0), b_ = (q1);                                                                                           \
        const v2f u1_ = {a_.x, a_.y}, v1_ = {a_.z, a_.w}, u2_ = {b_.x, b_.y}, v2_ = {b_.z, b_.w};                                     \
        if (MASKED) sampson_step2<EXACT>(u1_, v1_, u2_, v2_, 2 * (t) < cnt, 2 * (t) + 1 < cnt, Fp, smax, acc2, mind, nv, vmask);     \
        else sampson_step2<EXACT>(u1_, v1_, u2_, v2_, true, true, Fp, smax, acc2, mind, nv, vmask);                                  \
    } while (0)

// two steps at once, interleaved operation by operation (sampson_stepW): the same sums as two PD_LANE_STEPs, ta first
#define PD_LANE_STEP2(MASKED, qa0, qa1, ta, qb0, qb1, tb)                                                                            \
    do {                                                                                                                             \
        const float4 a_ = (qa0), b_ = (qa1), c_ = (qb0), d_ = (qb1);                                                                 \
        const v2f u1_[2] = {{a_.x, a_.y}, {c_.x, c_.y}}, v1_[2] = {{a_.z, a_.w}, {c_.z, c_.w}};                                      \
        const v2f u2_[2] = {{b_.x, b_.y}, {d_.x, d_.y}}, v2_[2] = {{b_.z, b_.w}, {d_.z, d_.w}};                                      \
        const bool ia_[2] = {!(MASKED) || 2 * (ta) < cnt, !(MASKED) || 2 * (tb) < cnt};                                              \
        const bool ib_[2] = {!(MASKED) || 2 * (ta) + 1 < cnt, !(MASKED) || 2 * (tb) + 1 < cnt};                                      \
        sampson_stepW<EXACT, 2>(u1_, v1_, u2_, v2_, ia_, ib_, Fp, smax, acc2, mind, nv, vmask);                                      \
    } while (0)

// ---- the streamed part of a wave's match stream: an LDS ring fed by LDS-DMA ---------------------------------------------------------
// The steps RV .. T-1 of a wave's lane-major stream (`n_s` of them, 2 KiB each, the same every iteration) go round a ring of PD_LANE_RING
// slots in LDS: global_load_lds_dwordx4 (two per step, hand-issued like pd_glds_item: the compiler neither drains nor waits for them)
// keeps PD_LANE_RING steps in flight per wave at ALL times -- a consumed slot is refilled at once with the step PD_LANE_RING further on
// in the PERIODIC sequence, so at the end of a pass the ring already receives the head of the next iteration's stream while the serial
// phases run.  n_s <= PD_LANE_RING: the steps are fetched once and stay (the "LDS-resident" case of round 3, with no code of its own).
struct LaneRing {
    const float4 *res;      // this lane's float4 in the first LDS-RESIDENT step, half 0 (PD_LANE_RL steps of 128 float4 each; generic LDS pointer)
    const float4 *src;      // wave-uniform: the wave's stream at its first STREAMED step
    unsigned lds0;          // wave-uniform LDS byte address of the wave's ring
    const float4 *rd;       // this lane's float4 in slot 0, half 0 (generic LDS pointer)
    int n_s;                // streamed steps per iteration
    int slot;               // ring slot of the oldest step in flight (= the next one consumed)
    int next;               // index (0 .. n_s - 1) of the step the next refill fetches
    int dir;                // +1 / -1: the direction `next` moves in (zigzag: it turns at both ends, fetching the turning step twice in a row)
    int fwd;                // the pass about to run consumes the streamed steps in ascending (1) or descending (0) order
};
// the refill pointer's successor in the fetch sequence 0, 1, .., n_s-1, n_s-1, .., 1, 0, 0, 1, .. (zigzag) or 0, 1, .., n_s-1, 0, .. (periodic)
__device__ __forceinline__ void lane_ring_advance(LaneRing &R) {
    if (PD_LANE_ZIGZAG) {
        if (R.next + R.dir < 0 || R.next + R.dir >= R.n_s) R.dir = -R.dir;
        else R.next += R.dir;
    } else {
        R.next = (R.next + 1 == R.n_s) ? 0 : R.next + 1;
    }
}
// slot <- streamed step `idx`
__device__ __forceinline__ void lane_ring_fetch(const LaneRing &R, int slot, int idx, unsigned lane16) {
    const unsigned off0 = (unsigned)idx * 2048u + lane16, off1 = off0 + 1024u;
    const unsigned dst = __builtin_amdgcn_readfirstlane(R.lds0 + (unsigned)slot * 2048u);
    unsigned keep;
    asm volatile("s_mov_b32 %[k], m0\n\ts_mov_b32 m0, %[d]\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %[o0], %[b]\n\ts_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %[o1], %[b]\n\ts_mov_b32 m0, %[k]"
                 : [k] "=&s"(keep) : [d] "s"(dst), [b] "s"(R.src), [o0] "v"(off0), [o1] "v"(off1) : "memory", "scc");
}
// one step (2 KiB at `src`, wave-uniform) -> the wave-uniform LDS byte address `dst` (the LDS-resident steps at launch)
__device__ __forceinline__ void lane_dma_step(const float4 *src, unsigned dst, unsigned lane16) {
    const unsigned off1 = lane16 + 1024u;
    dst = __builtin_amdgcn_readfirstlane(dst);
    unsigned keep;
    asm volatile("s_mov_b32 %[k], m0\n\ts_mov_b32 m0, %[d]\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %[o0], %[b]\n\ts_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %[o1], %[b]\n\ts_mov_b32 m0, %[k]"
                 : [k] "=&s"(keep) : [d] "s"(dst), [b] "s"(src), [o0] "v"(lane16), [o1] "v"(off1) : "memory", "scc");
}
// consume the oldest step: wait for it (at most `LEFT` DMA instructions of YOUNGER steps may still be in flight), read it out, refill its slot
template <int LEFT>
__device__ __forceinline__ void lane_ring_take(LaneRing &R, unsigned lane16, float4 &q0, float4 &q1, bool refill) {
    pd_vmcnt<LEFT>();
    const float4 *p = R.rd + R.slot * 128;
    q0 = p[0];
    q1 = p[64];
    if (refill) {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(q0.x), "+v"(q1.x) :: "memory");     // the slot is read out before the DMA may overwrite it
        lane_ring_fetch(R, R.slot, R.next, lane16);
        lane_ring_advance(R);
    }
    R.slot = (R.slot + 1 == PD_LANE_RING) ? 0 : R.slot + 1;
}

// the whole item of this lane: resident steps out of registers, the rest out of the ring, in step order
template <bool EXACT, int RV>
__device__ __forceinline__ void lane_pass(const float4 (&rv)[2 * RV], LaneRing &R, unsigned lane16, int T, int tfull, int cnt,
                                          unsigned long long vmask, const PdFPairs &Fp, float smax, v2f (&acc2)[PD_ITEM_VALS], float &mind, int &nv) {
    mind = __int_as_float(0x7f800000);
    nv = 0;
#pragma unroll
    for (int c = 0; c < PD_ITEM_VALS; ++c) acc2[c] = (v2f){0.0f, 0.0f};
    const bool full_res = !EXACT && tfull >= RV && T >= RV;      // the usual case: every register-resident step lies inside every lane's item
    static_assert(RV % 2 == 0, "register-resident steps are consumed in pairs");
    if (full_res) {
#pragma unroll
        for (int t = 0; t < RV; t += 2) {
            if (PD_LANE_PAIRED) {
                PD_LANE_STEP2(false, rv[2 * t], rv[2 * t + 1], t, rv[2 * t + 2], rv[2 * t + 3], t + 1);
            } else {
                PD_LANE_STEP(false, rv[2 * t], rv[2 * t + 1], t);
                PD_LANE_STEP(false, rv[2 * t + 2], rv[2 * t + 3], t + 1);
            }
        }
    } else {
#pragma unroll
        for (int t = 0; t < RV; ++t)
            if (t < T) PD_LANE_STEP(true, rv[2 * t], rv[2 * t + 1], t);
    }
    int t = RV;
    if constexpr (PD_LANE_RL > 0) {
        // steps RV .. RV + RL - 1 out of LDS, where they have been since the launch began: no wait, no refill; same order, same step functions
        const int t_res = min(RV + PD_LANE_RL, T);
        if (PD_LANE_PAIRED) {
            for (; t + 2 <= min(t_res, tfull); t += 2) {
                const float4 *p = R.res + (t - RV) * 128;
                PD_LANE_STEP2(false, p[0], p[64], t, p[128], p[192], t + 1);
            }
        }
        for (; t < t_res; ++t) {
            const float4 *p = R.res + (t - RV) * 128;
            PD_LANE_STEP(true, p[0], p[64], t);
        }
    }
    // streamed steps RV + RL .. T-1, ascending or (zigzag, every other pass) descending: two at a time -- unmasked while both lie inside every item
    // of the wave, else masked per lane (a wave that mixes item lengths: uneven pair sizes, or the boundary between the long and the short items of
    // the cut rule; the same sums in the same order as single steps, which ran at the unpaired issue rate: 37.7 k cycles per pass against 34.0 k) --,
    // then the odd one.  With n_s <= PD_LANE_RING nothing is refilled (the ring holds the whole tail for the launch, slot = step, always ascending).
    const bool refill = R.n_s > PD_LANE_RING;
    if (!refill) R.slot = 0;                          // (the tail sits in slots 0 .. n_s - 1 for the whole launch)
    const int S0 = t, n = T - t;                                     // this pass's streamed steps S0 .. T-1
    const int d = (PD_LANE_ZIGZAG && refill && !R.fwd) ? -1 : 1;
    if (d < 0) t = T - 1;
    int done = 0;
    if (PD_LANE_PAIRED && n >= 2) {
        // pairs in stream order; a pair is masked iff its higher step >= tfull.  Ascending: unmasked pairs, then masked ones; descending: masked, then
        // unmasked -- three segments {masked, unmasked, masked} of which the first or the last is empty
        const int tf = min(max(tfull, S0), T), np = n >> 1;
        const int nu_up = (tf - S0) >> 1;                               // ascending: pairs (S0 + 2 k, S0 + 2 k + 1) with S0 + 2 k + 1 < tf
        const int nm_dn = min(np, T - 1 >= tf ? ((T - 1 - tf) >> 1) + 1 : 0);   // descending: pairs (T - 1 - 2 k, T - 2 - 2 k) with T - 1 - 2 k >= tf
        const int seg0 = d > 0 ? 0 : nm_dn, seg1 = d > 0 ? nu_up : np - nm_dn, seg2 = d > 0 ? np - nu_up : 0;
        // (three loops one after the other: a loop over the segments that picks a body costs 20 spilled registers)
        for (int k = 0; k < seg0; ++k, t += 2 * d) {
            float4 a0, a1, b0, b1;
            lane_ring_take<2 * PD_LANE_RING - 2>(R, lane16, a0, a1, refill);     // (the oldest step: 2 of the <= 2 RING instructions in flight)
            lane_ring_take<2 * PD_LANE_RING - 2>(R, lane16, b0, b1, refill);
            PD_LANE_STEP2(true, a0, a1, t, b0, b1, t + d);
        }
        for (int k = 0; k < seg1; ++k, t += 2 * d) {
            float4 a0, a1, b0, b1;
            lane_ring_take<2 * PD_LANE_RING - 2>(R, lane16, a0, a1, refill);
            lane_ring_take<2 * PD_LANE_RING - 2>(R, lane16, b0, b1, refill);
            PD_LANE_STEP2(false, a0, a1, t, b0, b1, t + d);
        }
        for (int k = 0; k < seg2; ++k, t += 2 * d) {
            float4 a0, a1, b0, b1;
            lane_ring_take<2 * PD_LANE_RING - 2>(R, lane16, a0, a1, refill);
            lane_ring_take<2 * PD_LANE_RING - 2>(R, lane16, b0, b1, refill);
            PD_LANE_STEP2(true, a0, a1, t, b0, b1, t + d);
        }
        done = 2 * np;
    }
    for (; done < n; ++done, t += d) {
        float4 a0, a1;
        lane_ring_take<2 * PD_LANE_RING - 2>(R, lane16, a0, a1, refill);
        PD_LANE_STEP(true, a0, a1, t);
    }
    if (PD_LANE_ZIGZAG && refill) R.fwd ^= 1;
}

template <int RV>
__global__ __launch_bounds__(PD_LANE_THREADS, PD_LANE_WAVES / 4) void pd_ggs_lane_kernel(PdGgsParams P, int pinc_rows) {
    constexpr int NT = PD_LANE_THREADS;
    constexpr int wg = 0;                               // one workgroup per sequence
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform to the compiler too: everything derived from it stays scalar
    const int b = blockIdx.x;
    const PdSeqDesc D = P.seqs[b];
    const int N = D.n_frames;                           // this sequence's own frame count (see pd_ggs_kernel); rows of x stay P.N apart
    const Lds L = carve_lane(smem, pinc_rows);
    if (tid == 0) {
        // launch stamps (PdGgsParams::stamp): workgroup 0's start now; the pointer waits in two spare words of L.psum for the end of the kernel
        // (held in registers across the launch it costs a spilled VGPR: the kernel sits at 256)
        if (P.stamp && b == 0) P.stamp[0] = wall_clock64();      // (the launch's workgroups start within < 1 us of each other)
        ((unsigned *)L.psum)[14] = (unsigned)(size_t)P.stamp;                       // (two 32-bit words: no alignment asked of L.psum)
        ((unsigned *)L.psum)[15] = (unsigned)((size_t)P.stamp >> 32);
    }
    float *xg = P.x + (size_t)b * P.N * PD_POSE_DIM;
    const float smax = P.sampson_max;

    const bool own = (wave == 0 && lane < N);
    if (wave == 0) {
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            L.xst[lane * PD_XS_STRIDE + c] = own ? xg[lane * 9 + c] : 0.0f;
            L.mst[lane * PD_XS_STRIDE + c] = 0.0f;
        }
    }
    for (int q = tid; q <= N; q += NT) L.incoff[q] = D.n_pchunks > 0 ? D.pchunk_off[q] : 0;
    if (tid == 0) {
        L.ctl[0] = 0.0f;
        L.ctl[1] = 0.0f;
    }
    if (wave == 0) {
        float xr0[9];
        params_load(L.xst, lane, xr0);
        decode_all(L, xr0, lane, N, D);
    }
    // this lane's item, this wave's stream
    const bool has_item = tid < D.n_litems;
    const int4 li = has_item ? D.litems[tid] : make_int4(0, 0, 0, 0);   // (i | j << 8, count, pair, first match)
    const int pi = li.x & 0xff, pj = li.x >> 8, cnt = li.y;
    int wbase = 0, T = 0;
    if (wave < D.n_lwaves) {
        const int2 lw = D.lwave[wave];
        wbase = __builtin_amdgcn_readfirstlane(lw.x);
        T = __builtin_amdgcn_readfirstlane(lw.y);
    }
    // lanes without an item (the tail of the last wave) run along on padding and are kept out of every result: `vmask` masks the
    // valid counts and the threshold-band vote, their sums are never stored
    const unsigned long long vmask = __builtin_amdgcn_ballot_w64(has_item);
    int tf = has_item ? (cnt >> 1) : 0x7fffffff;        // steps in which both matches of EVERY item of the wave are in range
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) tf = min(tf, __shfl_xor(tf, d, 64));
    const int tfull = vmask ? __builtin_amdgcn_readfirstlane(tf) : 0;
    pd_gf4p sw = (pd_gf4p)D.lstream + wbase;            // wave-uniform; a wave without items re-reads the stream's head (never used)
    float4 rv[2 * RV];
#pragma unroll
    for (int t = 0; t < RV; ++t) {
        const int tt = max(min(t, T - 1), 0);
        rv[2 * t] = pd_g_load4(sw + (size_t)tt * 128, lane);
        rv[2 * t + 1] = pd_g_load4(sw + (size_t)tt * 128 + 64, lane);
    }
    // the rest of the stream: the wave's LDS ring, its first PD_LANE_RING (or all n_s) steps on their way
    LaneRing R;
    R.n_s = max(T - RV - PD_LANE_RL, 0);
    R.src = (const float4 *)D.lstream + wbase + (size_t)(RV + PD_LANE_RL) * 128;
    float *wave_lds = L.stage + wave * (PD_LANE_SLOTS * 512);                       // this wave's slots: [RL resident | RING]
    R.res = (const float4 *)wave_lds + lane;
    R.lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(wave_lds + PD_LANE_RL * 512));
    R.rd = (const float4 *)(wave_lds + PD_LANE_RL * 512) + lane;
    R.slot = 0;
    const unsigned lane16 = (unsigned)lane * 16u;
    {
        if constexpr (PD_LANE_RL > 0) {
            const int nr = max(min(T - RV, PD_LANE_RL), 0);
            for (int u = 0; u < nr; ++u)
                lane_dma_step((const float4 *)D.lstream + wbase + (size_t)(RV + u) * 128, (unsigned)(size_t)(wave_lds + u * 512), lane16);
        }
        const int n0 = min(R.n_s, PD_LANE_RING);
        R.next = 0;
        R.dir = 1;
        R.fwd = 1;
        for (int u = 0; u < n0; ++u) {
            lane_ring_fetch(R, u, u, lane16);
            if (R.n_s > PD_LANE_RING) lane_ring_advance(R);      // (a tail that fits the ring is fetched once: no refill pointer)
        }
        if (PD_LANE_RL > 0 || R.n_s <= PD_LANE_RING) pd_vmcnt<0>();   // resident steps (and a tail that stays in the ring) have landed before the first pass reads them
    }
    __syncthreads();

    // the serial phases' geometry (pd_ggs_kernel's fast path: rows at a fixed, bank-conflict-free stride per frame; pd_ggs_plan made the room)
    int cap = 0;
    for (int n = 0; n < N; ++n) cap = max(cap, L.incoff[n + 1] - L.incoff[n]);
    cap = (cap + 3) & ~3;
    const int rstride = cap + 1, n_row_waves = (N * 16 + 63) >> 6, ga_parts = n_row_waves;
    const bool p3a = tid < D.n_pairs;
    int4 my_pair = p3a ? D.ptab[tid] : make_int4(0, 0, 0, 0);
    if (p3a) {
        const int fi = my_pair.x & 0xff, fj = my_pair.x >> 8;
        my_pair.w = (fi * rstride + ((my_pair.w & 0xffff) - L.incoff[fi])) | ((fj * rstride + ((my_pair.w >> 16) - L.incoff[fj])) << 16);
    }
    for (int q = tid; q < N * rstride * 4; q += NT) ((float4 *)L.pinc)[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (wave == PD_LANE_WAVES - 1) jac_all(L, lane, N);
    const int2 my_lp = p3a ? D.lptab[tid] : make_int2(0, 0);
    int trace_row = 0;
    const float inv_M = 1.0f / (float)D.M;
    // phase clocks of one wave of workgroup 0 (pd_debug_ggs_prof): {match pass, wait for the other waves, P3a + P3b, P4, -, iterations}
    const bool prof = P.prof != nullptr && b == 0 && wave == (P.prof_wave & 7);
    long long pt0 = 0, pt1 = 0, pt2 = 0, pt3 = 0, pit = 0, pc = 0;
#define PD_LPROF(acc) do { if (prof) { const long long n_ = __builtin_amdgcn_s_memtime(); acc += n_ - pc; pc = n_; } } while (0)
    for (int st = 0; st < P.n_stages; ++st) {
        const PdGgsStage S = P.stages[st];
        int stepped = 0;
        if (tid == 0) {                                   // {printed statistic, valid count, loss} of the stage's last iteration (written by P4's lane 0)
            L.ctl[5] = __int_as_float(0x7fc00000);
            L.ctl[6] = 0.0f;
            L.ctl[7] = __int_as_float(0x7fc00000);
        }
        const bool need_rt = S.update_R || S.update_T;
        for (int it = 0; it < S.iters; ++it) {
            if (prof) pc = __builtin_amdgcn_s_memtime();
            const Cam cam = {L.cam[0], L.cam[1], L.cam[2], L.cam[3]};
            // ---- P1 + P2: this lane's F, then its whole item ------------------------------------------------------------
            {
                PdFPairs Fp;
                {
                    float Fm[9];
                    float Ri[9], Rj[9], ti[3], tj[3];
                    frame_load(L, pi, Ri, ti);
                    frame_load(L, pj, Rj, tj);
                    PairFwd f;
                    pair_forward(Ri, ti, Rj, tj, f);
                    fundamental_from_E(f.E, cam, Fm);
#pragma unroll
                    for (int c = 0; c < 4; ++c) Fp.p[c] = (v2f){Fm[2 * c], Fm[2 * c + 1]};
                    Fp.p[4] = (v2f){Fm[8], 0.0f};
                }
                v2f acc2[PD_ITEM_VALS];
                float mind;
                int nv;
                lane_pass<false, RV>(rv, R, lane16, T, tfull, cnt, vmask, Fp, smax, acc2, mind, nv);
                const float band = smax * (PD_SAMPSON_BAND_ULPS * 1.1920929e-7f);
                // wave-uniform, rare: the IEEE quotient decides (see sampson_step2).  The ring is periodic -- after a pass it holds the head of the
                // stream again, exactly as before the pass --, so the item is simply run once more.
                if ((__builtin_amdgcn_ballot_w64(mind <= band) & vmask) != 0ull)
                    lane_pass<true, RV>(rv, R, lane16, T, tfull, cnt, vmask, Fp, smax, acc2, mind, nv);
                if (has_item) {
#pragma unroll
                    for (int c = 0; c < 9; ++c) {
                        const float h = acc2[c].x + acc2[c].y;
                        L.item[tid * PD_LANE_ITEM_VALS + c] = h + h;                  // the factor 2 of ca, cb
                    }
                    L.item[tid * PD_LANE_ITEM_VALS + 9] = acc2[9].x + acc2[9].y;
                }
                if (lane == 0) L.psum[wave] = (float)nv;
            }
            // the quaternion Jacobian of the parameters this iteration runs on (first read behind two barriers): on the LAST wave -- the items are
            // ordered by length, so it is the shortest and, as the younger wave of its SIMD, done well before the pass ends (round 6: with the
            // [75 x 4, 38 x 4] cuts wave 3 is a long wave, and the ~ 4 k cycles of jac_all on it were what made those cuts look slower in round 5)
            if (wave == PD_LANE_WAVES - 1 && S.update_R) jac_all(L, lane, N);
            PD_LPROF(pt0);
            __syncthreads();
            PD_LPROF(pt1);

            // ---- P3a: pair backward, one thread per frame pair (sums its lane items in item order) ------------------------
            if (p3a) {
                const int4 mp = my_pair;
                const int pi = mp.x & 0xff, pj = mp.x >> 8;
                float G[9];
#pragma unroll
                for (int c = 0; c < 9; ++c) G[c] = 0.0f;
                for (int u = 0; u < my_lp.y; ++u)
#pragma unroll
                    for (int c = 0; c < 9; ++c) G[c] += L.item[(my_lp.x + u) * PD_LANE_ITEM_VALS + c];
#include "pd_ggs_pairbwd.inc"
            }
            if (wave == PD_LANE_WAVES - 1) {              // totals (after this wave's share of the pairs, if any)
                float s_sum = 0.0f;
                for (int q2 = lane; q2 < D.n_litems; q2 += 64) s_sum += L.item[q2 * PD_LANE_ITEM_VALS + 9];
                s_sum = wave_allsum(s_sum);
                const float s_cnt = wave_allsum(lane < PD_LANE_WAVES ? L.psum[lane] : 0.0f);
                if (lane == 0) {
                    L.cam[6] = s_sum;
                    L.cam[7] = s_cnt;
                    L.ctl[2] = s_sum + smax * ((float)D.M - s_cnt);   // sum(min(s, max)): every match that is not valid contributes max
                }
            }
            __syncthreads();
            // ---- P3b: per-frame sums, dL/dq and the dL/dA partials (the fast form of pd_ggs_kernel) ------------------------------------
            {
                int tid_b = tid;
                asm volatile("" : "+v"(tid_b));           // P3b role: thread (frame, component), formed here in every iteration: three registers less held across the match pass
                const int fb_n = tid_b >> 4, fb_c = tid_b & 15;
                const float fb_sign = (fb_c < 9) ? (fb_c < 6 ? -1.0f : 1.0f) : ((fb_c < 11) ? -1.0f : 1.0f);
#include "pd_ggs_p3b.inc"
            }
            __syncthreads();
            PD_LPROF(pt2);

#include "pd_ggs_p4q.inc"
            __syncthreads();
            PD_LPROF(pt3);
            pit += 1;
            if (L.ctl[0] != 0.0f) break;
        }
        if (wave == 0 && lane == 0 && P.stats) {
            float *so = P.stats + ((size_t)b * P.n_stages + st) * 4;
            so[0] = L.ctl[5];
            so[1] = (float)stepped;
            so[2] = L.ctl[6];
            so[3] = L.ctl[7];
        }
        if (P.eval_only) break;
    }
    if (prof && lane == 0) {
        P.prof[0] = 0;
        P.prof[1] = pt0;
        P.prof[2] = pt1;
        P.prof[3] = pt2;
        P.prof[4] = pt3;
        P.prof[5] = pit;
    }
    if (own && !P.eval_only) {
#pragma unroll
        for (int c = 0; c < 9; ++c) xg[lane * 9 + c] = L.xst[lane * PD_XS_STRIDE + c];
    }
    pd_vmcnt<0>();      // the ring's DMA must land before the workgroup's LDS is handed on
    if (tid == 0) {
        unsigned long long *stamp = (unsigned long long *)((size_t)((unsigned *)L.psum)[14] | ((size_t)((unsigned *)L.psum)[15] << 32));
        if (stamp) atomicMax(stamp + 1, (unsigned long long)wall_clock64());
    }
}
#undef PD_LANE_STEP
#undef PD_LANE_STEP2
#undef PD_LPROF
