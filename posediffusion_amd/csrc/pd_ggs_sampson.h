// pd_ggs_sampson.h -- the match pass of the GGS kernels: the Sampson residual + dL/dF of two matches at once (sampson_step2), of W such steps in
// lockstep (sampson_stepW) and of one match (sampson_step1); where a wave-per-item kernel's matches come from (MatchRegs / MatchLds), an item's
// steps, its fast and exact pass and its totals; the hand-issued LDS-DMA that stages items (pd_glds_item, pd_vmcnt).
// Textually part of pd_ggs.hip: that file's `#pragma clang fp contract(on)` stands ahead of this include (the step functions switch contraction off
// themselves and write every fused multiply-add out).
#pragma once
#include "pd_ggs_dev.h"

// F[k] as a two-match operand.  From nine scalars (the wave-per-item kernels: F is wave-uniform) or from five register PAIRS
// {F0,F1} {F2,F3} {F4,F5} {F6,F7} {F8,-} (the lane-per-item kernel: F is per lane; a half of a 64-bit pair feeds both halves of a
// packed instruction through op_sel, so the nine values cost 10 registers instead of 18 splatted ones)
struct PdFPairs {
    v2f p[5];
};
template <int K>
__device__ __forceinline__ v2f pd_fsplat(const float *F) { return pd_splat(F[K]); }
template <int K>
__device__ __forceinline__ v2f pd_fsplat(const PdFPairs &F) {
    return (K & 1) ? __builtin_shufflevector(F.p[K / 2], F.p[K / 2], 1, 1) : __builtin_shufflevector(F.p[K / 2], F.p[K / 2], 0, 0);
}

// Sampson residual + dL/dF of two matches (geometry_guided_sampling.py:157-170); acc[0..8] dL/dF sums,
// acc[9] sum(s valid), each as {match A, match B} partial sums.  Kept out of the per-match work (item_totals() finishes them per item):
//   * acc[0..8] accumulate HALF of dL/dF (ca, cb below without their factor 2 -- an exact scaling, doubled after the reduction);
//   * n_valid (slot 10) is counted on the scalar unit: popcounts of the two compare masks, wave-uniform and exact;
//   * sum(min(s, max)) (slot 11, the printed statistic :169) = sum(s valid) + max * (in-range matches - n_valid).
//
// Threshold rule (:170 `sampson < sampson_max` on torch's IEEE quotient top / bottom): EXACT = false computes the
// quotient as top * v_rcp_f32(bottom) (within 2 ulp of the IEEE quotient) and records in `mind` how close any in-range
// match came to the threshold; the caller re-runs the whole item with EXACT = true (IEEE divide for the quotient that
// is compared, clamped and summed) when some match of the wave lies within PD_SAMPSON_BAND_ULPS of sampson_max --
// outside that band both quotients decide alike, so the valid set is always the one the IEEE quotient gives.  The
// gradient scales 1/bottom keep the 1-ulp reciprocal in both variants (no threshold hangs on them).
#define PD_SAMPSON_BAND_ULPS 16.0f
// Every fused multiply-add below is written out and contraction is off inside the two step functions, so the packed and the
// single-match form perform the same roundings: an item's sums do not depend on which form ran its tail.
template <bool EXACT, typename FT>
__device__ __forceinline__ void sampson_step2(const v2f u1, const v2f v1, const v2f u2, const v2f v2, bool ina, bool inb, const FT &F, float smax,
                                              v2f (&acc)[PD_ITEM_VALS], float &mind, int &nv, unsigned long long lanes = ~0ull) {
#pragma clang fp contract(off)
    // left = x1^T F, right = F x2   (:158-159)
    const v2f l0 = pd_fma2(u1, pd_fsplat<0>(F), pd_fma2(v1, pd_fsplat<3>(F), pd_fsplat<6>(F)));
    const v2f l1 = pd_fma2(u1, pd_fsplat<1>(F), pd_fma2(v1, pd_fsplat<4>(F), pd_fsplat<7>(F)));
    const v2f l2 = pd_fma2(u1, pd_fsplat<2>(F), pd_fma2(v1, pd_fsplat<5>(F), pd_fsplat<8>(F)));
    const v2f r0 = pd_fma2(pd_fsplat<0>(F), u2, pd_fma2(pd_fsplat<1>(F), v2, pd_fsplat<2>(F)));
    const v2f r1 = pd_fma2(pd_fsplat<3>(F), u2, pd_fma2(pd_fsplat<4>(F), v2, pd_fsplat<5>(F)));
    const v2f ee = pd_fma2(l0, u2, pd_fma2(l1, v2, l2));
    const v2f bottom = pd_fma2(r1, r1, pd_fma2(r0, r0, pd_fma2(l1, l1, l0 * l0)));   // :161
    const v2f inv = {pd_rcp(bottom.x), pd_rcp(bottom.y)};
    const v2f top = ee * ee;
    v2f sam;                                                            // :162-164
    if (EXACT) {
        sam = (v2f){top.x / bottom.x, top.y / bottom.y};                // IEEE, as torch divides
    } else {
        sam = top * inv;
        const v2f d = sam - pd_splat(smax);
        // lanes past the item's end carry a clamped copy of its last match: harmless (same decision as that match)
        mind = fminf(mind, fminf(fabsf(d.x), fabsf(d.y)));              // one v_min3_f32 with |.| modifiers
    }
    const bool va = ina && (sam.x < smax), vb = inb && (sam.y < smax);   // :170 (false for NaN)
    // everything below is scaled by inv_v = valid ? 1/bottom : 0 (a select, not a product: 1/bottom may be inf),
    // so invalid / out-of-range matches contribute exact zeros without further masking
    const v2f inv_v = {va ? inv.x : 0.0f, vb ? inv.y : 0.0f};
    const v2f ca = ee * inv_v;                        // ee / bottom      (half of d sam / d ee)
    const v2f sam_v = EXACT ? (v2f){va ? sam.x : 0.0f, vb ? sam.y : 0.0f} : top * inv_v;   // = sam where valid, else 0
    const v2f cb = sam_v * inv_v;                     // sam / bottom     (half of -d sam / d bottom)
    acc[9] += sam_v;
    // (`lanes`: the lanes that count -- all of them in the wave-per-item kernels; the lane-per-item kernel's last wave has lanes without an item)
    nv += __builtin_popcountll(__builtin_amdgcn_ballot_w64(va) & lanes) + __builtin_popcountll(__builtin_amdgcn_ballot_w64(vb) & lanes);
    // (d sam / dF[r][c]) / 2 = x1[r] g_c - cb r_r x2[c] [r<2],  g_c = ca x2[c] - cb l_c [c<2]   (x1[2] = x2[2] = 1)
    const v2f g0 = pd_fma2(ca, u2, -(cb * l0)), g1 = pd_fma2(ca, v2, -(cb * l1));
    const v2f nbr0 = -(cb * r0), nbr1 = -(cb * r1);
    acc[0] = pd_fma2(nbr0, u2, pd_fma2(u1, g0, acc[0]));
    acc[1] = pd_fma2(nbr0, v2, pd_fma2(u1, g1, acc[1]));
    acc[2] = pd_fma2(u1, ca, acc[2]) + nbr0;
    acc[3] = pd_fma2(nbr1, u2, pd_fma2(v1, g0, acc[3]));
    acc[4] = pd_fma2(nbr1, v2, pd_fma2(v1, g1, acc[4]));
    acc[5] = pd_fma2(v1, ca, acc[5]) + nbr1;
    acc[6] += g0;
    acc[7] += g1;
    acc[8] += ca;
}

// W two-match steps at once, operation by operation (the lane-per-item kernel: one or two waves per SIMD cannot hide the VALU dependency
// latency of ONE step's serial chain l -> bottom -> 1/bottom -> sam -> valid -> ca, cb -> g -> sums; W independent chains issued in
// lockstep can).  Same operations as sampson_step2 on every match, and the sums take step 0's contribution first, then step 1's, ...:
// exactly what W successive sampson_step2 calls compute.
template <bool EXACT, int W, typename FT>
__device__ __forceinline__ void sampson_stepW(const v2f (&u1)[W], const v2f (&v1)[W], const v2f (&u2)[W], const v2f (&v2)[W], const bool (&ina)[W],
                                              const bool (&inb)[W], const FT &F, float smax, v2f (&acc)[PD_ITEM_VALS], float &mind, int &nv,
                                              unsigned long long lanes) {
#pragma clang fp contract(off)
    v2f l0[W], l1[W], l2[W], r0[W], r1[W], ee[W], bottom[W], inv[W], top[W], sam[W], inv_v[W], ca[W], sam_v[W], cb[W], g0[W], g1[W], nbr0[W], nbr1[W];
    bool va[W], vb[W];
#define PD_W for (int w = 0; w < W; ++w)
#pragma unroll
    PD_W l0[w] = pd_fma2(v1[w], pd_fsplat<3>(F), pd_fsplat<6>(F));
#pragma unroll
    PD_W l1[w] = pd_fma2(v1[w], pd_fsplat<4>(F), pd_fsplat<7>(F));
#pragma unroll
    PD_W l2[w] = pd_fma2(v1[w], pd_fsplat<5>(F), pd_fsplat<8>(F));
#pragma unroll
    PD_W r0[w] = pd_fma2(pd_fsplat<1>(F), v2[w], pd_fsplat<2>(F));
#pragma unroll
    PD_W r1[w] = pd_fma2(pd_fsplat<4>(F), v2[w], pd_fsplat<5>(F));
#pragma unroll
    PD_W l0[w] = pd_fma2(u1[w], pd_fsplat<0>(F), l0[w]);
#pragma unroll
    PD_W l1[w] = pd_fma2(u1[w], pd_fsplat<1>(F), l1[w]);
#pragma unroll
    PD_W l2[w] = pd_fma2(u1[w], pd_fsplat<2>(F), l2[w]);
#pragma unroll
    PD_W r0[w] = pd_fma2(pd_fsplat<0>(F), u2[w], r0[w]);
#pragma unroll
    PD_W r1[w] = pd_fma2(pd_fsplat<3>(F), u2[w], r1[w]);
#pragma unroll
    PD_W ee[w] = pd_fma2(l1[w], v2[w], l2[w]);
#pragma unroll
    PD_W bottom[w] = l0[w] * l0[w];
#pragma unroll
    PD_W ee[w] = pd_fma2(l0[w], u2[w], ee[w]);
#pragma unroll
    PD_W bottom[w] = pd_fma2(l1[w], l1[w], bottom[w]);
#pragma unroll
    PD_W bottom[w] = pd_fma2(r0[w], r0[w], bottom[w]);
#pragma unroll
    PD_W bottom[w] = pd_fma2(r1[w], r1[w], bottom[w]);                      // :161
#pragma unroll
    PD_W top[w] = ee[w] * ee[w];
#pragma unroll
    PD_W inv[w] = (v2f){pd_rcp(bottom[w].x), pd_rcp(bottom[w].y)};
    if (EXACT) {
#pragma unroll
        PD_W sam[w] = (v2f){top[w].x / bottom[w].x, top[w].y / bottom[w].y};   // IEEE, as torch divides   (:162-164)
    } else {
#pragma unroll
        PD_W sam[w] = top[w] * inv[w];
#pragma unroll
        PD_W {
            const v2f d = sam[w] - pd_splat(smax);
            mind = fminf(mind, fminf(fabsf(d.x), fabsf(d.y)));               // one v_min3_f32 with |.| modifiers
        }
    }
#pragma unroll
    PD_W {
        va[w] = ina[w] && (sam[w].x < smax);                                 // :170 (false for NaN)
        vb[w] = inb[w] && (sam[w].y < smax);
    }
#pragma unroll
    PD_W inv_v[w] = (v2f){va[w] ? inv[w].x : 0.0f, vb[w] ? inv[w].y : 0.0f};
#pragma unroll
    PD_W ca[w] = ee[w] * inv_v[w];
#pragma unroll
    PD_W sam_v[w] = EXACT ? (v2f){va[w] ? sam[w].x : 0.0f, vb[w] ? sam[w].y : 0.0f} : top[w] * inv_v[w];
#pragma unroll
    PD_W cb[w] = sam_v[w] * inv_v[w];
#pragma unroll
    PD_W nv += __builtin_popcountll(__builtin_amdgcn_ballot_w64(va[w]) & lanes) + __builtin_popcountll(__builtin_amdgcn_ballot_w64(vb[w]) & lanes);
#pragma unroll
    PD_W g0[w] = -(cb[w] * l0[w]);
#pragma unroll
    PD_W g1[w] = -(cb[w] * l1[w]);
#pragma unroll
    PD_W nbr0[w] = -(cb[w] * r0[w]);
#pragma unroll
    PD_W nbr1[w] = -(cb[w] * r1[w]);
#pragma unroll
    PD_W g0[w] = pd_fma2(ca[w], u2[w], g0[w]);
#pragma unroll
    PD_W g1[w] = pd_fma2(ca[w], v2[w], g1[w]);
#pragma unroll
    PD_W {                                                                   // the sums, step by step
        acc[9] += sam_v[w];
        acc[0] = pd_fma2(nbr0[w], u2[w], pd_fma2(u1[w], g0[w], acc[0]));
        acc[1] = pd_fma2(nbr0[w], v2[w], pd_fma2(u1[w], g1[w], acc[1]));
        acc[2] = pd_fma2(u1[w], ca[w], acc[2]) + nbr0[w];
        acc[3] = pd_fma2(nbr1[w], u2[w], pd_fma2(v1[w], g0[w], acc[3]));
        acc[4] = pd_fma2(nbr1[w], v2[w], pd_fma2(v1[w], g1[w], acc[4]));
        acc[5] = pd_fma2(v1[w], ca[w], acc[5]) + nbr1[w];
        acc[6] += g0[w];
        acc[7] += g1[w];
        acc[8] += ca[w];
    }
#undef PD_W
}

// The same for ONE match per lane on plain fp32 VALU (half the issue cycles of a packed step): the tail of an item whose
// last 128-match step would be at most half full (300 matches = 2 packed steps + 44: the third packed step ran 34 % full).
// It accumulates into the .x halves exactly what the packed step accumulates there when its .y match is masked off
// (+0 contributions), so an item's sums do not depend on which of the two forms ran its tail.
template <bool EXACT>
__device__ __forceinline__ void sampson_step1(const float4 pa, bool ina, const float *F, float smax, v2f (&acc)[PD_ITEM_VALS],
                                              float &mind, int &nv) {
#pragma clang fp contract(off)
    const float u1 = pa.x, v1 = pa.y, u2 = pa.z, v2 = pa.w;
    const float l0 = __builtin_fmaf(u1, F[0], __builtin_fmaf(v1, F[3], F[6]));
    const float l1 = __builtin_fmaf(u1, F[1], __builtin_fmaf(v1, F[4], F[7]));
    const float l2 = __builtin_fmaf(u1, F[2], __builtin_fmaf(v1, F[5], F[8]));
    const float r0 = __builtin_fmaf(F[0], u2, __builtin_fmaf(F[1], v2, F[2]));
    const float r1 = __builtin_fmaf(F[3], u2, __builtin_fmaf(F[4], v2, F[5]));
    const float ee = __builtin_fmaf(l0, u2, __builtin_fmaf(l1, v2, l2));
    const float bottom = __builtin_fmaf(r1, r1, __builtin_fmaf(r0, r0, __builtin_fmaf(l1, l1, l0 * l0)));
    const float inv = pd_rcp(bottom);
    const float top = ee * ee;
    float sam;
    if (EXACT) {
        sam = top / bottom;
    } else {
        sam = top * inv;
        mind = fminf(mind, fabsf(sam - smax));
    }
    const bool va = ina && (sam < smax);
    const float inv_v = va ? inv : 0.0f;
    const float ca = ee * inv_v;
    const float sam_v = EXACT ? (va ? sam : 0.0f) : top * inv_v;
    const float cb = sam_v * inv_v;
    acc[9].x += sam_v;
    nv += __builtin_popcountll(__builtin_amdgcn_ballot_w64(va));
    const float g0 = __builtin_fmaf(ca, u2, -(cb * l0)), g1 = __builtin_fmaf(ca, v2, -(cb * l1));
    const float nbr0 = -(cb * r0), nbr1 = -(cb * r1);
    acc[0].x = __builtin_fmaf(nbr0, u2, __builtin_fmaf(u1, g0, acc[0].x));
    acc[1].x = __builtin_fmaf(nbr0, v2, __builtin_fmaf(u1, g1, acc[1].x));
    acc[2].x = __builtin_fmaf(u1, ca, acc[2].x) + nbr0;
    acc[3].x = __builtin_fmaf(nbr1, u2, __builtin_fmaf(v1, g0, acc[3].x));
    acc[4].x = __builtin_fmaf(nbr1, v2, __builtin_fmaf(v1, g1, acc[4].x));
    acc[5].x = __builtin_fmaf(v1, ca, acc[5].x) + nbr1;
    acc[6].x += g0;
    acc[7].x += g1;
    acc[8].x += ca;
}

// where an item's matches come from: registers (resident / streamed through registers) or this wave's LDS staging buffer
// (lane-linear image written by LDS-DMA: match m at byte 16 m)
// Table layout (built at upload, host and device builders alike): inside an item every FULL group of 128 matches is stored
// pair-interleaved -- element lane of the group = (u1_A, u1_B, v1_A, v1_B), element 64 + lane = (u2_A, u2_B, v2_A, v2_B) with A = match
// lane, B = match 64 + lane of the group -- so a full packed step finds its four operand pairs in adjacent registers (8 register
// moves per step less; the pass is bound by VALU cycles).  The remainder of an item (< 128 matches) stays one float4 per match.
struct MatchRegs {
    const float4 (&M)[8];
    __device__ __forceinline__ float4 get(int j, int) const { return M[j]; }
    __device__ __forceinline__ void full_pairs(int j, v2f &u1, v2f &v1, v2f &u2, v2f &v2) const {
        const float4 q0 = M[2 * j], q1 = M[2 * j + 1];
        u1 = (v2f){q0.x, q0.y}; v1 = (v2f){q0.z, q0.w}; u2 = (v2f){q1.x, q1.y}; v2 = (v2f){q1.z, q1.w};
    }
};
struct MatchLds {
    const float4 *B;
    __device__ __forceinline__ float4 get(int j, int lane) const { return B[lane + 64 * j]; }
};


// the (<= 4) two-match steps of an item as straight-line code per step count: without the per-step branch the
// scheduler interleaves the independent steps, which hides the VALU dependency latency two waves per SIMD cannot
// (a FULL step lies wholly inside the item: its range masks are compile-time true and the selects they feed fold away)
#define PD_P2_FULL(j) do { v2f a_, b_, c_, d_; src.full_pairs(j, a_, b_, c_, d_); sampson_step2<EXACT>(a_, b_, c_, d_, true, true, Fm, smax, acc2, mind, nv); } while (0)
#define PD_P2_STEP(j) do { const float4 pa_ = src.get(2 * (j), lane), pb_ = src.get(2 * (j) + 1, lane);                                       \
        sampson_step2<EXACT>((v2f){pa_.x, pb_.x}, (v2f){pa_.y, pb_.y}, (v2f){pa_.z, pb_.z}, (v2f){pa_.w, pb_.w}, (lane + 128 * (j)) < cnt,   \
                             (lane + 128 * (j) + 64) < cnt, Fm, smax, acc2, mind, nv); } while (0)
#define PD_P2_TAIL(j)                                                                                           \
    do {                                                                                                        \
        if (rem > 64 || (!TAIL1 && rem > 0)) PD_P2_STEP(j);                                                     \
        else if (TAIL1 && rem > 0) sampson_step1<EXACT>(src.get(2 * (j), lane), (lane + 128 * (j)) < cnt, Fm, smax, acc2, mind, nv); \
    } while (0)
// TAIL1: run a tail of <= 64 matches as a single-match step (same sums; the variants that keep matches in registers leave it
// off -- they sit at the register limit and are latency-, not issue-bound)
template <bool EXACT, bool TAIL1, typename Src>
__device__ __forceinline__ void item_steps(const Src &src, int cnt, int lane, const float *Fm, float smax,
                                           v2f (&acc2)[PD_ITEM_VALS], float &mind, int &nv) {
    const int full = cnt >> 7, rem = cnt & 127;       // full packed steps; the rest: a packed step, a single-match step or nothing
    if (full >= 4) {
        PD_P2_FULL(0); PD_P2_FULL(1); PD_P2_FULL(2); PD_P2_FULL(3);
    } else if (full == 3) {
        PD_P2_FULL(0); PD_P2_FULL(1); PD_P2_FULL(2); PD_P2_TAIL(3);
    } else if (full == 2) {
        PD_P2_FULL(0); PD_P2_FULL(1); PD_P2_TAIL(2);
    } else if (full == 1) {
        PD_P2_FULL(0); PD_P2_TAIL(1);
    } else {
        PD_P2_TAIL(0);
    }
}
// one work item: the fast pass, and -- when some match of the wave came within the band of the threshold where the
// 1-ulp quotient could decide differently from the IEEE quotient -- the exact pass over the same data instead
template <bool TAIL1, typename Src>
__device__ __forceinline__ void item_pass(const Src &src, int cnt, int lane, const float *Fm, float smax,
                                          v2f (&acc2)[PD_ITEM_VALS], int &nv) {
    float mind = __int_as_float(0x7f800000);
    nv = 0;
#pragma unroll
    for (int c = 0; c < PD_ITEM_VALS; ++c) acc2[c] = (v2f){0.0f, 0.0f};
    item_steps<false, TAIL1>(src, cnt, lane, Fm, smax, acc2, mind, nv);
    const float band = smax * (PD_SAMPSON_BAND_ULPS * 1.1920929e-7f);
    if (__builtin_amdgcn_ballot_w64(mind <= band) != 0ull) {   // wave-uniform, rare (P ~ 1e-7 per match)
#pragma unroll
        for (int c = 0; c < PD_ITEM_VALS; ++c) acc2[c] = (v2f){0.0f, 0.0f};
        nv = 0;
        item_steps<true, false>(src, cnt, lane, Fm, smax, acc2, mind, nv);
    }
}
// fold the two-match partial sums, reduce across the wave: this lane then holds the item total of `slot` (n_valid: the scalar count)
__device__ __forceinline__ float item_totals(const v2f (&acc2)[PD_ITEM_VALS], int nv, int cnt, float smax, int lane, int &slot) {
    float acc[PD_ITEM_VALS];
#pragma unroll
    for (int c = 0; c < 10; ++c) acc[c] = acc2[c].x + acc2[c].y;
    acc[10] = acc[11] = 0.0f;                           // not reduced: finished from the scalar count below
    const float tot = wave_reduce12_transpose(acc, lane, slot);
    const float tot9 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tot), 6));   // lane 6 holds slot 9 (see the slot map)
    if (slot < 9) return tot + tot;                     // the factor 2 of ca, cb
    if (slot == 10) return (float)nv;
    if (slot == 11) return tot9 + smax * (float)(cnt - nv);   // every in-range match that is not valid contributes min(s, max) = max
    return tot;
}

// LDS-DMA (global_load_lds_dwordx4: 64 lanes x 16 B land lane-linear at the wave-uniform LDS byte address in M0) straight from
// global memory, no VGPR round trip.  Hand-issued: hipcc neither counts it (so nothing drains it at the next s_barrier and a
// prefetch can cross the serial phases of an iteration) nor waits for it -- every consumer waits with pd_vmcnt<> itself,
// and the kernel drains before it exits (an LDS-DMA landing after the workgroup's LDS was handed on would corrupt it).
// A whole staged item (P pieces of 1 KiB) in ONE statement: wave-uniform 64-bit base in SGPRs, a 32-bit byte offset per lane
// and piece, M0 stepped by 1 KiB between the pieces -- ~3 instructions per piece instead of ~12 (64-bit address arithmetic,
// M0 save / restore and readfirstlane per piece): the match pass is bound by how fast a wave ISSUES instructions.
template <int P>
__device__ __forceinline__ void pd_glds_item(const float4 *base, const unsigned (&off)[6], unsigned lds_dst) {
    static_assert(P == 3 || P == 5 || P == 6, "staging pieces");
    unsigned keep;
    lds_dst = __builtin_amdgcn_readfirstlane(lds_dst);
    if constexpr (P == 3)
        asm volatile("s_mov_b32 %[k], m0\n\ts_mov_b32 m0, %[d]\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %[o0], %[b]\n\ts_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %[o1], %[b]\n\ts_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %[o2], %[b]\n\ts_mov_b32 m0, %[k]"
                     : [k] "=&s"(keep) : [d] "s"(lds_dst), [b] "s"(base), [o0] "v"(off[0]), [o1] "v"(off[1]), [o2] "v"(off[2]) : "memory", "scc");
    else if constexpr (P == 5)
        asm volatile("s_mov_b32 %[k], m0\n\ts_mov_b32 m0, %[d]\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %[o0], %[b]\n\ts_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %[o1], %[b]\n\ts_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %[o2], %[b]\n\ts_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %[o3], %[b]\n\ts_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %[o4], %[b]\n\ts_mov_b32 m0, %[k]"
                     : [k] "=&s"(keep) : [d] "s"(lds_dst), [b] "s"(base), [o0] "v"(off[0]), [o1] "v"(off[1]), [o2] "v"(off[2]),
                       [o3] "v"(off[3]), [o4] "v"(off[4]) : "memory", "scc");
    else
        asm volatile("s_mov_b32 %[k], m0\n\ts_mov_b32 m0, %[d]\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %[o0], %[b]\n\ts_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %[o1], %[b]\n\ts_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %[o2], %[b]\n\ts_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %[o3], %[b]\n\ts_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %[o4], %[b]\n\ts_add_u32 m0, m0, 0x400\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %[o5], %[b]\n\ts_mov_b32 m0, %[k]"
                     : [k] "=&s"(keep) : [d] "s"(lds_dst), [b] "s"(base), [o0] "v"(off[0]), [o1] "v"(off[1]), [o2] "v"(off[2]),
                       [o3] "v"(off[3]), [o4] "v"(off[4]), [o5] "v"(off[5]) : "memory", "scc");
}
template <int N>
__device__ __forceinline__ void pd_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
