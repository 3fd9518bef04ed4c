// pd_ggs_dev.h -- device helpers shared by the three GGS kernels (pd_ggs_kernels.h, pd_ggs_lane.inc): cross-lane sums on the DPP / permlane
// network, the 1-ulp reciprocal and square root, packed-fp32 operands, the forward of one frame pair (essential and fundamental matrix), the
// per-frame tables in LDS, pose decode and the quaternion Jacobian.
// Textually part of pd_ggs.hip: that file's `#pragma clang fp contract(on)` stands ahead of this include and governs the arithmetic below.
#pragma once
#include "pd_ggs_lds.h"

typedef unsigned long long u64;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
#define PD_XCHG_LINE 16   // granules per item record in the exchange buffer (one 128-byte line)

// 64-lane sum on the DPP cross-lane network (no LDS round trips): xor-1, xor-2 quad permutes,
// half-row and row mirrors give every lane its 16-lane row sum; row_bcast15/31 chain the four rows;
// lane 63 holds the total, read back into an SGPR.  Fixed tree -> bitwise reproducible, and the
// result is wave-uniform by construction.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float v) {
    const int moved = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, false);
    return v + __int_as_float(moved);
}
__device__ __forceinline__ float wave_allsum(float v) {
    v = dpp_add<0xB1, 0xf>(v);    // quad_perm [1,0,3,2]
    v = dpp_add<0x4E, 0xf>(v);    // quad_perm [2,3,0,1]
    v = dpp_add<0x141, 0xf>(v);   // row_half_mirror
    v = dpp_add<0x140, 0xf>(v);   // row_mirror
    v = dpp_add<0x142, 0xa>(v);   // row_bcast:15 -> rows 1, 3
    v = dpp_add<0x143, 0xc>(v);   // row_bcast:31 -> rows 2, 3
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// 1-ulp hardware reciprocal / sqrt for scale factors on the serial per-iteration chain and for the gradient scales
// of the match pass.  The hard `sampson < sampson_max` test (geometry_guided_sampling.py:170) is decided on the IEEE
// quotient top / bottom like torch's: see sampson_step2 (fast pass + exact re-run of an item that has a match inside
// the band where the 1-ulp quotient could decide differently).
__device__ __forceinline__ float pd_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float pd_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }

// Transposing butterfly over the per-item sums (slots 0..9 carry values; 10..15 are padding): at every step a lane KEEPS half
// of its values and SENDS the other half to the partner that differs in exactly ONE lane bit (who keeps exactly those), so the
// live values go 16 -> 8 -> 4 -> 2 -> 1 per lane.  Lane bits 2 and 3 go first: they select a DPP bank (4 lanes), so a row shift
// with a bank mask adds the partner's value AND picks which of the two values a lane keeps in one v_add_f32_dpp -- no selects
// (hand-written: hipcc only emits the masked form as v_mov_b32_dpp pairs + selects).  Then bits 0 / 1 as quad permutes with
// selects, bits 4 / 5 as permlane swaps.  ~45 instructions per item instead of 10 full 64-lane reductions.  Value `slot`
// ends up in every lane whose low four bits encode that slot.  Fixed tree -> bitwise reproducible; every lane must be active.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// Partner exchanges of the butterfly, all on the VALU cross-lane paths (no LDS crossbar round trips: ds_swizzle / ds_bpermute
// cost ~100+ cycles each on a chain that runs once per work item):
//   lane ^ 4, lane ^ 8   two DPP row shifts each (up for the lanes whose bit is clear, down for the others, picked by bank_mask)
//   lane ^ 16, lane ^ 32 gfx950's v_permlane16_swap / v_permlane32_swap: swapping the odd rows (upper half) of one copy with
//                        the even rows (lower half) of another leaves {x[lane & ~b], x[lane | b]} in the two copies
__device__ __forceinline__ float add_xor16(float v) {    // v[lane] + v[lane ^ 16]
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_int(v), __float_as_int(v), false, false);
    return __int_as_float(r[0]) + __int_as_float(r[1]);
}
__device__ __forceinline__ float add_xor32(float v) {    // v[lane] + v[lane ^ 32]
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_int(v), __float_as_int(v), false, false);
    return __int_as_float(r[0]) + __int_as_float(r[1]);
}
__device__ __forceinline__ float wave_reduce12_transpose(const float (&a)[PD_ITEM_VALS], int lane, int &slot) {
    const bool b0 = lane & 1, b1 = lane & 2;
    float w0, w1, w2, w3, w4, w5, w6, w7;
    // lane ^ 4: banks 0, 2 (bit 2 clear) keep slot j = a[j] + a[j] of lane + 4; banks 1, 3 keep slot j + 8 (only 8 and 9 exist; the
    // other lanes of w2..w7 stay undefined -- they would hold the padding slots, which nobody reads).  The leading s_nop covers
    // the VALU-write -> DPP-read hazard the assembler cannot see for us.
    asm volatile("s_nop 1\n\t"
                 "v_add_f32_dpp %0, %8, %8 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
                 "v_add_f32_dpp %1, %9, %9 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
                 "v_add_f32_dpp %2, %10, %10 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
                 "v_add_f32_dpp %3, %11, %11 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
                 "v_add_f32_dpp %4, %12, %12 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
                 "v_add_f32_dpp %5, %13, %13 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
                 "v_add_f32_dpp %6, %14, %14 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
                 "v_add_f32_dpp %7, %15, %15 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
                 "v_add_f32_dpp %0, %16, %16 row_shr:4 row_mask:0xf bank_mask:0xa\n\t"
                 "v_add_f32_dpp %1, %17, %17 row_shr:4 row_mask:0xf bank_mask:0xa"
                 : "=&v"(w0), "=&v"(w1), "=&v"(w2), "=&v"(w3), "=&v"(w4), "=&v"(w5), "=&v"(w6), "=&v"(w7)
                 : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "v"(a[4]), "v"(a[5]), "v"(a[6]), "v"(a[7]), "v"(a[8]), "v"(a[9]));
    // lane ^ 8: banks 0, 1 (bit 3 clear) keep w[j], banks 2, 3 keep w[j + 4]
    float q0, q1, q2, q3;
    asm volatile("s_nop 1\n\t"
                 "v_add_f32_dpp %0, %4, %4 row_shl:8 row_mask:0xf bank_mask:0x3\n\t"
                 "v_add_f32_dpp %1, %5, %5 row_shl:8 row_mask:0xf bank_mask:0x3\n\t"
                 "v_add_f32_dpp %2, %6, %6 row_shl:8 row_mask:0xf bank_mask:0x3\n\t"
                 "v_add_f32_dpp %3, %7, %7 row_shl:8 row_mask:0xf bank_mask:0x3\n\t"
                 "v_add_f32_dpp %0, %8, %8 row_shr:8 row_mask:0xf bank_mask:0xc\n\t"
                 "v_add_f32_dpp %1, %9, %9 row_shr:8 row_mask:0xf bank_mask:0xc\n\t"
                 "v_add_f32_dpp %2, %10, %10 row_shr:8 row_mask:0xf bank_mask:0xc\n\t"
                 "v_add_f32_dpp %3, %11, %11 row_shr:8 row_mask:0xf bank_mask:0xc"
                 : "=&v"(q0), "=&v"(q1), "=&v"(q2), "=&v"(q3)
                 : "v"(w0), "v"(w1), "v"(w2), "v"(w3), "v"(w4), "v"(w5), "v"(w6), "v"(w7));
    const float p0 = (b0 ? q2 : q0) + dpp_mov<0xB1>(b0 ? q0 : q2);     // lane ^ 1
    const float p1 = (b0 ? q3 : q1) + dpp_mov<0xB1>(b0 ? q1 : q3);
    float v = (b1 ? p1 : p0) + dpp_mov<0x4E>(b1 ? p0 : p1);            // lane ^ 2
    v = add_xor16(v);
    v = add_xor32(v);
    slot = ((lane & 4) ? 8 : 0) + ((lane & 8) ? 4 : 0) + (b0 ? 2 : 0) + (b1 ? 1 : 0);
    return v;
}

// two 64-lane sums for little more than the price of one: v_permlane32_swap folds a's upper half onto its lower half and b's lower
// half onto its upper half (one swap + one add), then ONE five-step DPP chain sums both 32-lane halves; a in lane 31, b in lane 63.
__device__ __forceinline__ void wave_allsum2(float a, float b, float &sa, float &sb) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_int(a), __float_as_int(b), false, false);
    float v = __int_as_float(r[0]) + __int_as_float(r[1]);   // lanes < 32: a[l] + a[l + 32]; lanes >= 32: b[l - 32] + b[l]
    v = dpp_add<0xB1, 0xf>(v);    // quad_perm [1,0,3,2]
    v = dpp_add<0x4E, 0xf>(v);    // quad_perm [2,3,0,1]
    v = dpp_add<0x141, 0xf>(v);   // row_half_mirror
    v = dpp_add<0x140, 0xf>(v);   // row_mirror
    v = dpp_add<0x142, 0xa>(v);   // row_bcast:15 -> rows 1, 3
    sa = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 31));
    sb = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

struct Cam {   // shared intrinsics of the step: A = K^-1 = [[a0,0,c0],[0,a1,c1],[0,0,1]]
    float a0, a1, c0, c1;
};

// forward of get_essential_matrix for one ordered pair (camera 1 = i, camera 2 = j)
// (get_fundamental_matrix.py:45-51), keeping the intermediates the backward needs.
struct PairFwd {
    float R12[9], t12[3], Et[3], E[9];
};

__device__ __forceinline__ void pair_forward(const float *Ri, const float *ti, const float *Rj, const float *tj,
                                             PairFwd &o) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            o.R12[a * 3 + c] = Rj[a * 3 + 0] * Ri[c * 3 + 0] + Rj[a * 3 + 1] * Ri[c * 3 + 1] + Rj[a * 3 + 2] * Ri[c * 3 + 2];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        o.t12[a] = tj[a] - (o.R12[a * 3 + 0] * ti[0] + o.R12[a * 3 + 1] * ti[1] + o.R12[a * 3 + 2] * ti[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a)
        o.Et[a] = -(o.R12[0 * 3 + a] * o.t12[0] + o.R12[1 * 3 + a] * o.t12[1] + o.R12[2 * 3 + a] * o.t12[2]);
    const float ex = o.Et[0], ey = o.Et[1], ez = o.Et[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) {   // E = R12 * hat(Et), hat = [[0,-z,y],[z,0,-x],[-y,x,0]]
        o.E[a * 3 + 0] = o.R12[a * 3 + 1] * ez - o.R12[a * 3 + 2] * ey;
        o.E[a * 3 + 1] = o.R12[a * 3 + 2] * ex - o.R12[a * 3 + 0] * ez;
        o.E[a * 3 + 2] = o.R12[a * 3 + 0] * ey - o.R12[a * 3 + 1] * ex;
    }
}

// F as used by _sampson_distance after the permute of geometry_guided_sampling.py:155:
// F = (K2^-T E K1^-1)^T = (A^T E A)^T   (get_fundamental_matrix.py:41; K1 = K2, focal is the mean)
__device__ __forceinline__ void fundamental_from_E(const float *E, const Cam &c, float *F) {
    float Mx[9];   // A^T E
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        Mx[0 * 3 + q] = c.a0 * E[0 * 3 + q];
        Mx[1 * 3 + q] = c.a1 * E[1 * 3 + q];
        Mx[2 * 3 + q] = c.c0 * E[0 * 3 + q] + c.c1 * E[1 * 3 + q] + E[2 * 3 + q];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {   // Fo = Mx A ; F[c][r] = Fo[r][c]
        F[0 * 3 + r] = Mx[r * 3 + 0] * c.a0;
        F[1 * 3 + r] = Mx[r * 3 + 1] * c.a1;
        F[2 * 3 + r] = Mx[r * 3 + 0] * c.c0 + Mx[r * 3 + 1] * c.c1 + Mx[r * 3 + 2];
    }
}

// Two matches per lane at once on packed-fp32 VALU (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32): every per-match
// quantity is a float2 (x = match A, y = match B).  P2 is VALU-issue bound (2 waves per SIMD x ~85 instructions per
// match when the compiler packs within one match), so packing ACROSS matches nearly halves its instruction count.
typedef float v2f __attribute__((ext_vector_type(2)));
typedef int v2i __attribute__((ext_vector_type(2)));
__device__ __forceinline__ v2f pd_fma2(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ v2f pd_splat(float a) { return (v2f){a, a}; }

// per-frame tables in LDS, 16 bytes at a time
__device__ __forceinline__ void frame_load(const Lds &L, int n, float (&R)[9], float (&t)[3]) {
    const float4 *p = (const float4 *)(L.Rc + n * PD_FR_STRIDE);
    const float4 a = p[0], b = p[1], c = p[2];
    R[0] = a.x; R[1] = a.y; R[2] = a.z; R[3] = a.w;
    R[4] = b.x; R[5] = b.y; R[6] = b.z; R[7] = b.w;
    R[8] = c.x; t[0] = c.y; t[1] = c.z; t[2] = c.w;
}
__device__ __forceinline__ void params_load(const float *tab, int n, float (&x)[9]) {     // tab = L.xst or L.mst
    const float4 *p = (const float4 *)(tab + n * PD_XS_STRIDE);
    const float4 a = p[0], b = p[1];
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
    x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
    x[8] = tab[n * PD_XS_STRIDE + 8];
}
__device__ __forceinline__ void params_store(float *tab, int n, const float (&x)[9]) {
    float4 *p = (float4 *)(tab + n * PD_XS_STRIDE);
    p[0] = make_float4(x[0], x[1], x[2], x[3]);
    p[1] = make_float4(x[4], x[5], x[6], x[7]);
    tab[n * PD_XS_STRIDE + 8] = x[8];
}

// decode one frame's 9-vector into R_cv, t_cv, focal (camera_transform.py:80-97 + pytorch3d
// quaternion_to_matrix + opencv_from_cameras_projection); executed by lane n of wave 0.  In three parts, so that a stage
// that leaves R / T / the focal lengths alone (geometry_guided_sampling.py:144-151) does not recompute them.
__device__ __forceinline__ void decode_frame_r(const float *x, float *Rc) {
    const float r = x[3], i = x[4], j = x[5], k = x[6];
    const float two_s = 2.0f * pd_rcp(r * r + i * i + j * j + k * k);
    float R[9];
    R[0] = 1.0f - two_s * (j * j + k * k);
    R[1] = two_s * (i * j - k * r);
    R[2] = two_s * (i * k + j * r);
    R[3] = two_s * (i * j + k * r);
    R[4] = 1.0f - two_s * (i * i + k * k);
    R[5] = two_s * (j * k - i * r);
    R[6] = two_s * (i * k - j * r);
    R[7] = two_s * (j * k + i * r);
    R[8] = 1.0f - two_s * (i * i + j * j);
    // Rc[a][b] = D[a] * R[b][a], D = diag(-1,-1,1); tc = D * T
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c) Rc[a * 3 + c] = (a < 2 ? -1.0f : 1.0f) * R[c * 3 + a];
}
__device__ __forceinline__ void decode_frame_t(const float *x, float *tc) {
    tc[0] = -x[0];
    tc[1] = -x[1];
    tc[2] = x[2];
}
__device__ __forceinline__ void decode_frame_fl(const float *x, float &flx, float &fly, float &px, float &py) {
    const float fx = __expf(x[7] + 1.8f), fy = __expf(x[8] + 1.8f);
    px = (fx >= 0.1f && fx <= 20.0f) ? 1.0f : 0.0f;   // torch.clamp backward passes min <= v <= max
    py = (fy >= 0.1f && fy <= 20.0f) ? 1.0f : 0.0f;
    flx = fminf(fmaxf(fx, 0.1f), 20.0f);
    fly = fminf(fmaxf(fy, 0.1f), 20.0f);
}
__device__ __forceinline__ void decode_frame(const float *x, float *Rc, float *tc, float &flx, float &fly,
                                             float &px, float &py) {
    decode_frame_r(x, Rc);
    decode_frame_t(x, tc);
    decode_frame_fl(x, flx, fly, px, py);
}

// wave 0: publish the decoded cameras of the current parameters to LDS (do_*: the parts whose parameters changed)
__device__ __forceinline__ void decode_all(const Lds &L, const float *xr, int lane, int N, const PdSeqDesc &D, bool do_r = true,
                                           bool do_t = true, bool do_fl = true) {
    if (lane < N) {
        float *dst = L.Rc + lane * PD_FR_STRIDE;
        if (do_r) {
            float Rc[9];
            decode_frame_r(xr, Rc);
            ((float4 *)dst)[0] = make_float4(Rc[0], Rc[1], Rc[2], Rc[3]);
            ((float4 *)dst)[1] = make_float4(Rc[4], Rc[5], Rc[6], Rc[7]);
            dst[8] = Rc[8];
        }
        if (do_t) decode_frame_t(xr, dst + 9);
    }
    if (!do_fl) return;                               // (wave-uniform)
    float flx = 0.f, fly = 0.f, px = 0.f, py = 0.f;
    if (lane < N) {
        decode_frame_fl(xr, flx, fly, px, py);
        *(float4 *)&L.fl[lane * 4] = make_float4(flx, fly, px, py);
    }
    // focal_length.mean(dim=0) over all cameras (geometry_guided_sampling.py:142)
    int n_op = N;
    asm volatile("" : "+s"(n_op));                   // formed here every time: hoisted out of the iteration loop the reciprocal becomes a register held
    const float rN = pd_rcp((float)n_op);            // for the whole launch -- in the 168-register variants a spill, reloaded from scratch on the critical path
    float fbx, fby;
    wave_allsum2(flx, fly, fbx, fby);
    fbx *= rN;
    fby *= rN;
    if (lane == 0) {
        const float a0 = pd_rcp(fbx * D.sc), a1 = pd_rcp(fby * D.sc);
        L.cam[0] = a0;
        L.cam[1] = a1;
        L.cam[2] = -D.cx * a0;
        L.cam[3] = -D.cy * a1;
        L.cam[4] = fbx;
        L.cam[5] = fby;
    }
}

// lane `K` of this lane's 16-lane row (DPP row_newbcast); the whole row must be active
template <int K>
__device__ __forceinline__ float row_bcast(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x150 + K, 0xf, 0xf, false));
}

// The chain rule from dL/dR (PyTorch3D R = I + two_s Pm(q), two_s = 2 / |q|^2) to the un-normalised quaternion is LINEAR in dL/dR:
// dL/dq_x = sum_c J[x][c] dL/dR[c], J[x][c] = two_s dPm_c/dq_x - two_s^2 q_x Pm_c.  J depends on the parameters only, so an idle wave
// (lane = frame) forms it while the others compute the next F's -- off the critical path -- and the per-frame sums of the backward
// phase turn into dL/dq with nine multiply-adds per quaternion component.  Stored for the ORDER those sums come in:
// S[m], m = a * 3 + b, = D[a] dL/dRc[a][b] = dL/dR[b][a]  ->  W[frame][x][m] = J[x][b * 3 + a]   (rows padded to 12 floats).
__device__ __forceinline__ void jac_row(const float (&q)[4], const float (&dPx)[9], float qx, float (&w)[9]) {
    const float r = q[0], i = q[1], j = q[2], k = q[3];
    const float rn2 = pd_rcp(r * r + i * i + j * j + k * k);
    const float ts = 2.0f * rn2, qs = ts * ts * qx;
    const float Pm[9] = {-(j * j + k * k), i * j - k * r, i * k + j * r, i * j + k * r, -(i * i + k * k), j * k - i * r, i * k - j * r, j * k + i * r, -(i * i + j * j)};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b2 = 0; b2 < 3; ++b2) w[a * 3 + b2] = ts * dPx[b2 * 3 + a] - qs * Pm[b2 * 3 + a];
}
// row x of the Jacobian of the quaternion q (x is a compile-time constant in jac_all's unrolled loop, a lane value in the general path)
__device__ __forceinline__ void jac_row_x(const float (&q)[4], int x, float (&w)[9]) {
    const float r = q[0], i = q[1], j = q[2], k = q[3];
    if (x == 0) {
        const float d[9] = {0.0f, -k, j, k, 0.0f, -i, -j, i, 0.0f};
        jac_row(q, d, r, w);
    } else if (x == 1) {
        const float d[9] = {0.0f, j, k, j, -2.0f * i, -r, k, r, -2.0f * i};
        jac_row(q, d, i, w);
    } else if (x == 2) {
        const float d[9] = {-2.0f * j, i, r, i, 0.0f, k, -r, k, -2.0f * j};
        jac_row(q, d, j, w);
    } else {
        const float d[9] = {-2.0f * k, -r, i, r, -2.0f * k, j, i, j, 0.0f};
        jac_row(q, d, k, w);
    }
}
__device__ __forceinline__ void jac_all(const Lds &L, int lane, int N) {
    if (lane >= N || N > PD_GGS_FAST_FRAMES) return;
    const float q[4] = {L.xst[lane * PD_XS_STRIDE + 3], L.xst[lane * PD_XS_STRIDE + 4], L.xst[lane * PD_XS_STRIDE + 5], L.xst[lane * PD_XS_STRIDE + 6]};
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        float w[9];
        jac_row_x(q, x, w);
        float4 *dst = (float4 *)(L.W + (lane * 4 + x) * 12);
        dst[0] = make_float4(w[0], w[1], w[2], w[3]);
        dst[1] = make_float4(w[4], w[5], w[6], w[7]);
        dst[2] = make_float4(w[8], 0.0f, 0.0f, 0.0f);
    }
}
