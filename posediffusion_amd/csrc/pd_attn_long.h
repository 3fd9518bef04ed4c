// pd_attn_long.h -- the attention core for sequences of more than 64 frames (up to PD_MAX_DENOISER_FRAMES = 256): softmax(q k^T / sqrt(hd)) v
// with K and V streamed through LDS in tiles of 64 keys.  The kernels of pd_attn.h and pd_gen_attn_kernel map one lane to one key and hold K
// and V of a (sequence, head) whole in LDS: 2 x 256 x 132 x 4 B = 270 KB at 256 frames of the default head, above the 160 KB of a CU.
//
//   grid      (sequence x head, blocks of 4 x PD_ATTN_LONG_RPW = 20 query rows): B = 1, N = 256 is 52 workgroups, not 4.  Every wave works
//             on PD_ATTN_LONG_RPW query rows at once, as pd_attn_seq_kernel does: one K (V) read from LDS serves all of them.
//   pass 1    K tiles of 64 keys through ONE tile buffer ([64][hd + 4]); lane = key within the tile, so a lane holds up to 4 scores of a
//             query row in registers (the 128-deep fmaf chain over the head dim in ascending order, from zero).
//   softmax   exact, two passes, the formulas of the short kernels: maximum over all N scores (per-lane maximum of its <= 4 scores, then
//             pd_wave_max), e = expf(s - mx), sum = pd_wave_sum(e_tile0 + e_tile1 + e_tile2 + e_tile3), p = e * (1 / sum).  No online
//             rescaling: <= 256 scores per row fit in registers, and this form keeps the arithmetic of the short kernels.  The probabilities
//             of the wave's rows go to LDS ([4 waves][RPW][64 x tiles]).
//   pass 2    V tiles through the same buffer in ascending order; the same fmaf chain over the keys, lanes own output dims lane + 64 c.
//
// Summation order: masked scores are -inf and masked / absent tiles contribute e = 0, and x + 0 = x exactly, so at N <= 64 (one tile) every
// operation is that of pd_attn_kernel / pd_attn_seq_kernel on the same operands: the default-shape kernel gives their bits
// (PD_OPT_DENOISER_LONG_ATTN = 1 forces it there; tests/test_gpu_long_sequences.py).
//
// Frame counts per sequence (pd_engine_set_frame_counts): `nf` != null gives sequence b its own number of frames Nk = nf[b] <= N in rows
// 0 .. Nk - 1 of its N-row block.  Only keys < Nk are staged, scored and summed -- a padding row of qkv is never read, whatever it holds --, query
// rows >= Nk are skipped (their ctx rows keep what they held; every later kernel is per-row work and the tail writes zeros there), and a
// workgroup whose query rows all lie beyond Nk leaves at once.  With Nk == N every operation is that of the uniform call (same bits).
//
// One body serves the default shape (head dim a compile-time 128: pd_attn_long_kernel<SPLIT_OUT>) and the shape-generic path (runtime head
// dim, a multiple of 4 in [8, 256], rows of stride Dp: pd_gen_attn_long_kernel).
// LDS: pd_attn_long_lds(N, hd) -- 64 832 B at the default head and 256 frames (two workgroups per CU), 107 840 B at head dim 256.
#pragma once
#include <stddef.h>

#define PD_ATTN_LONG_TILE 64       // keys per tile = lanes of a wavefront
#define PD_ATTN_LONG_RPW 5         // query rows per wave (PD_ATTN_RPW of pd_attn_seq_kernel)
#define PD_ATTN_LONG_MAX_TILES 4   // PD_MAX_DENOISER_FRAMES / PD_ATTN_LONG_TILE: scores per lane and query row
#define PD_ATTN_LONG_ROWS (4 * PD_ATTN_LONG_RPW)   // query rows per workgroup of 4 waves

// dynamic LDS in bytes: one K / V tile, the workgroup's scaled query rows, the probabilities of its rows over ceil(N / 64) tiles
static inline size_t pd_attn_long_lds(int N, int hd) {
    const int nt = (N + PD_ATTN_LONG_TILE - 1) / PD_ATTN_LONG_TILE;
    return ((size_t)(PD_ATTN_LONG_TILE + PD_ATTN_LONG_ROWS) * (hd + 4) + (size_t)PD_ATTN_LONG_ROWS * PD_ATTN_LONG_TILE * nt) * sizeof(float);
}

#ifndef PD_ATTN_LONG_HOST_ONLY     // (a plain C++ translation unit may include this file for the function above)
#include "pd_denoiser_dev.h"       // pd_wave_max, pd_wave_sum, DH, NH, DM
#include "pd_gemm_stream.h"        // pd_split_word_as

// HD: the head dim at compile time, 0 = hd_rt.  qkv rows [q | k | v] of Dp columns each, head h at columns h hd ..; ctx rows of stride Dp.
// SPLIT_OUT: 0 fp32, 1 bf16 split words, 2 fp16 split words of ctx * out_scale (pd_split_word_as)
template <int HD, int SPLIT_OUT>
__device__ __forceinline__ void pd_attn_long_body(const float *__restrict__ qkv, float *__restrict__ ctx, int N, int nhead, int hd_rt, int Dp,
                                                  float scale, float out_scale, const int *__restrict__ nf) {
    constexpr int R = PD_ATTN_LONG_RPW, TK = PD_ATTN_LONG_TILE, NT = PD_ATTN_LONG_MAX_TILES, NC = HD ? HD / 64 : 4;
    const int hd = HD ? HD : hd_rt, LD = hd + 4, hd4 = hd / 4;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.x / nhead, h = blockIdx.x % nhead, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.y * (4 * R);                        // this workgroup's first query row
    const size_t ld3 = (size_t)3 * Dp;
    const float *base = qkv + (size_t)b * N * ld3 + (size_t)h * hd;
    const int Ns = N;                                           // rows per sequence block (the stride of qkv and ctx)
    if (nf) {                                                   // this sequence's own frame count (clamped: nothing is indexed past the block)
        N = max(1, min(nf[b], Ns));
        if (i0 >= N) return;                                    // (uniform over the workgroup, before any barrier)
    }
    const int nt = (N + TK - 1) / TK, PS = TK * nt;
    float *T = lds, *Q = T + TK * LD, *P = Q + 4 * R * LD;      // tile [64][LD], Q [4 R][LD], P [4 waves][R][PS]
    for (int idx = tid; idx < 4 * R * hd4; idx += 256) {
        const int r = idx / hd4, d4 = idx - r * hd4;
        float4 q = *(const float4 *)(base + (size_t)min(i0 + r, N - 1) * ld3 + 4 * d4);
        q.x *= scale; q.y *= scale; q.z *= scale; q.w *= scale;
        *(float4 *)(Q + r * LD + 4 * d4) = q;
    }
    const float4 *qa[R];
#pragma unroll
    for (int t = 0; t < R; ++t) qa[t] = (const float4 *)(Q + (wave * R + t) * LD);
    // ---- pass 1: scores, lane = key within the tile
    float s[R][NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
        for (int t = 0; t < R; ++t) s[t][kt] = -INFINITY;
        if (kt < nt) {                                          // (uniform over the workgroup: the barriers below are reached by all or none)
            const int j0 = kt * TK, jn = min(TK, N - j0);
            __syncthreads();                                    // the previous tile has been read (first tile: nothing to wait for but Q)
            for (int idx = tid; idx < jn * hd4; idx += 256) {
                const int j = idx / hd4, d4 = idx - j * hd4;
                *(float4 *)(T + j * LD + 4 * d4) = *(const float4 *)(base + (size_t)(j0 + j) * ld3 + Dp + 4 * d4);
            }
            __syncthreads();
            const float4 *kb = (const float4 *)(T + min(lane, jn - 1) * LD);
            float acc[R];
#pragma unroll
            for (int t = 0; t < R; ++t) acc[t] = 0.0f;
#pragma unroll 4
            for (int d = 0; d < hd4; ++d) {
                const float4 c = kb[d];
#pragma unroll
                for (int t = 0; t < R; ++t) {
                    const float4 a = qa[t][d];
                    acc[t] = fmaf(a.x, c.x, acc[t]);
                    acc[t] = fmaf(a.y, c.y, acc[t]);
                    acc[t] = fmaf(a.z, c.z, acc[t]);
                    acc[t] = fmaf(a.w, c.w, acc[t]);
                }
            }
#pragma unroll
            for (int t = 0; t < R; ++t) s[t][kt] = lane < jn ? acc[t] : -INFINITY;
        }
    }
    // ---- softmax over all N scores of a row; probabilities to LDS
    float *pw = P + wave * (R * PS);
#pragma unroll
    for (int t = 0; t < R; ++t) {
        float m = s[t][0];
#pragma unroll
        for (int kt = 1; kt < NT; ++kt)
            if (kt < nt) m = fmaxf(m, s[t][kt]);
        const float mx = pd_wave_max(m);
        float e[NT], esum = 0.0f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            e[kt] = (kt < nt && kt * TK + lane < N) ? expf(s[t][kt] - mx) : 0.0f;
            esum = kt == 0 ? e[0] : esum + e[kt];
        }
        const float inv = 1.0f / pd_wave_sum(esum);
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
            if (kt < nt) pw[t * PS + kt * TK + lane] = e[kt] * inv;
    }
    // ---- pass 2: O = P V, keys in ascending order
    float o[R][NC];
#pragma unroll
    for (int t = 0; t < R; ++t)
#pragma unroll
        for (int c = 0; c < NC; ++c) o[t][c] = 0.0f;
    for (int kt = 0; kt < nt; ++kt) {
        const int j0 = kt * TK, jn = min(TK, N - j0);
        __syncthreads();                                        // the tile buffer is free (and, first round, every wave has written its P)
        for (int idx = tid; idx < jn * hd4; idx += 256) {
            const int j = idx / hd4, d4 = idx - j * hd4;
            *(float4 *)(T + j * LD + 4 * d4) = *(const float4 *)(base + (size_t)(j0 + j) * ld3 + 2 * Dp + 4 * d4);
        }
        __syncthreads();
        for (int j = 0; j < jn; ++j) {
            float v[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) v[c] = (HD != 0 || lane + 64 * c < hd) ? T[j * LD + lane + 64 * c] : 0.0f;
#pragma unroll
            for (int t = 0; t < R; ++t) {
                const float pj = pw[t * PS + j0 + j];
#pragma unroll
                for (int c = 0; c < NC; ++c) o[t][c] = fmaf(pj, v[c], o[t][c]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < R; ++t) {
        const int i = i0 + wave * R + t;
        if (i < N) {
            float *out = ctx + (size_t)(b * Ns + i) * Dp + (size_t)h * hd;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int dd = lane + 64 * c;
                if (HD != 0 || dd < hd) {
                    if constexpr (SPLIT_OUT != 0) ((unsigned *)out)[dd] = pd_split_word_as<SPLIT_OUT>(o[t][c], out_scale);
                    else out[dd] = o[t][c];
                }
            }
        }
    }
}

// the default shape: grid (B x NH, ceil(N / PD_ATTN_LONG_ROWS)), 256 threads, pd_attn_long_lds(N, DH) bytes
template <int SPLIT_OUT>
__global__ __launch_bounds__(256) void pd_attn_long_kernel(const float *__restrict__ qkv, float *__restrict__ ctx, int N, float out_scale,
                                                           const int *__restrict__ nf) {
    pd_attn_long_body<DH, SPLIT_OUT>(qkv, ctx, N, NH, DH, DM, 0.08838834764831845f /* 1/sqrt(128) */, out_scale, nf);
}
// the shape-generic path: grid (B x nhead, ceil(N / PD_ATTN_LONG_ROWS)), 256 threads, pd_attn_long_lds(N, hd) bytes (a template like its twin,
// so that only the translation unit that launches it holds an instantiation; the generic path has fp32 activations only: SPLIT_OUT = 0)
template <int SPLIT_OUT>
__global__ __launch_bounds__(256) void pd_gen_attn_long_kernel(const float *__restrict__ qkv, float *__restrict__ ctx, int N, int nhead, int hd, int Dp,
                                                               float scale, const int *__restrict__ nf) {
    pd_attn_long_body<0, SPLIT_OUT>(qkv, ctx, N, nhead, hd, Dp, scale, 1.0f, nf);
}
#endif
