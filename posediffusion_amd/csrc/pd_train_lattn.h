// pd_train_lattn.h -- the trainer's key-tiled attention (included by pd_train_kernels.h): forward with site-0 dropout and its backward for
// sequences of up to PD_TR_LA_MAX_N = 256 frames.  pd_tr_attn_kernel / pd_tr_attn_bwd_kernel map one lane to one key and hold K, V, P and dS
// of a (sequence, head) whole in LDS; these kernels stream K and V through LDS in tiles of 64 keys (the scheme of pd_attn_long.h), so a lane
// holds at most 4 scores of a query row.  The head dim is a run-time value (a multiple of 4, <= 128): nothing here is the denoiser's own.
//
//   pd_tr_lattn_kernel           grid (sequence x head, blocks of 16 query rows).  K tiles -> scores; exact two-pass softmax (maximum over all
//                                scores, e = expf(s - mx), sum = pd_wave_sum(e0 + e1 + e2 + e3), p = e (1 / sum)); DROP: p = keep ? p scale : 0
//                                with the global key index as the mask column; V tiles -> ctx = P V over the keys in ascending order.
//   pd_tr_lattn_bwd_rows_kernel  phase A, same grid.  K tiles -> P; V tiles -> dP_ij = dO_i . V_j (DROP: dP and P~ by selects); rs_i =
//                                pd_wave_sum(dP P of tile 0) + pd_wave_sum(sum of dP P over tiles 1 ..), dS = P (dP - rs) with the
//                                unmasked P; K tiles again -> dQ_i = scale sum_j dS_ij K_j.
//                                Writes (row maximum, 1 / sum, rs of lanes 0 .. 31, rs of lanes 32 .. 63) of every (b, h, i) to `stats`
//                                [B nhead N][4]: under -ffp-contract=fast the first step of the wave sum is fused with the product, so
//                                the two halves of a wave hold sums that differ in their last bit, here as in pd_tr_attn_bwd_kernel.
//   pd_tr_lattn_bwd_keys_kernel  phase B, grid (sequence x head, tiles of 64 keys).  The K and the V tile stay in LDS; the query rows pass in
//                                blocks of 16 in ascending order: P~ and dS of the [16 x 64] block are recomputed from `stats` by the code
//                                phase A ran (pd_tr_la_dots, pd_tr_la_mask) into LDS, then wave w adds row after row into dV_j = sum_i P~_ij dO_i
//                                and dK_j = scale sum_i dS_ij Q_i of its keys j = w, w + 4, ..., held in registers across the blocks.
// No N x N array in global memory, no float atomics; every sum over keys is ascending, every sum over query rows is in row order.
//
// Summation order at N <= 64 (one tile): absent tiles contribute e = 0, dP = 0, P = 0 and are not added at all, so every operation is that
// of pd_tr_attn_kernel / pd_tr_attn_bwd_kernel on the same operands -- the same fmaf chains from zero, the same selects, the same products --
// and the results are theirs bit for bit (PD_TR_OPT_LONG_ATTN = 1 runs these kernels there; tests/test_gpu_train_long.py).
//
// Frame counts (pd_trainer_set_frame_counts): `nf` is null on a uniform call, else nf[b] = the frames of sequence b.  N is then the ROW
// STRIDE alone -- block base, `stats` index, dropout mask row, LDS sizes -- and nk = nf[b] the number of keys and query rows: tile count,
// jn, the lane selects and the row clamps follow nk, so a slot sees the operations of its sequence alone at N = nk and gives its bits.
// The grid is that of the padded N: a workgroup whose rows (tile) lie at or beyond nk writes +0 to the padding rows of ctx / dQ (dK, dV)
// it owns and leaves; `stats` of padding rows are neither written nor read.
#pragma once
#include <stddef.h>

#define PD_TR_LA_TILE 64           // keys per tile = lanes of a wavefront
#define PD_TR_LA_RPW 4              // query rows per wave
#define PD_TR_LA_ROWS (4 * PD_TR_LA_RPW)   // query rows per workgroup (forward, phase A) and per block of phase B
#define PD_TR_LA_MAX_TILES 4
#define PD_TR_LA_PL (PD_TR_LA_TILE + 1)    // row stride of phase B's P~ / dS blocks

constexpr int pd_tr_la_tiles(int N) { return (N + PD_TR_LA_TILE - 1) / PD_TR_LA_TILE; }   // (constexpr: callable from host and device code)
// dynamic LDS in bytes.  Forward: one K / V tile, the scaled query rows, their probabilities over the tiles
static inline size_t pd_tr_lattn_lds(int N, int hd) {
    return ((size_t)(PD_TR_LA_TILE + PD_TR_LA_ROWS) * (hd + 4) + (size_t)PD_TR_LA_ROWS * PD_TR_LA_TILE * pd_tr_la_tiles(N)) * sizeof(float);
}
// phase A: one tile, the scaled query rows, the dO rows, dS of the rows over the tiles
static inline size_t pd_tr_lattn_bwd_rows_lds(int N, int hd) {
    return ((size_t)(PD_TR_LA_TILE + 2 * PD_TR_LA_ROWS) * (hd + 4) + (size_t)PD_TR_LA_ROWS * PD_TR_LA_TILE * pd_tr_la_tiles(N)) * sizeof(float);
}
// phase B: the K and the V tile, 16 scaled query rows and dO rows, the P~ and dS blocks [16][65] (no dependence on N)
static inline size_t pd_tr_lattn_bwd_keys_lds(int N, int hd) {
    (void)N;
    return ((size_t)(2 * PD_TR_LA_TILE + 2 * PD_TR_LA_ROWS) * (hd + 4) + (size_t)2 * PD_TR_LA_ROWS * PD_TR_LA_PL) * sizeof(float);
}

#ifndef PD_TR_LATTN_HOST_ONLY       // (a plain C++ translation unit may include this file for the functions above)

// PD_TR_LA_MAX_N and PD_TR_LA_STATS size both trainers' allocations: pd_train_launch.h holds them (pd_train_kernels.h has included it)
static_assert(PD_TR_LA_MAX_N == PD_TR_LA_TILE * PD_TR_LA_MAX_TILES, "PD_TR_LA_MAX_N is the keys of PD_TR_LA_MAX_TILES tiles");

// rows i0 .. i0 + 15 of `src` (row stride ld, clamped to row N - 1) times `mul` into dst [16][hd + 4]
__device__ __forceinline__ void pd_tr_la_stage_rows(const float *__restrict__ src, size_t ld, int i0, int N, int hd, float mul, float *dst) {
    const int LD = hd + 4, hd4 = hd / 4;
    for (int idx = threadIdx.x; idx < PD_TR_LA_ROWS * hd4; idx += 256) {
        const int r = idx / hd4, d4 = idx - r * hd4;
        float4 q = *(const float4 *)(src + (size_t)min(i0 + r, N - 1) * ld + 4 * d4);
        q.x *= mul; q.y *= mul; q.z *= mul; q.w *= mul;
        *(float4 *)(dst + r * LD + 4 * d4) = q;
    }
}
// +0 into columns 0 .. hd - 1 of rows r0 .. r1 - 1 of dst (row stride ld): the padding rows a workgroup owns while frame counts are set
__device__ __forceinline__ void pd_tr_la_zero_rows(float *__restrict__ dst, size_t ld, int r0, int r1, int hd) {
    for (int idx = threadIdx.x; idx < (r1 - r0) * hd; idx += 256) {
        const int r = idx / hd, c = idx - r * hd;
        dst[(size_t)(r0 + r) * ld + c] = 0.0f;
    }
}
// keys j0 .. j0 + jn - 1 of K (which = 1) or V (which = 2) into dst [64][hd + 4]
__device__ __forceinline__ void pd_tr_la_stage_tile(const float *__restrict__ base, size_t ld3, int d, int which, int j0, int jn, int hd, float *dst) {
    const int LD = hd + 4, hd4 = hd / 4;
    for (int idx = threadIdx.x; idx < jn * hd4; idx += 256) {
        const int j = idx / hd4, d4 = idx - j * hd4;
        *(float4 *)(dst + j * LD + 4 * d4) = *(const float4 *)(base + (size_t)(j0 + j) * ld3 + (size_t)which * d + 4 * d4);
    }
}
// acc[t] = sum over the head dim (ascending, from zero) of rows[t][.] T[lane][.]: the scores (rows = scale q, T = a K tile) and dP
// (rows = dO, T = a V tile) of the wave's PD_TR_LA_RPW query rows against the key of this lane; one read of the key serves the four rows
__device__ __forceinline__ void pd_tr_la_dots(const float *rows, const float *T, int LD, int hd4, int lane, int jn, float acc[PD_TR_LA_RPW]) {
    const float4 *kb = (const float4 *)(T + min(lane, jn - 1) * LD);
#pragma unroll
    for (int t = 0; t < PD_TR_LA_RPW; ++t) acc[t] = 0.0f;
#pragma unroll 2
    for (int d4 = 0; d4 < hd4; ++d4) {
        const float4 c = kb[d4];
#pragma unroll
        for (int t = 0; t < PD_TR_LA_RPW; ++t) {
            const float4 a = ((const float4 *)(rows + t * LD))[d4];
            acc[t] = fmaf(a.x, c.x, acc[t]);
            acc[t] = fmaf(a.y, c.y, acc[t]);
            acc[t] = fmaf(a.z, c.z, acc[t]);
            acc[t] = fmaf(a.w, c.w, acc[t]);
        }
    }
}
// the scores of all tiles of the wave's rows (-inf where there is no key), K tiles through T; every thread of the workgroup calls it
__device__ __forceinline__ void pd_tr_la_scores(const float *__restrict__ base, size_t ld3, int d, int N, int hd, const float *rows, float *T,
                                                float s[PD_TR_LA_RPW][PD_TR_LA_MAX_TILES]) {
    const int LD = hd + 4, lane = threadIdx.x & 63, nt = pd_tr_la_tiles(N);
#pragma unroll
    for (int kt = 0; kt < PD_TR_LA_MAX_TILES; ++kt) {
#pragma unroll
        for (int t = 0; t < PD_TR_LA_RPW; ++t) s[t][kt] = -INFINITY;
        if (kt < nt) {                                          // (uniform over the workgroup: all or none reach the barriers)
            const int j0 = kt * PD_TR_LA_TILE, jn = min(PD_TR_LA_TILE, N - j0);
            __syncthreads();                                    // the previous tile has been read; first tile: the staged rows are complete
            pd_tr_la_stage_tile(base, ld3, d, 1, j0, jn, hd, T);
            __syncthreads();
            float acc[PD_TR_LA_RPW];
            pd_tr_la_dots(rows, T, LD, hd / 4, lane, jn, acc);
#pragma unroll
            for (int t = 0; t < PD_TR_LA_RPW; ++t) s[t][kt] = lane < jn ? acc[t] : -INFINITY;
        }
    }
}
// softmax of one row held as <= 4 scores per lane: s becomes the probabilities (0 where there is no key); mx and inv = 1 / sum are returned
__device__ __forceinline__ void pd_tr_la_softmax(float s[PD_TR_LA_MAX_TILES], int N, int lane, float *mx_out, float *inv_out) {
    const int nt = pd_tr_la_tiles(N);
    float m = s[0];
#pragma unroll
    for (int kt = 1; kt < PD_TR_LA_MAX_TILES; ++kt)
        if (kt < nt) m = fmaxf(m, s[kt]);
    const float mx = pd_wave_max(m);
    float esum = 0.0f;
#pragma unroll
    for (int kt = 0; kt < PD_TR_LA_MAX_TILES; ++kt) {
        const float e = (kt < nt && kt * PD_TR_LA_TILE + lane < N) ? expf(s[kt] - mx) : 0.0f;
        if (kt == 0) esum = e;
        else if (kt < nt) esum += e;
        s[kt] = e;
    }
    const float inv = 1.0f / pd_wave_sum(esum);
#pragma unroll
    for (int kt = 0; kt < PD_TR_LA_MAX_TILES; ++kt) s[kt] = s[kt] * inv;
    *mx_out = mx;
    *inv_out = inv;
}
// (dP, P~) of one element from the raw dP = dO . V and the unmasked P: selects, as in pd_tr_attn_bwd_kernel (see the comment there)
template <bool DROP>
__device__ __forceinline__ void pd_tr_la_mask(const PdTrDrop &dr, unsigned int row, unsigned int col, float p, float *dp, float *pt) {
    *pt = p;
    if constexpr (DROP) {
        const bool keep = pd_tr_keep(dr, row, col);
        *dp = keep ? *dp * dr.scale : 0.0f;
        *pt = keep ? p * dr.scale : 0.0f;
    }
}

template <bool DROP>
__global__ __launch_bounds__(256) void pd_tr_lattn_kernel(const float *__restrict__ qkv, float *__restrict__ ctx, const int *__restrict__ nf, int N,
                                                          int nhead, int hd, int d, float scale, PdTrDrop dr) {
    constexpr int R = PD_TR_LA_RPW, TK = PD_TR_LA_TILE, NT = PD_TR_LA_MAX_TILES;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int LD = hd + 4;
    const int b = blockIdx.x / nhead, h = blockIdx.x % nhead, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nk = nf ? nf[b] : N;                                      // keys and query rows of this sequence; N stays the row stride
    const int i0 = blockIdx.y * PD_TR_LA_ROWS, nt = pd_tr_la_tiles(nk), PS = TK * nt;
    const size_t ld3 = (size_t)3 * d;
    const float *base = qkv + (size_t)b * N * ld3 + (size_t)h * hd;
    if (i0 >= nk) {                                                     // padding rows only (uniform over the workgroup): ctx = +0
        pd_tr_la_zero_rows(ctx + (size_t)b * N * d + (size_t)h * hd, (size_t)d, i0, min(i0 + PD_TR_LA_ROWS, N), hd);
        return;
    }
    float *T = lds, *Q = T + TK * LD, *P = Q + PD_TR_LA_ROWS * LD;      // tile [64][LD], Q [16][LD], P [16][PS]
    pd_tr_la_stage_rows(base, ld3, i0, nk, hd, scale, Q);
    float s[R][NT];
    pd_tr_la_scores(base, ld3, d, nk, hd, Q + wave * R * LD, T, s);
    float *pw = P + wave * R * PS;
#pragma unroll
    for (int t = 0; t < R; ++t) {
        float mx, inv;
        pd_tr_la_softmax(s[t], nk, lane, &mx, &inv);
        const int i = min(i0 + wave * R + t, nk - 1);
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
            if (kt < nt) {
                float p = s[t][kt];
                if constexpr (DROP) p = pd_tr_keep(dr, (unsigned int)(blockIdx.x * N + i), (unsigned int)(kt * TK + lane)) ? p * dr.scale : 0.0f;
                pw[t * PS + kt * TK + lane] = p;
            }
    }
    float o[R][2];
#pragma unroll
    for (int t = 0; t < R; ++t) o[t][0] = o[t][1] = 0.0f;
    for (int kt = 0; kt < nt; ++kt) {
        const int j0 = kt * TK, jn = min(TK, nk - j0);
        __syncthreads();                                        // the tile buffer is free (and, first round, the wave's P rows are written)
        pd_tr_la_stage_tile(base, ld3, d, 2, j0, jn, hd, T);
        __syncthreads();
        for (int j = 0; j < jn; ++j) {
            float v[2];
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) v[cc] = lane + 64 * cc < hd ? T[j * LD + lane + 64 * cc] : 0.0f;
#pragma unroll
            for (int t = 0; t < R; ++t) {
                const float pj = pw[t * PS + j0 + j];
#pragma unroll
                for (int cc = 0; cc < 2; ++cc) o[t][cc] = fmaf(pj, v[cc], o[t][cc]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < R; ++t) {
        const int i = i0 + wave * R + t;
        if (i < N) {
            float *out = ctx + (size_t)(b * N + i) * d + (size_t)h * hd;
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const int dd = lane + 64 * cc;
                if (dd < hd) out[dd] = i < nk ? o[t][cc] : 0.0f;
            }
        }
    }
}

// phase A of the backward: dQ and the row statistics
template <bool DROP>
__global__ __launch_bounds__(256) void pd_tr_lattn_bwd_rows_kernel(const float *__restrict__ qkv, const float *__restrict__ dctx,
                                                                   float *__restrict__ dqkv, float *__restrict__ stats, const int *__restrict__ nf,
                                                                   int N, int nhead, int hd, int d, float scale, PdTrDrop dr) {
    constexpr int R = PD_TR_LA_RPW, TK = PD_TR_LA_TILE, NT = PD_TR_LA_MAX_TILES;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int LD = hd + 4;
    const int b = blockIdx.x / nhead, h = blockIdx.x % nhead, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nk = nf ? nf[b] : N;
    const int i0 = blockIdx.y * PD_TR_LA_ROWS, nt = pd_tr_la_tiles(nk), PS = TK * nt;
    const size_t ld3 = (size_t)3 * d;
    const float *base = qkv + (size_t)b * N * ld3 + (size_t)h * hd;
    const float *dO = dctx + (size_t)b * N * d + (size_t)h * hd;
    float *dbase = dqkv + (size_t)b * N * ld3 + (size_t)h * hd;
    if (i0 >= nk) {                                                     // padding rows only: dQ = +0 (in_proj's weight gradient sums these rows)
        pd_tr_la_zero_rows(dbase, ld3, i0, min(i0 + PD_TR_LA_ROWS, N), hd);
        return;
    }
    float *T = lds, *Q = T + TK * LD, *G = Q + PD_TR_LA_ROWS * LD, *DS = G + PD_TR_LA_ROWS * LD;    // tile, Q [16][LD], dO [16][LD], dS [16][PS]
    pd_tr_la_stage_rows(base, ld3, i0, nk, hd, scale, Q);
    pd_tr_la_stage_rows(dO, (size_t)d, i0, nk, hd, 1.0f, G);
    float p[R][NT], dp[R][NT];
    pd_tr_la_scores(base, ld3, d, nk, hd, Q + wave * R * LD, T, p);
    float mx[R], inv[R];
#pragma unroll
    for (int t = 0; t < R; ++t) pd_tr_la_softmax(p[t], nk, lane, &mx[t], &inv[t]);
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
        for (int t = 0; t < R; ++t) dp[t][kt] = 0.0f;
        if (kt < nt) {
            const int j0 = kt * TK, jn = min(TK, nk - j0);
            __syncthreads();
            pd_tr_la_stage_tile(base, ld3, d, 2, j0, jn, hd, T);
            __syncthreads();
            float acc[R];
            pd_tr_la_dots(G + wave * R * LD, T, LD, hd / 4, lane, jn, acc);
#pragma unroll
            for (int t = 0; t < R; ++t) dp[t][kt] = lane < jn ? acc[t] : 0.0f;
        }
    }
    float *dsw = DS + wave * R * PS;
#pragma unroll
    for (int t = 0; t < R; ++t) {
        const int i = i0 + wave * R + t, ic = min(i, nk - 1);
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
            if (kt < nt) {
                float pt;
                pd_tr_la_mask<DROP>(dr, (unsigned int)(blockIdx.x * N + ic), (unsigned int)(kt * TK + lane), p[t][kt], &dp[t][kt], &pt);
            }
        // rs = pd_wave_sum(dP P of tile 0) + pd_wave_sum(sum of dP P over tiles 1 ..), not one wave sum of the sum over all tiles: the first
        // term is the short kernel's expression as it stands there.  Under -ffp-contract=fast its product is fused into the first add of
        // pd_wave_sum (fma(dp, p, shuffled product)); a sum over tiles that merely has one term is not fused and rounds differently.
        float rs = pd_wave_sum(dp[t][0] * p[t][0]);
        if (nt > 1) {
            float part = dp[t][1] * p[t][1];
#pragma unroll
            for (int kt = 2; kt < NT; ++kt)
                if (kt < nt) part += dp[t][kt] * p[t][kt];
            rs += pd_wave_sum(part);
        }
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
            if (kt < nt) dsw[t * PS + kt * TK + lane] = p[t][kt] * (dp[t][kt] - rs);
        // rs has one value per half of the wave: the fused first step adds a lane's exact product to its partner's rounded one, which is
        // not symmetric between lanes l and l ^ 32; the later steps stay inside a half.  Phase B needs the value of its key's lane.
        if ((lane & 31) == 0 && i < nk) {
            float *st = stats + ((size_t)blockIdx.x * N + i) * PD_TR_LA_STATS;
            if (lane == 0) {
                st[0] = mx[t];
                st[1] = inv[t];
            }
            st[2 + (lane >> 5)] = rs;
        }
    }
    float o[R][2];
#pragma unroll
    for (int t = 0; t < R; ++t) o[t][0] = o[t][1] = 0.0f;
    for (int kt = 0; kt < nt; ++kt) {
        const int j0 = kt * TK, jn = min(TK, nk - j0);
        __syncthreads();
        pd_tr_la_stage_tile(base, ld3, d, 1, j0, jn, hd, T);
        __syncthreads();
        for (int j = 0; j < jn; ++j) {
            float k[2];
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) k[cc] = lane + 64 * cc < hd ? T[j * LD + lane + 64 * cc] : 0.0f;
#pragma unroll
            for (int t = 0; t < R; ++t) {
                const float dj = dsw[t * PS + j0 + j];
#pragma unroll
                for (int cc = 0; cc < 2; ++cc) o[t][cc] = fmaf(dj, k[cc], o[t][cc]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < R; ++t) {
        const int i = i0 + wave * R + t;
        if (i < N) {
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const int dd = lane + 64 * cc;
                if (dd < hd) dbase[(size_t)i * ld3 + dd] = i < nk ? scale * o[t][cc] : 0.0f;
            }
        }
    }
}

// phase B of the backward: dK and dV of one tile of 64 keys
template <bool DROP>
__global__ __launch_bounds__(256) void pd_tr_lattn_bwd_keys_kernel(const float *__restrict__ qkv, const float *__restrict__ dctx,
                                                                   float *__restrict__ dqkv, const float *__restrict__ stats,
                                                                   const int *__restrict__ nf, int N, int nhead, int hd, int d, float scale,
                                                                   PdTrDrop dr) {
    constexpr int R = PD_TR_LA_RPW, TK = PD_TR_LA_TILE, PL = PD_TR_LA_PL, KPW = PD_TR_LA_TILE / 4;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int LD = hd + 4;
    const int b = blockIdx.x / nhead, h = blockIdx.x % nhead, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nk = nf ? nf[b] : N;
    const int j0 = blockIdx.y * TK, jn = min(TK, nk - j0);
    const size_t ld3 = (size_t)3 * d;
    const float *base = qkv + (size_t)b * N * ld3 + (size_t)h * hd;
    const float *dO = dctx + (size_t)b * N * d + (size_t)h * hd;
    float *dbase = dqkv + (size_t)b * N * ld3 + (size_t)h * hd;
    if (j0 >= nk) {                                                     // a tile of padding keys only: dK = dV = +0
        pd_tr_la_zero_rows(dbase + d, ld3, j0, min(j0 + TK, N), hd);
        pd_tr_la_zero_rows(dbase + 2 * d, ld3, j0, min(j0 + TK, N), hd);
        return;
    }
    float *Kt = lds, *Vt = Kt + TK * LD, *Q = Vt + TK * LD, *G = Q + PD_TR_LA_ROWS * LD, *Pb = G + PD_TR_LA_ROWS * LD, *Sb = Pb + PD_TR_LA_ROWS * PL;
    pd_tr_la_stage_tile(base, ld3, d, 1, j0, jn, hd, Kt);
    pd_tr_la_stage_tile(base, ld3, d, 2, j0, jn, hd, Vt);
    float dk[KPW][2], dv[KPW][2];
#pragma unroll
    for (int k = 0; k < KPW; ++k) dk[k][0] = dk[k][1] = dv[k][0] = dv[k][1] = 0.0f;
    for (int i0 = 0; i0 < nk; i0 += PD_TR_LA_ROWS) {
        const int in = min(PD_TR_LA_ROWS, nk - i0);
        pd_tr_la_stage_rows(base, ld3, i0, nk, hd, scale, Q);   // (the previous block's recomputation has passed the barrier below)
        pd_tr_la_stage_rows(dO, (size_t)d, i0, nk, hd, 1.0f, G);
        __syncthreads();                                        // first round: the K and V tiles too
        float sc[R], dpv[R];
        pd_tr_la_dots(Q + wave * R * LD, Kt, LD, hd / 4, lane, jn, sc);
        pd_tr_la_dots(G + wave * R * LD, Vt, LD, hd / 4, lane, jn, dpv);
#pragma unroll
        for (int t = 0; t < R; ++t) {
            const int r = wave * R + t, ic = min(i0 + r, nk - 1);
            const float *st = stats + ((size_t)blockIdx.x * N + ic) * PD_TR_LA_STATS;
            const float mx = st[0], inv = st[1], rs = st[2 + (lane >> 5)];
            const float e = lane < jn ? expf(sc[t] - mx) : 0.0f;
            const float p = e * inv;
            float dp = lane < jn ? dpv[t] : 0.0f, pt;
            pd_tr_la_mask<DROP>(dr, (unsigned int)(blockIdx.x * N + ic), (unsigned int)(j0 + lane), p, &dp, &pt);
            Pb[r * PL + lane] = pt;
            Sb[r * PL + lane] = p * (dp - rs);
        }
        __syncthreads();
        for (int r = 0; r < in; ++r) {
            float g[2], q[2];
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const int dd = min(lane + 64 * cc, hd - 1);
                g[cc] = dO[(size_t)(i0 + r) * d + dd];
                q[cc] = base[(size_t)(i0 + r) * ld3 + dd];
            }
#pragma unroll
            for (int k = 0; k < KPW; ++k) {
                const float pij = Pb[r * PL + wave + 4 * k], dsij = Sb[r * PL + wave + 4 * k];
#pragma unroll
                for (int cc = 0; cc < 2; ++cc) {
                    dv[k][cc] = fmaf(pij, g[cc], dv[k][cc]);
                    dk[k][cc] = fmaf(dsij, q[cc], dk[k][cc]);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < KPW; ++k) {
        const int j = wave + 4 * k;
        if (j0 + j < N) {                                       // keys jn .. of the tile are padding rows: +0
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const int dd = lane + 64 * cc;
                if (dd < hd) {
                    dbase[(size_t)(j0 + j) * ld3 + d + dd] = j < jn ? scale * dk[k][cc] : 0.0f;
                    dbase[(size_t)(j0 + j) * ld3 + 2 * d + dd] = j < jn ? dv[k][cc] : 0.0f;
                }
            }
        }
    }
}
#endif
