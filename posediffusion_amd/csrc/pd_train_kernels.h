// pd_train_kernels.h -- device code of the training branch with gradients (pd_train.hip; include/pd_engine_train.h).
//
// Everything is exact fp32.  Every matrix product -- forward Linear, data gradient, weight gradient -- is ONE kernel,
// pd_tr_gemm_kernel: C(i, j) = sum_r A(i, r) B(r, j) on v_mfma_f32_32x32x2_f32 with both operands addressed through a row and a column
// stride, so that the caller's LIVE row-major weights [out, in] serve as B of the forward (B(r, j) = W[j][r]), as B of the data gradient
// (B(r, j) = W[r][j]) and never need a padded or transposed copy.  Tiles are 64 x 64 x 32; rows, columns and the reduction tail are
// zero-filled while they are staged into LDS, so any width works (K = 702, d_model = 96, ff = 200, Nout = 9).
//
// Determinism: no float atomics anywhere.  A reduction over the token rows (weight gradients, bias gradients, LayerNorm gamma / beta) is
// cut into chunks whose size depends on M = B x N alone (pd_tr_chunks); every chunk writes its partial sum to a workspace slice and
// pd_tr_reduce_kernel adds the slices in chunk order.
//
// pd_train.hip is the ONE translation unit that includes this file.  The backbone trainer (pd_vit_train.hip) runs the GEMM, the reductions,
// the column sums, LayerNorm and the key-tiled attention through the launch helpers of pd_train_launch.h, which pd_train.hip defines.
#pragma once
#include "pd_denoiser_dev.h"
#include "pd_train_launch.h"        // PD_TR_MAX_CHUNKS, PD_TR_MAX_HD, PdTrDrop, PdTrGemm

#include <math.h>

#define PD_TR_TILE 64
#define PD_TR_KC 32
#define PD_TR_LD 65                 // LDS row stride of a staged tile [KC][64]: both staging patterns and the MFMA reads stay spread over the banks
#define PD_TR_FIRST_FIXED 317       // harmonic (180) + x (9) + t_emb (128): the columns of _first before z
#define PD_TR_MAX_N 64
#define PD_TR_TAIL_PER 16           // hidden <= 1024 = 16 values per lane

#define PD_TR_ERR_T_RANGE 8u        // the trainer's error word: a timestep outside [0, timesteps) was clamped

// --------------------------------------------------------------------------------------------
// dropout masks (DESIGN 3.9 "Dropout"): Philox4x32-10, counter = (row >> 2, column, 4 layer + site, step), key = the call's 64-bit seed;
// the element at (row, column) is kept iff word (row & 3) of the output is >= thr = floor(p 2^32).  Four consecutive rows share one call.
// Masks are never stored: forward and backward recompute them from (seed, step, p).
// --------------------------------------------------------------------------------------------
struct PdTrRand {
    unsigned int w[4];
};

__host__ __device__ __forceinline__ PdTrRand pd_tr_philox(unsigned int c0, unsigned int c1, unsigned int c2, unsigned int c3, unsigned int k0,
                                                          unsigned int k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned int n0 = (unsigned int)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned int)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned int)p1;
        c3 = (unsigned int)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    PdTrRand r;
    r.w[0] = c0; r.w[1] = c1; r.w[2] = c2; r.w[3] = c3;
    return r;
}

__host__ __device__ __forceinline__ bool pd_tr_keep(const PdTrDrop &dr, unsigned int row, unsigned int col) {
    const PdTrRand r = pd_tr_philox(row >> 2, col, dr.ctr2, dr.step, dr.key0, dr.key1);
    const unsigned int k = row & 3;                     // selected, not indexed: a run-time index would put the four words in scratch
    const unsigned int lo = k & 1 ? r.w[1] : r.w[0], hi = k & 1 ? r.w[3] : r.w[2];
    return (k & 2 ? hi : lo) >= dr.thr;
}

// DROP: the epilogue applies `dr` after the ReLU / mask and before the residual add: v = keep ? v scale : 0.  A lane's 16 accumulators are
// four groups of four consecutive rows at one column, so a group is one Philox call.  DROP = false is the kernel as it was.
template <bool DROP>
__global__ __launch_bounds__(256) void pd_tr_gemm_kernel(PdTrGemm g, PdTrDrop dr) {
    __shared__ float As[PD_TR_KC * PD_TR_LD];
    __shared__ float Bs[PD_TR_KC * PD_TR_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const int i0 = blockIdx.y * PD_TR_TILE, j0 = blockIdx.x * PD_TR_TILE;
    const int r_begin = blockIdx.z * g.r_chunk;
    const int r_end = min(g.R, r_begin + g.r_chunk);
    const int wi = (wave >> 1) * 32, wj = (wave & 1) * 32;
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
    for (int r0 = r_begin; r0 < r_end; r0 += PD_TR_KC) {
#pragma unroll
        for (int q = 0; q < (PD_TR_TILE * PD_TR_KC) / 256; ++q) {
            const int idx = tid + 256 * q;
            int ii, rr;
            if (g.a_rfast) {
                rr = idx & (PD_TR_KC - 1);
                ii = idx / PD_TR_KC;
            } else {
                ii = idx & (PD_TR_TILE - 1);
                rr = idx / PD_TR_TILE;
            }
            const int gi = i0 + ii, gr = r0 + rr;
            As[rr * PD_TR_LD + ii] = (gi < g.I && gr < r_end) ? g.A[(long long)gi * g.a_rs + (long long)gr * g.a_cs] : 0.0f;
            int jj, rb;
            if (g.b_rfast) {
                rb = idx & (PD_TR_KC - 1);
                jj = idx / PD_TR_KC;
            } else {
                jj = idx & (PD_TR_TILE - 1);
                rb = idx / PD_TR_TILE;
            }
            const int gj = j0 + jj, gr2 = r0 + rb;
            Bs[rb * PD_TR_LD + jj] = (gj < g.J && gr2 < r_end) ? g.B[(long long)gr2 * g.b_rs + (long long)gj * g.b_cs] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < PD_TR_KC / 2; ++kk) {
            const float a = As[(2 * kk + hi) * PD_TR_LD + wi + l31];
            const float b = Bs[(2 * kk + hi) * PD_TR_LD + wj + l31];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    float *C = g.C + (long long)blockIdx.z * g.I * g.ldc;
    const int gj = j0 + wj + l31;
    if (gj >= g.J) return;
    const float bias = g.bias ? g.bias[gj] : 0.0f;
    PdTrRand rnd = {{0u, 0u, 0u, 0u}};
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int gi = i0 + wi + (q & 3) + 8 * (q >> 2) + 4 * hi;
        if constexpr (DROP) {
            if ((q & 3) == 0 && dr.philox) rnd = pd_tr_philox((unsigned int)gi >> 2, (unsigned int)gj, dr.ctr2, dr.step, dr.key0, dr.key1);
        }
        if (gi >= g.I) continue;
        float v = acc[q] + bias;
        if (g.relu) v = pd_relu(v);
        if (g.mask_mode == 1) {
            v = g.aux[(long long)gi * g.ldaux + gj] > 0.0f ? v : 0.0f;
        } else if (g.mask_mode == 2) {
            const float a = g.aux[(long long)gi * g.ldaux + gj];
            const float sg = 1.0f / (1.0f + expf(-a));
            v *= sg * (1.0f + a * (1.0f - sg));
        }
        if constexpr (DROP) {
            const bool keep = dr.philox ? rnd.w[q & 3] >= dr.thr : true;
            v = keep ? v * dr.scale : 0.0f;
        }
        if (g.resid) v += g.resid[(long long)gi * g.ldr + gj];
        C[(long long)gi * g.ldc + gj] = v;
    }
}

// out[e] = ws[0][e] + ws[1][e] + ... in slice order (the fixed order of every split reduction); T = float (weight-gradient partials) or
// double (column-sum partials).  ACC: the sum is ADDED to out (the backbone's gradients, accumulated over the scales of a call)
template <typename T, bool ACC>
__global__ __launch_bounds__(256) void pd_tr_reduce_kernel(const T *__restrict__ ws, long long total, int nz, float *__restrict__ out) {
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        T s = ws[e];
        for (int z = 1; z < nz; ++z) s += ws[(long long)z * total + e];
        if constexpr (ACC) out[e] += (float)s;
        else out[e] = (float)s;
    }
}

// out = in masked at one site (dropout backward of a residual sublayer's output): out[r][c] = keep(r, c) ? in[r][c] scale : 0 over
// [M, D]; a thread owns four consecutive rows of one column = one Philox call
__global__ __launch_bounds__(256) void pd_tr_dropmask_kernel(const float *__restrict__ in, float *__restrict__ out, int M, int D, PdTrDrop dr) {
    const long long total = (long long)((M + 3) / 4) * D;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int g4 = (int)(idx / D), c = (int)(idx - (long long)g4 * D);
        const PdTrRand rnd = pd_tr_philox((unsigned int)g4, (unsigned int)c, dr.ctr2, dr.step, dr.key0, dr.key1);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = 4 * g4 + k;
            if (r < M) out[(long long)r * D + c] = rnd.w[k] >= dr.thr ? in[(long long)r * D + c] * dr.scale : 0.0f;
        }
    }
}

// Column sums over a chunk of rows: bias gradients (LN = false: sum_m dy[m][c]) and LayerNorm's dgamma / dbeta (LN = true:
// sum_m dy[m][c] xhat[m][c] and sum_m dy[m][c], xhat from the stashed (mean, rstd)).  grid (ceil(C / 64), chunks), 256 threads: thread
// (c, rg) adds rows rg, rg + 4, ... of its chunk in order, the four row groups are added in order.  out_a / out_b: [chunks][C] slices.
// These sums of up to M addends per column cost nothing next to the GEMMs, so they are carried in double (addends and products are the
// fp32 values): a bias gradient whose addends are all +-g (l1 loss into _last.3.bias) then comes out correctly rounded, as torch's
// pairwise fp32 sum of equal magnitudes does -- plain fp32 chains were 1.9e-7 off there at 800 rows, 12 x the reference's own distance.
template <bool LN>
__global__ __launch_bounds__(256) void pd_tr_colsum_kernel(const float *__restrict__ dy, long long ldy, const float *__restrict__ x, long long ldx,
                                                           const float *__restrict__ stats, int M, int Ccols, int r_chunk,
                                                           double *__restrict__ out_a, double *__restrict__ out_b) {
    __shared__ double sa[4][64], sb[4][64];
    const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    const int r_begin = blockIdx.y * r_chunk, r_end = min(M, r_begin + r_chunk);
    double a = 0.0, b = 0.0;
    if (c < Ccols) {
        for (int r = r_begin + rg; r < r_end; r += 4) {
            const float v = dy[(long long)r * ldy + c];
            if constexpr (LN) {
                const float xh = (x[(long long)r * ldx + c] - stats[2 * r]) * stats[2 * r + 1];
                a += (double)v * (double)xh;
            }
            b += (double)v;
        }
    }
    sa[rg][cl] = a;
    sb[rg][cl] = b;
    __syncthreads();
    if (rg == 0 && c < Ccols) {
        if constexpr (LN) out_a[(long long)blockIdx.y * Ccols + c] = ((sa[0][cl] + sa[1][cl]) + sa[2][cl]) + sa[3][cl];
        out_b[(long long)blockIdx.y * Ccols + c] = ((sb[0][cl] + sb[1][cl]) + sb[2][cl]) + sb[3][cl];
    }
}

// --------------------------------------------------------------------------------------------
// forward pieces
// --------------------------------------------------------------------------------------------
// Frame counts (pd_trainer_set_frame_counts): nf is null on a uniform call, else nf[b] = the frames of sequence b, whose rows
// nf[b] .. n_frames - 1 of its n_frames-row block are padding.  The first kernels of the pass write +0 there INSTEAD OF reading the
// caller's rows, the tail writes +0 outputs and dl = 0, its backward takes gout = 0 by a select: every stashed value of a padding row is
// finite and every gradient row of a padding row is exactly zero, so it adds nothing to any sum over rows.
__device__ __forceinline__ bool pd_tr_is_padding(const int *__restrict__ nf, int m, int n_frames) {
    if (!nf) return false;
    const int b = m / n_frames;
    return m - b * n_frames >= nf[b];
}
// the counts as kernel arguments (count - 1 in a byte, PD_TR_NF_CHUNK per launch), as pd_engine_set_frame_counts sends them: ordered on the
// stream like any launch, no staging buffer that a later call could overwrite in flight
#define PD_TR_NF_CHUNK 1024
struct PdTrCountsChunk {
    unsigned w[PD_TR_NF_CHUNK / 4];
};
__global__ void pd_tr_set_counts_kernel(PdTrCountsChunk v, int first, int n, int *__restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[first + i] = (int)((v.w[i >> 2] >> (8 * (i & 3))) & 255u) + 1;
}
// the counts of a forward belong to its stash: copied at forward time, so that a later pd_trainer_set_frame_counts leaves the backward alone
__global__ void pd_tr_copy_counts_kernel(const int *__restrict__ src, int n, int *__restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// q_sample (gaussian_diffuser.py:211-216) in torch's own roundings, and the clamped timestep of every sequence (t_b[b])
__global__ void pd_tr_q_sample_kernel(const float *__restrict__ x_start, const float *__restrict__ noise, const int64_t *__restrict__ t_seq,
                                      const float *__restrict__ qa, const float *__restrict__ qb, const int *__restrict__ nf, int M, int n_frames,
                                      int timesteps, float *__restrict__ xt, int *__restrict__ t_b, unsigned int *err) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * 9) return;
    const int m = i / 9, b = m / n_frames;
    if (pd_tr_is_padding(nf, m, n_frames)) {            // (never row 0 of a sequence, which writes t_b below)
        xt[i] = 0.0f;
        return;
    }
    const long long tv = t_seq[b];
    int t = (int)tv;
    if (tv < 0 || tv >= timesteps) {
        atomicOr(err, PD_TR_ERR_T_RANGE);
        t = tv < 0 ? 0 : timesteps - 1;
    }
    if (i == b * n_frames * 9) t_b[b] = t;
    xt[i] = __fadd_rn(__fmul_rn(qa[t], x_start[i]), __fmul_rn(qb[t], noise[i]));
}

// TimeStepEmbedding.forward (util/embedding.py:28-37) of sequence b's timestep from the LIVE weights, one block of 128 threads per
// sequence, with what its backward needs: emb [B, 256] = [cos | sin], a0 [B, 128] = linear.0's output (the SiLU input),
// sact [B, 128] = SiLU(a0), temb [B, 128] = linear.2's output.  The expressions are those of the engine's time table.
__global__ __launch_bounds__(128) void pd_tr_time_kernel(const int *__restrict__ t_b, const float *__restrict__ w0, const float *__restrict__ b0,
                                                         const float *__restrict__ w2, const float *__restrict__ b2, float *__restrict__ emb_out,
                                                         float *__restrict__ a0_out, float *__restrict__ sact_out, float *__restrict__ temb_out) {
    __shared__ float emb[256];
    __shared__ float hid[128];
    const int i = threadIdx.x, b = blockIdx.x;
    const float t = (float)t_b[b];
    // freqs = exp(-ln(10000) arange(128, fp32) / 128) (embedding.py:24-26): the fp32 argument as torch forms it, its exponential correctly
    // rounded (through double) -- at t = 99 one ulp of a frequency is 6e-6 of the angle, and dW of linear.0 is proportional to cos / sin of it
    const float freq = (float)exp((double)((-9.210340371976184f * (float)i) / 128.0f));
    const float arg = t * freq;
    emb[i] = cosf(arg);
    emb[128 + i] = sinf(arg);
    __syncthreads();
    emb_out[(size_t)b * 256 + i] = emb[i];
    emb_out[(size_t)b * 256 + 128 + i] = emb[128 + i];
    float a = b0[i];
    for (int k = 0; k < 256; ++k) a = fmaf(emb[k], w0[i * 256 + k], a);
    const float sv = a / (1.0f + expf(-a));
    hid[i] = sv;
    a0_out[(size_t)b * 128 + i] = a;
    sact_out[(size_t)b * 128 + i] = sv;
    __syncthreads();
    float o = b2[i];
    for (int k = 0; k < 128; ++k) o = fmaf(hid[k], w2[i * 128 + k], o);
    temb_out[(size_t)b * 128 + i] = o;
}

// _first's input rows [M, Kf] in the reference's column order (models/denoiser.py:56-68), Kf = 317 + z + pivot, no padding:
//   [0,180) harmonic(x) | [180,189) x | [189,317) t_emb of the row's sequence | [317,317+z) z | pivot (frame 0 of a sequence)
__global__ __launch_bounds__(256) void pd_tr_embed_kernel(const float *__restrict__ x, const float *__restrict__ z, const float *__restrict__ temb,
                                                          const int *__restrict__ nf, int M, int n_frames, int zdim, int pivot, int Kf,
                                                          float *__restrict__ out) {
    const size_t total = (size_t)M * Kf;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % Kf);
        const int row = (int)(idx / Kf);
        float v = 0.0f;
        if (pd_tr_is_padding(nf, row, n_frames)) {
            // a padding row is +0 in every column: z is not read
        } else if (c < 180) {
            const int s = c / 90, rem = c - s * 90, d = rem / 10, kk = rem - d * 10;
            const float a = x[(size_t)row * 9 + d] * (float)(1 << kk);
            v = sinf(s ? a + 1.5707963267948966f : a);
        } else if (c < 189) {
            v = x[(size_t)row * 9 + (c - 180)];
        } else if (c < PD_TR_FIRST_FIXED) {
            v = temb[(size_t)(row / n_frames) * 128 + (c - 189)];
        } else if (c < PD_TR_FIRST_FIXED + zdim) {
            v = z[(size_t)row * zdim + (c - PD_TR_FIRST_FIXED)];
        } else {
            v = (pivot && row % n_frames == 0) ? 1.0f : 0.0f;
        }
        out[idx] = v;
    }
}

// LayerNorm over rows [M, D] with its affine (eps: the denoiser's 1e-5, DINO's 1e-6): one wave per row (the generic path's kernel), also
// writing stats[m] = (mean, rstd) when stats is not null
__global__ __launch_bounds__(256) void pd_tr_ln_kernel(const float *__restrict__ in, float *__restrict__ out, const float *__restrict__ gamma,
                                                       const float *__restrict__ beta, int M, int D, float eps, float *__restrict__ stats) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const float *src = in + (size_t)row * D;
    float mean, rstd;
    pd_wave_row_stats(src, D, lane, eps, &mean, &rstd);
    float *dst = out + (size_t)row * D;
    for (int c = lane; c < D; c += 64) dst[c] = (src[c] - mean) * rstd * gamma[c] + beta[c];
    if (stats && lane == 0) {
        stats[2 * (size_t)row] = mean;
        stats[2 * (size_t)row + 1] = rstd;
    }
}

// LayerNorm backward of one row per wave: g = dy gamma, dx = rstd (g - mean(g) - xhat mean(g xhat)), ADDED to dres (the gradient of the
// residual stream the LayerNorm read)
__global__ __launch_bounds__(256) void pd_tr_ln_bwd_kernel(const float *__restrict__ dy, const float *__restrict__ x, const float *__restrict__ stats,
                                                           const float *__restrict__ gamma, int M, int D, float *__restrict__ dres) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const float *xr = x + (size_t)row * D, *dr = dy + (size_t)row * D;
    const float mean = stats[2 * (size_t)row], rstd = stats[2 * (size_t)row + 1];
    float s1 = 0.0f, s2 = 0.0f;
    for (int c = lane; c < D; c += 64) {
        const float g = dr[c] * gamma[c], xh = (xr[c] - mean) * rstd;
        s1 += g;
        s2 = fmaf(g, xh, s2);
    }
    const float m1 = pd_wave_sum(s1) / (float)D, m2 = pd_wave_sum(s2) / (float)D;
    float *o = dres + (size_t)row * D;
    for (int c = lane; c < D; c += 64) {
        const float g = dr[c] * gamma[c], xh = (xr[c] - mean) * rstd;
        o[c] += rstd * (g - m1 - xh * m2);
    }
}

// --------------------------------------------------------------------------------------------
// attention, one workgroup per (sequence, head), N <= 64 frames, head dim hd (a multiple of 4, <= 128).  qkv rows [q (d) | k (d) | v (d)],
// head h at columns h hd ..; K and V of the head staged in LDS ([N][hd + 4] each).  pd_tr_attn_prob is THE expression of a softmax row,
// used by the forward and recomputed by the backward: lane j holds the probability of key j of query row qrow.
// --------------------------------------------------------------------------------------------
__device__ __forceinline__ float pd_tr_attn_prob(const float4 *__restrict__ qa, const float4 *kb, int hd4, float scale, int lane, int N) {
    float s = 0.0f;
    for (int d4 = 0; d4 < hd4; ++d4) {
        const float4 a = qa[d4], c = kb[d4];
        s = fmaf(a.x * scale, c.x, s);
        s = fmaf(a.y * scale, c.y, s);
        s = fmaf(a.z * scale, c.z, s);
        s = fmaf(a.w * scale, c.w, s);
    }
    const float sv = lane < N ? s : -INFINITY;
    const float mx = pd_wave_max(sv);
    const float e = lane < N ? expf(sv - mx) : 0.0f;
    return e * (1.0f / pd_wave_sum(e));
}

__device__ __forceinline__ void pd_tr_attn_stage_kv(const float *__restrict__ base, int N, int hd, int d, float *Kk, float *V) {
    const int LD = hd + 4, hd4 = hd / 4;
    const size_t ld3 = (size_t)3 * d;
    for (int idx = threadIdx.x; idx < N * hd4; idx += 256) {
        const int j = idx / hd4, d4 = idx - j * hd4;
        const float *row = base + (size_t)j * ld3 + 4 * d4;
        *(float4 *)(Kk + j * LD + 4 * d4) = *(const float4 *)(row + d);
        *(float4 *)(V + j * LD + 4 * d4) = *(const float4 *)(row + 2 * d);
    }
}

// DROP: site 0, the probability of (query row i, key j) is multiplied by keep scale before P V; mask row = (b nhead + h) N + i, column = j
template <bool DROP>
__global__ __launch_bounds__(256) void pd_tr_attn_kernel(const float *__restrict__ qkv, float *__restrict__ ctx, int N, int nhead, int hd, int d,
                                                         float scale, PdTrDrop dr) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int LD = hd + 4;
    float *Kk = lds, *V = lds + (size_t)N * LD;
    const int b = blockIdx.x / nhead, h = blockIdx.x % nhead, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t ld3 = (size_t)3 * d;
    const float *base = qkv + (size_t)b * N * ld3 + (size_t)h * hd;
    pd_tr_attn_stage_kv(base, N, hd, d, Kk, V);
    __syncthreads();
    const int jj = lane < N ? lane : N - 1;
    const float4 *kb = (const float4 *)(Kk + jj * LD);
    for (int i = wave; i < N; i += 4) {
        float p = pd_tr_attn_prob((const float4 *)(base + (size_t)i * ld3), kb, hd / 4, scale, lane, N);
        if constexpr (DROP) p = pd_tr_keep(dr, (unsigned int)(blockIdx.x * N + i), (unsigned int)lane) ? p * dr.scale : 0.0f;
        float o[2] = {0.0f, 0.0f};
        for (int j = 0; j < N; ++j) {
            const float pj = __shfl(p, j, 64);
            const float *vr = V + j * LD;
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const int dd = lane + 64 * cc;
                if (dd < hd) o[cc] = fmaf(pj, vr[dd], o[cc]);
            }
        }
        float *out = ctx + (size_t)(b * N + i) * d + (size_t)h * hd;
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            const int dd = lane + 64 * cc;
            if (dd < hd) out[dd] = o[cc];
        }
    }
}
static inline size_t pd_tr_attn_lds(int N, int hd) { return (size_t)2 * N * (hd + 4) * sizeof(float); }

// Attention backward.  Phase 1, wave w owns query rows w, w + 4, ...: P row recomputed, dP_ij = dO_i . V_j, dS_ij = P_ij (dP_ij -
// sum_j dP_ij P_ij), both rows kept in LDS, dQ_i = scale sum_j dS_ij K_j.  Phase 2, wave w owns key rows: dV_j = sum_i P_ij dO_i,
// dK_j = scale sum_i dS_ij Q_i, the sums over the query rows in row order.  At N = 1: P = 1 and dS = 1 (dP - dP) = 0 exactly.
// DROP (site 0), with ks = keep scale of the element and P~ = P ks what the forward multiplied into V: dP = (dO . V) ks, dS from the
// UNMASKED P as above, and the LDS P rows that phase 2 reads hold P~ (dV = P~^T dO).  At N = 1 dS is still 1 (dP - dP) = 0.
template <bool DROP>
__global__ __launch_bounds__(256) void pd_tr_attn_bwd_kernel(const float *__restrict__ qkv, const float *__restrict__ dctx, float *__restrict__ dqkv,
                                                             int N, int nhead, int hd, int d, float scale, PdTrDrop dr) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int LD = hd + 4, PL = N + 1;
    float *Kk = lds, *V = lds + (size_t)N * LD, *P = V + (size_t)N * LD, *dS = P + (size_t)N * PL;
    const int b = blockIdx.x / nhead, h = blockIdx.x % nhead, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t ld3 = (size_t)3 * d;
    const float *base = qkv + (size_t)b * N * ld3 + (size_t)h * hd;
    const float *dO = dctx + (size_t)b * N * d + (size_t)h * hd;
    float *dbase = dqkv + (size_t)b * N * ld3 + (size_t)h * hd;
    pd_tr_attn_stage_kv(base, N, hd, d, Kk, V);
    __syncthreads();
    const int jj = lane < N ? lane : N - 1, hd4 = hd / 4;
    const float4 *kb = (const float4 *)(Kk + jj * LD), *vb = (const float4 *)(V + jj * LD);
    for (int i = wave; i < N; i += 4) {
        const float p = pd_tr_attn_prob((const float4 *)(base + (size_t)i * ld3), kb, hd4, scale, lane, N);
        const float4 *go = (const float4 *)(dO + (size_t)i * d);
        float dp = 0.0f;
        for (int d4 = 0; d4 < hd4; ++d4) {
            const float4 a = go[d4], c = vb[d4];
            dp = fmaf(a.x, c.x, dp);
            dp = fmaf(a.y, c.y, dp);
            dp = fmaf(a.z, c.z, dp);
            dp = fmaf(a.w, c.w, dp);
        }
        dp = lane < N ? dp : 0.0f;
        float pt = p;
        if constexpr (DROP) {
            // selects, not products with (keep ? scale : 0): a product feeding dp - rs below is contracted into an fma whose result at
            // N = 1 is the product's rounding error instead of 0
            const bool keep = pd_tr_keep(dr, (unsigned int)(blockIdx.x * N + i), (unsigned int)lane);
            dp = keep ? dp * dr.scale : 0.0f;
            pt = keep ? p * dr.scale : 0.0f;
        }
        const float rs = pd_wave_sum(dp * p);
        const float ds = p * (dp - rs);
        if (lane < N) {
            P[i * PL + lane] = pt;
            dS[i * PL + lane] = ds;
        }
        float o[2] = {0.0f, 0.0f};
        for (int j = 0; j < N; ++j) {
            const float dj = __shfl(ds, j, 64);
            const float *kr = Kk + j * LD;
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const int dd = lane + 64 * cc;
                if (dd < hd) o[cc] = fmaf(dj, kr[dd], o[cc]);
            }
        }
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            const int dd = lane + 64 * cc;
            if (dd < hd) dbase[(size_t)i * ld3 + dd] = scale * o[cc];
        }
    }
    __syncthreads();
    for (int j = wave; j < N; j += 4) {
        float dk[2] = {0.0f, 0.0f}, dv[2] = {0.0f, 0.0f};
        for (int i = 0; i < N; ++i) {
            const float pij = P[i * PL + j], dsij = dS[i * PL + j];
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const int dd = lane + 64 * cc;
                if (dd < hd) {
                    dv[cc] = fmaf(pij, dO[(size_t)i * d + dd], dv[cc]);
                    dk[cc] = fmaf(dsij, base[(size_t)i * ld3 + dd], dk[cc]);
                }
            }
        }
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            const int dd = lane + 64 * cc;
            if (dd < hd) {
                dbase[(size_t)j * ld3 + d + dd] = scale * dk[cc];
                dbase[(size_t)j * ld3 + 2 * d + dd] = dv[cc];
            }
        }
    }
}
static inline size_t pd_tr_attn_bwd_lds(int N, int hd) { return ((size_t)2 * N * (hd + 4) + (size_t)2 * N * (N + 1)) * sizeof(float); }

// the same attention for up to 256 frames, K and V through LDS in tiles of 64 keys (PD_TR_OPT_MAX_FRAMES): pd_tr_lattn_* kernels
#include "pd_train_lattn.h"

// --------------------------------------------------------------------------------------------
// tail: LayerNorm(hidden) -> ReLU -> Linear(hidden, 9) (_last.1 .. 3) and the outputs of p_losses (gaussian_diffuser.py:312-327), one
// wave per token row, lane l holds hidden values l, l + 64, ... (hidden <= 1024).  Stash: stats (mean, rstd), the post-ReLU hidden row,
// and dl [M, 9] = d loss / d model_out (sign(d) with sign(0) = 0 for l1, 2 d for l2)
// --------------------------------------------------------------------------------------------
struct PdTrTail {
    const float *hid;               // [M, H] = _last.0 output
    const float *lnw, *lnb, *w3, *b3;
    const float *xt, *target;       // [M, 9]
    const int *t_b;                 // [B]
    const int *nf;                  // [B] frame counts, or null (uniform)
    const float *c_recip, *c_recipm1;   // [timesteps] or null (x0_out then stays unwritten under pred_noise)
    float *loss_out, *x0_out, *model_out;   // [M, 9]; x0_out / model_out may be null
    float *stats, *hid_post, *dl;
    int M, H, n_frames, pred_x0, loss_type;
};
__global__ __launch_bounds__(256) void pd_tr_tail_kernel(PdTrTail g) {
    const int lane = threadIdx.x & 63, m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= g.M) return;
    const float *row = g.hid + (size_t)m * g.H;
    float v[PD_TR_TAIL_PER];
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < PD_TR_TAIL_PER; ++i) {
        const int c = lane + 64 * i;
        v[i] = c < g.H ? row[c] : 0.0f;
        s += v[i];
    }
    const float mean = pd_wave_sum(s) / (float)g.H;
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < PD_TR_TAIL_PER; ++i) {
        const float e = lane + 64 * i < g.H ? v[i] - mean : 0.0f;
        q = fmaf(e, e, q);
    }
    const float rstd = 1.0f / sqrtf(pd_wave_sum(q) / (float)g.H + 1e-5f);
    if (lane == 0) {
        g.stats[2 * (size_t)m] = mean;
        g.stats[2 * (size_t)m + 1] = rstd;
    }
#pragma unroll
    for (int i = 0; i < PD_TR_TAIL_PER; ++i) {
        const int c = lane + 64 * i;
        v[i] = c < g.H ? pd_relu((v[i] - mean) * rstd * g.lnw[c] + g.lnb[c]) : 0.0f;
        if (c < g.H) g.hid_post[(size_t)m * g.H + c] = v[i];
    }
    float e = 0.0f;
#pragma unroll 1
    for (int o = 0; o < 9; ++o) {
        float part = 0.0f;
#pragma unroll
        for (int i = 0; i < PD_TR_TAIL_PER; ++i)       // v is 0 beyond H: a clamped column needs no predicate
            part = fmaf(v[i], g.w3[(size_t)o * g.H + min(lane + 64 * i, g.H - 1)], part);
        part = pd_wave_sum(part);
        e = (lane == o) ? part : e;
    }
    if (lane < 9) {
        const size_t at = (size_t)m * 9 + lane;
        if (pd_tr_is_padding(g.nf, m, g.n_frames)) {   // +0 outputs, no loss derivative; the target row is not read
            if (g.model_out) g.model_out[at] = 0.0f;
            if (g.x0_out && (g.pred_x0 || g.c_recip)) g.x0_out[at] = 0.0f;
            g.loss_out[at] = 0.0f;
            g.dl[at] = 0.0f;
            return;
        }
        e += g.b3[lane];
        if (g.model_out) g.model_out[at] = e;
        if (g.x0_out) {
            if (g.pred_x0) {
                g.x0_out[at] = e;
            } else if (g.c_recip) {
                const int t = g.t_b[m / g.n_frames];
                g.x0_out[at] = g.c_recip[t] * g.xt[at] - g.c_recipm1[t] * e;                   // :316
            }
        }
        const float d = e - g.target[at];
        g.loss_out[at] = g.loss_type == 2 ? d * d : fabsf(d);                                  // :323, reduction "none"
        g.dl[at] = g.loss_type == 2 ? 2.0f * d : (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f));
    }
}

// tail backward of one row per wave: gout -> _last.3 -> ReLU mask (stashed post-ReLU values) = dy -> LayerNorm(hidden) backward = dhid.
// gout = the sum of the upstream terms that are PRESENT (pd_train_backward_ex), in this order: g_loss dl, g_mo, k_b g_x0 with k_b = 1
// under pred_x0 and -sqrt_recipm1_alphas_cumprod[t_b] under pred_noise (x_0_pred = c_recip x_t - c_recipm1 model_out, :316).  An absent
// term is not added: one term alone is that single fp32 product (the plain value for g_mo, and for g_x0 under pred_x0), and the sums are
// separate roundings, never contracted with a product.  gout [M, 9], dy [M, H] (LayerNorm's dgamma / dbeta, _last.3's weight gradient)
// and dhid [M, H] are written.
struct PdTrTailBwd {
    const float *g_loss, *dl, *w3, *lnw, *hid, *hid_post, *stats;
    const float *g_mo, *g_x0;       // [M, 9] upstreams of model_out and x_0_pred; each of the three may be null (not all)
    const float *c_recipm1;         // [timesteps]; read only for g_x0 under pred_noise
    const int *t_b;                 // [B] the forward's clamped timesteps
    const int *nf;                  // [B] frame counts of the forward, or null (uniform)
    float *gout, *dy, *dhid;
    int M, H, n_frames, pred_x0;
};
__global__ __launch_bounds__(256) void pd_tr_tail_bwd_kernel(PdTrTailBwd g) {
    const int lane = threadIdx.x & 63, m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= g.M) return;
    float gv = 0.0f;
    if (lane < 9) {
        // a padding row's upstreams are not read (a product with the stashed dl = 0 would pass a NaN on)
        if (!pd_tr_is_padding(g.nf, m, g.n_frames)) {
            const size_t at = (size_t)m * 9 + lane;
            bool have = false;
            if (g.g_loss) {
                gv = __fmul_rn(g.g_loss[at], g.dl[at]);
                have = true;
            }
            if (g.g_mo) {
                const float v = g.g_mo[at];
                gv = have ? __fadd_rn(gv, v) : v;
                have = true;
            }
            if (g.g_x0) {
                const float v = g.pred_x0 ? g.g_x0[at] : __fmul_rn(-g.c_recipm1[g.t_b[m / g.n_frames]], g.g_x0[at]);
                gv = have ? __fadd_rn(gv, v) : v;
            }
        }
        g.gout[(size_t)m * 9 + lane] = gv;
    }
    const float mean = g.stats[2 * (size_t)m], rstd = g.stats[2 * (size_t)m + 1];
    float gg[PD_TR_TAIL_PER], xh[PD_TR_TAIL_PER];
#pragma unroll
    for (int i = 0; i < PD_TR_TAIL_PER; ++i) gg[i] = 0.0f;
    for (int o = 0; o < 9; ++o) {
        const float go = __shfl(gv, o, 64);
#pragma unroll
        for (int i = 0; i < PD_TR_TAIL_PER; ++i) {
            const int c = lane + 64 * i;
            if (c < g.H) gg[i] = fmaf(go, g.w3[(size_t)o * g.H + c], gg[i]);
        }
    }
    float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int i = 0; i < PD_TR_TAIL_PER; ++i) {
        const int c = lane + 64 * i;
        xh[i] = 0.0f;
        if (c < g.H) {
            const size_t at = (size_t)m * g.H + c;
            const float dyv = g.hid_post[at] > 0.0f ? gg[i] : 0.0f;
            g.dy[at] = dyv;
            xh[i] = (g.hid[at] - mean) * rstd;
            gg[i] = dyv * g.lnw[c];
            s1 += gg[i];
            s2 = fmaf(gg[i], xh[i], s2);
        } else {
            gg[i] = 0.0f;
        }
    }
    const float m1 = pd_wave_sum(s1) / (float)g.H, m2 = pd_wave_sum(s2) / (float)g.H;
#pragma unroll
    for (int i = 0; i < PD_TR_TAIL_PER; ++i) {
        const int c = lane + 64 * i;
        if (c < g.H) g.dhid[(size_t)m * g.H + c] = rstd * (gg[i] - m1 - xh[i] * m2);
    }
}

// the t_emb columns' gradient summed over a sequence's N rows in row order: dtemb[b][c] = sum_n demb[(b N + n)][c], c < 128
__global__ __launch_bounds__(128) void pd_tr_tsum_kernel(const float *__restrict__ demb, int n_frames, float *__restrict__ dtemb) {
    const int b = blockIdx.x, c = threadIdx.x;
    float s = 0.0f;
    for (int n = 0; n < n_frames; ++n) s += demb[((size_t)b * n_frames + n) * 128 + c];
    dtemb[(size_t)b * 128 + c] = s;
}
