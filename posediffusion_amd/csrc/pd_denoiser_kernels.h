// pd_denoiser_kernels.h -- the default-shape denoiser's kernels that are neither GEMM nor attention: _first's step rows and creation-time
// pieces, the time-step and pose embeddings, the fused tail of the head, and the fp16-subnormal probe.
#pragma once
#include "pd_gemm_small.h"      // PD_STAMP
#include "pd_gemm_stream.h"     // f16x8

// _first's STEP rows for the streamed path (>= PD_STREAM_MIN_ROWS token rows): [harmonic(x) (180) | x (9) | pivot | 0 0] = KFIRST_D
// columns (piece PD_FIRST_D of pd_denoiser_dev.h), one wave per row, written once per step and read by pd_gemm_dma like any activation
// (denoiser.py:60-68; the same expressions as the AMODE 2 staging of the small-batch pd_gemm_kernel).  z and t_emb never enter the loop: their products
// are hoisted (pd_denoiser_prepare, pd_first_ttab_kernel).
__global__ __launch_bounds__(256) void pd_embed_rows_kernel(const float *__restrict__ x, int n_frames, int M, float *__restrict__ out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    float4 *dst = (float4 *)(out + (size_t)row * KFIRST_D);
    float xv[9];
#pragma unroll
    for (int d = 0; d < 9; ++d) xv[d] = x[(size_t)row * 9 + d];
    if (lane < 45) {                                            // harmonic: 180 values = 45 float4 at [0, 45)
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int idx = 4 * lane + e, s = idx / 90, rem = idx - s * 90, d = rem / 10, kk = rem - d * 10;
            float xd = xv[0];
#pragma unroll
            for (int q = 1; q < 9; ++q) xd = (d == q) ? xv[q] : xd;
            const float a = xd * (float)(1 << kk);
            o[e] = sinf(s ? a + 1.5707963267948966f : a);
        }
        dst[lane] = make_float4(o[0], o[1], o[2], o[3]);
    } else if (lane == 45) {
        dst[45] = make_float4(xv[0], xv[1], xv[2], xv[3]);
    } else if (lane == 46) {
        dst[46] = make_float4(xv[4], xv[5], xv[6], xv[7]);
    } else if (lane == 47) {
        dst[47] = make_float4(xv[8], (row % n_frames == 0) ? 1.0f : 0.0f, 0.0f, 0.0f);   // pivot one-hot on frame 0, padding
    }
}
// a piece of W_first [512, 702] -> row-major [512, Kdst] in the engine's column order of that piece (pd_first_col)
__global__ void pd_first_rowmajor_kernel(const float *__restrict__ W, float *__restrict__ Wf, int piece, int Kdst) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= DM * Kdst) return;
    const int n = idx / Kdst, k = pd_first_col(piece, idx - n * Kdst);
    Wf[idx] = k < KFIRST ? W[(size_t)n * KFIRST + k] : 0.0f;
}
// the time piece of _first: ttab[t][n] = sum_k W_first[n][189 + k] t_emb(t)[k], an fmaf chain over the 128 columns (one block per t)
__global__ __launch_bounds__(DM) void pd_first_ttab_kernel(const float *__restrict__ W, const float *__restrict__ t_table, float *__restrict__ ttab) {
    __shared__ float te[128];
    const int t = blockIdx.x, n = threadIdx.x;
    if (n < 128) te[n] = t_table[(size_t)t * 128 + n];
    __syncthreads();
    const float *w = W + (size_t)n * KFIRST + pd_first_col(PD_FIRST_T, 0);
    float a = 0.0f;
    for (int k = 0; k < 128; ++k) a = fmaf(te[k], w[k], a);
    ttab[(size_t)t * DM + n] = a;
}

// time-step embedding (util/embedding.py:28-37) of one timestep value t: 128 threads, thread i owns output i
__device__ __forceinline__ float pd_time_embed_one(float t, const float *__restrict__ w0, const float *__restrict__ b0,
                                                   const float *__restrict__ w2, const float *__restrict__ b2, float *emb, float *hid) {
    const int i = threadIdx.x;
    // freqs = exp(-ln(10000) * arange(128, fp32) / 128)  (embedding.py:24-26), args = t * freqs
    const float freq = expf((-9.210340371976184f * (float)i) / 128.0f);
    const float arg = t * freq;
    emb[i] = cosf(arg);
    emb[128 + i] = sinf(arg);
    __syncthreads();
    float a = b0[i];
    for (int k = 0; k < 256; ++k) a = fmaf(emb[k], w0[i * 256 + k], a);
    hid[i] = a / (1.0f + expf(-a));   // SiLU
    __syncthreads();
    float o = b2[i];
    for (int k = 0; k < 128; ++k) o = fmaf(hid[k], w2[i * 128 + k], o);
    return o;
}
// the engine's table: one block per step t = 0 .. T-1
__global__ void pd_time_table_kernel(const float *__restrict__ w0, const float *__restrict__ b0, const float *__restrict__ w2,
                                     const float *__restrict__ b2, float *__restrict__ table) {
    __shared__ float emb[256];
    __shared__ float hid[128];
    table[blockIdx.x * 128 + threadIdx.x] = pd_time_embed_one((float)blockIdx.x, w0, b0, w2, b2, emb, hid);
}
// TimeStepEmbedding.forward for arbitrary timesteps (pd_time_embedding): the same arithmetic, one block per entry of tvals
__global__ void pd_time_embed_kernel(const float *__restrict__ tvals, const float *__restrict__ w0, const float *__restrict__ b0,
                                     const float *__restrict__ w2, const float *__restrict__ b2, float *__restrict__ out) {
    __shared__ float emb[256];
    __shared__ float hid[128];
    out[(size_t)blockIdx.x * 128 + threadIdx.x] = pd_time_embed_one(tvals[blockIdx.x], w0, b0, w2, b2, emb, hid);
}
// PoseEmbedding.forward = pytorch3d HarmonicEmbedding(n = 10, append_input = True) of rows [rows, dim] (pd_pose_embedding):
// out [rows, 21 dim] = [sin(x_d 2^k) (d-major, k = 0..9) | sin(x_d 2^k + pi / 2) | x] -- the expressions of pd_embed_rows_kernel and
// of the AMODE 2 staging, in the reference's own column order
__global__ void pd_harmonic_rows_kernel(const float *__restrict__ x, long long rows, int dim, float *__restrict__ out) {
    const int per = 21 * dim;
    const long long total = rows * per;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long row = idx / per;
        const int c = (int)(idx - row * per);
        float v;
        if (c >= 20 * dim) {
            v = x[row * dim + (c - 20 * dim)];
        } else {
            const int s = c / (10 * dim), rem = c - s * 10 * dim, d = rem / 10, kk = rem - d * 10;
            const float a = x[row * dim + d] * (float)(1 << kk);
            v = sinf(s ? a + 1.5707963267948966f : a);
        }
        out[idx] = v;
    }
}

// --------------------------------------------------------------------------------------------
// tail of the head: LayerNorm(128) -> ReLU -> Linear(128 -> 9) (denoiser.py:51,74 `_last.1..3`)
// fused with predict_start_from_noise / q_posterior / the sample update
// (gaussian_diffuser.py:190-209, :280).  One wave per token; lane holds 2 of the 128 hidden values.
// --------------------------------------------------------------------------------------------
struct HeadArgs {
    const float *hid;      // [M, 128] = _last.0 output (bias included)
    const float *lnw, *lnb, *w3, *b3;
    const float *x;        // [M, 9] current sample
    const float *noise;    // [M, 9] or null
    float *eps_out, *mean_out, *x0_out, *xnext_out;   // each [M, 9] or null
    float c_recip, c_recipm1, coef1, coef2, sigma;
    int M;
    int pred_x0;           // objective "pred_x0": the model output is x_start (gaussian_diffuser.py:225-227)
#ifdef PD_DEN_STAMPS
    long long *stamps;
#endif
};

__global__ __launch_bounds__(256) void pd_tail_kernel(HeadArgs g) {
#ifdef PD_DEN_STAMPS
    long long *const stamps = g.stamps;
#endif
    PD_STAMP(stamps, 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = blockIdx.x * 4 + wave;
    if (m >= g.M) return;
    const float *row = g.hid + (size_t)m * HID;
    const float v0 = row[lane], v1 = row[64 + lane];
    // everything the last nine lanes add at the end is requested now (clamped lane: no predicated loads), not behind the reductions
    const int l9 = lane < 9 ? lane : 8;
    const size_t at = (size_t)m * 9 + l9;
    const float b3v = g.b3[l9], xv = g.x[at], nz = g.noise ? g.noise[at] : 0.0f;
    const float mean = pd_wave_sum(v0 + v1) * (1.0f / HID);
    const float d0 = v0 - mean, d1 = v1 - mean;
    const float rstd = 1.0f / sqrtf(pd_wave_sum(d0 * d0 + d1 * d1) * (1.0f / HID) + 1e-5f);
    const float a0 = pd_relu(d0 * rstd * g.lnw[lane] + g.lnb[lane]);
    const float a1 = pd_relu(d1 * rstd * g.lnw[64 + lane] + g.lnb[64 + lane]);
    float e = 0.0f;
#pragma unroll
    for (int o = 0; o < 9; ++o) {
        const float part = pd_wave_sum(fmaf(a0, g.w3[o * HID + lane], a1 * g.w3[o * HID + 64 + lane]));
        e = (lane == o) ? part : e;
    }
    if (lane < 9) {
        e += b3v;
        const float x0 = g.pred_x0 ? e : g.c_recip * xv - g.c_recipm1 * e;   // gaussian_diffuser.py:190-194, :221-227
        const float mu = g.coef1 * x0 + g.coef2 * xv;               // :201-205
        if (g.eps_out) g.eps_out[at] = e;
        if (g.x0_out) g.x0_out[at] = x0;
        if (g.mean_out) g.mean_out[at] = mu;
        if (g.xnext_out) g.xnext_out[at] = g.noise ? mu + g.sigma * nz : mu;   // :280
    }
    PD_STAMP(stamps, 5);
    PD_STAMP_DRAIN();
    PD_STAMP(stamps, 6);
}

// ---- probe: fp16-subnormal operands on the fp16 matrix pipe (pd_engine.h pd_debug_mfma_f16_subnormal) ----------------------------
__global__ __launch_bounds__(64) void pd_mfma_f16_subnormal_kernel(float *out) {
    const float av[4] = {9.5367431640625e-07f, 1024.0f, 9.5367431640625e-07f, 1.0f};      // 2^-20 is an fp16 subnormal (min normal 2^-14)
    const float bv[4] = {1024.0f, 9.5367431640625e-07f, 0.0625f, 1.0f};
    for (int c = 0; c < 4; ++c) {
        f16x8 a, b;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            a[e] = (_Float16)av[c];
            b[e] = (_Float16)bv[c];
        }
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
        if (threadIdx.x == 0) {
            out[c] = acc[0];
            out[4 + c] = (float)a[0];       // what the conversion itself kept of the operand
        }
    }
}
