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
    const int *nf;         // frame counts per sequence (pd_engine_set_frame_counts) or null: row m is padding when m % n_frames >= nf[m / n_frames]
    int n_frames;          //   rows per sequence block
#ifdef PD_DEN_STAMPS
    long long *stamps;
#endif
};

// LayerNorm(128) -> ReLU -> Linear(128 -> 9) of token row m, shared by the two tail kernels: lane o < 9 returns output o WITHOUT its bias
__device__ __forceinline__ float pd_tail_project(const HeadArgs &g, int m, int lane) {
    const float *row = g.hid + (size_t)m * HID;
    const float v0 = row[lane], v1 = row[64 + lane];
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
    return e;
}

__global__ __launch_bounds__(256) void pd_tail_kernel(HeadArgs g) {
#ifdef PD_DEN_STAMPS
    long long *const stamps = g.stamps;
#endif
    PD_STAMP(stamps, 0);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = blockIdx.x * 4 + wave;
    if (m >= g.M) return;
    // everything the last nine lanes add at the end is requested now (clamped lane: no predicated loads), not behind the reductions
    const int l9 = lane < 9 ? lane : 8;
    const size_t at = (size_t)m * 9 + l9;
    if (g.nf) {            // a padding row (wave-uniform): every output gets +0, nothing of the row is read
        const int sb = m / g.n_frames;
        if (m - sb * g.n_frames >= g.nf[sb]) {
            if (lane < 9) {
                if (g.eps_out) g.eps_out[at] = 0.0f;
                if (g.x0_out) g.x0_out[at] = 0.0f;
                if (g.mean_out) g.mean_out[at] = 0.0f;
                if (g.xnext_out) g.xnext_out[at] = 0.0f;
            }
            return;
        }
    }
    const float b3v = g.b3[l9], xv = g.x[at], nz = g.noise ? g.noise[at] : 0.0f;
    float e = pd_tail_project(g, m, lane);
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

// --------------------------------------------------------------------------------------------
// one timestep per sequence (pd_denoise_step_t, pd_p_losses; gaussian_diffuser.py:308-332)
// --------------------------------------------------------------------------------------------
#define PD_ASYNC_ERR_T_RANGE 8u     // bit 3 of the asynchronous error word: an entry of t_seq outside [0, timesteps)
// t_seq[b] clamped into [0, timesteps): nothing downstream indexes a table out of bounds; a clamped entry raises the error word
__device__ __forceinline__ int pd_t_checked(const int64_t *__restrict__ t_seq, int b, int timesteps, unsigned int *err) {
    const long long tv = t_seq[b];
    if (tv >= 0 && tv < timesteps) return (int)tv;
    atomicOr(err, PD_ASYNC_ERR_T_RANGE);
    return tv < 0 ? 0 : timesteps - 1;
}
// t_row[m] = t_seq[m / n_frames]: the per-row index that _first and the tail read (pd_denoise_step_t's pre-pass)
__global__ void pd_t_rows_kernel(const int64_t *__restrict__ t_seq, int M, int n_frames, int timesteps, int *__restrict__ t_row,
                                 unsigned int *err) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m < M) t_row[m] = pd_t_checked(t_seq, m / n_frames, timesteps, err);
}
// q_sample (gaussian_diffuser.py:211-216): x_t = sqrt_alphas_cumprod[t] x_start + sqrt_one_minus_alphas_cumprod[t] noise over the
// M * 9 values, in torch's own roundings (two products, one sum: no fused multiply-add); the element of column 0 also writes t_row[m]
__global__ void pd_q_sample_kernel(const float *__restrict__ x_start, const float *__restrict__ noise, const int64_t *__restrict__ t_seq,
                                   const float *__restrict__ qa, const float *__restrict__ qb, int M, int n_frames, int timesteps,
                                   float *__restrict__ xt, int *__restrict__ t_row, unsigned int *err) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * 9) return;
    const int m = i / 9;
    const int t = pd_t_checked(t_seq, m / n_frames, timesteps, err);
    if (i - m * 9 == 0) t_row[m] = t;
    xt[i] = __fadd_rn(__fmul_rn(qa[t], x_start[i]), __fmul_rn(qb[t], noise[i]));
}
// pd_tail_kernel with the schedule coefficients of every row's own timestep (device tables) and the outputs of p_losses (:312-327):
// eps_out = the model output, x0_out = x_0_pred, loss_out = |model_out - target| (loss_type 1) or its square (2), each may be null
struct HeadArgsT {
    HeadArgs h;                           // hid .. b3, x (= x_t), eps_out, x0_out, M, pred_x0; the posterior fields are not read
    const int *t_row;                     // [M]
    const float *c_recip, *c_recipm1;     // [timesteps] sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod
    const float *target;                  // [M, 9] noise (pred_noise) or x_start (pred_x0); null without loss_out
    float *loss_out;
    int loss_type;
};
__global__ __launch_bounds__(256) void pd_tail_t_kernel(HeadArgsT a) {
    const HeadArgs &g = a.h;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = blockIdx.x * 4 + wave;
    if (m >= g.M) return;
    const int l9 = lane < 9 ? lane : 8;
    const size_t at = (size_t)m * 9 + l9;
    const int t = a.t_row[m];
    const float b3v = g.b3[l9], xv = g.x[at], tg = a.loss_out ? a.target[at] : 0.0f, cr = a.c_recip[t], crm1 = a.c_recipm1[t];
    float e = pd_tail_project(g, m, lane);
    if (lane < 9) {
        e += b3v;
        if (g.eps_out) g.eps_out[at] = e;
        if (g.x0_out) g.x0_out[at] = g.pred_x0 ? e : cr * xv - crm1 * e;     // gaussian_diffuser.py:316, :319
        if (a.loss_out) {
            const float d = e - tg;
            a.loss_out[at] = a.loss_type == 2 ? d * d : fabsf(d);               // F.mse_loss / F.l1_loss, reduction "none" (:323)
        }
    }
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
// the same four products on v_mfma_f32_16x16x32_f16 (the large-batch planes' shape): 32 k per instruction
__global__ __launch_bounds__(64) void pd_mfma16_f16_subnormal_kernel(float *out) {
    const float av[4] = {9.5367431640625e-07f, 1024.0f, 9.5367431640625e-07f, 1.0f};
    const float bv[4] = {1024.0f, 9.5367431640625e-07f, 0.0625f, 1.0f};
    for (int c = 0; c < 4; ++c) {
        f16x8 a, b;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            a[e] = (_Float16)av[c];
            b[e] = (_Float16)bv[c];
        }
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0);
        if (threadIdx.x == 0) {
            out[c] = acc[0];
            out[4 + c] = (float)a[0];
        }
    }
}
