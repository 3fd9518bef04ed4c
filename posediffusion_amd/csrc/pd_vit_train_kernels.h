// pd_vit_train_kernels.h -- the device code of the backbone trainer (pd_vit_train.hip; include/pd_engine_vit_train.h)
// that the denoiser trainer's header lacks.  Every matrix product, LayerNorm and its backward, the column sums, the split reductions and
// the key-tiled attention are pd_train_kernels.h's kernels, compiled once in pd_train.hip and launched through pd_train_launch.h's helpers;
// the kernels here are the ViT's own pieces:
//   pd_vt_im2col_kernel         normalise + bilinear rescale (vit_prep_kernel's arithmetic) straight into patch rows [n P, 768]
//   pd_vt_assemble_kernel       x0[img, 0] = cls + pos[0], x0[img, 1 + p] = patch_out + pos[1 + p]; pd_vt_assemble_bwd_kernel its adjoint
//   pd_vt_gelu_kernel / _bwd    nn.GELU() in its exact erf form from the stashed pre-activation; dy (Phi(a) + a phi(a))
//   pd_vt_final_kernel / _bwd / _param   the final LayerNorm of the CLS rows, the average over the scales, and their backward
//   pd_vt_posgrid_kernel        d pos_embed / d cls_token from one scale's per-token position gradient: the adjoint of the bicubic resampling
// No float atomics; every sum has a fixed order that depends on the shapes of the call alone.
#pragma once
#include "pd_denoiser_dev.h"
#include "pd_train_launch.h"

#include <math.h>
#include <stddef.h>

#define PD_VT_PATCH 16
#define PD_VT_KP 768                // 3 x 16 x 16: the columns of a patch row, k = c 256 + ky 16 + kx
#define PD_VT_MAX_TOKENS 256        // the key-tiled attention's limit
static_assert(PD_VT_MAX_TOKENS == PD_TR_LA_MAX_N, "the tokens of an image are the keys of pd_tr_lattn_*");

// Patch rows of the prepared images: (image - mean) / std (image_feature_extractor.py:62-63), F.interpolate(scale_factor, bilinear,
// align_corners=False) (:86-87; identity: skipped) in the expressions of vit_prep_kernel, written as row (image, patch), column k.
// Pixels of the rescaled image beyond the last whole patch are never read, as the convolution never reads them.
__global__ __launch_bounds__(256) void pd_vt_im2col_kernel(const float *__restrict__ in, int n, int H, int W, int gh, int gw, float inv_sf,
                                                           int identity, float *__restrict__ out) {
    const int P = gh * gw;
    const size_t total = (size_t)n * P * PD_VT_KP;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int k = (int)(idx % PD_VT_KP);
        const size_t row = idx / PD_VT_KP;
        const int im = (int)(row / P), p = (int)(row - (size_t)im * P), py = p / gw, px = p - py * gw;
        const int c = k >> 8, ky = (k >> 4) & 15, kx = k & 15;
        const int oy = py * PD_VT_PATCH + ky, ox = px * PD_VT_PATCH + kx;
        const float mean = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f), sd = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
        const float *src = in + ((size_t)im * 3 + c) * (size_t)H * W;
        float v;
        if (identity) {
            v = (src[(size_t)oy * W + ox] - mean) / sd;
        } else {
            const float sy = fmaxf(inv_sf * ((float)oy + 0.5f) - 0.5f, 0.0f), sx = fmaxf(inv_sf * ((float)ox + 0.5f) - 0.5f, 0.0f);
            const int y0 = min((int)sy, H - 1), x0 = min((int)sx, W - 1);
            const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
            const float ly = sy - (float)y0, lx = sx - (float)x0, hy = 1.0f - ly, hx = 1.0f - lx;
            const float a = (src[(size_t)y0 * W + x0] - mean) / sd, b = (src[(size_t)y0 * W + x1] - mean) / sd;
            const float d = (src[(size_t)y1 * W + x0] - mean) / sd, e = (src[(size_t)y1 * W + x1] - mean) / sd;
            v = hy * (hx * a + lx * b) + ly * (hx * d + lx * e);
        }
        out[idx] = v;
    }
}

// token rows of one scale: x0[img, 0] = cls + pos[0], x0[img, 1 + p] = patch_out[img P + p] + pos[1 + p]   (T = 1 + P tokens, D columns)
__global__ __launch_bounds__(256) void pd_vt_assemble_kernel(const float *__restrict__ patch_out, const float *__restrict__ cls,
                                                             const float *__restrict__ pos, int n, int T, int D, float *__restrict__ x0) {
    const size_t total = (size_t)n * T * D;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % D);
        const size_t row = idx / D;
        const int im = (int)(row / T), t = (int)(row - (size_t)im * T);
        const float v = t == 0 ? cls[c] : patch_out[((size_t)im * (T - 1) + (t - 1)) * D + c];
        x0[idx] = v + pos[(size_t)t * D + c];
    }
}

// its adjoint: dpatch[img P + p] = dx0[img, 1 + p] (the patch GEMM's output gradient, compact rows), dpos[t] = sum over the images of
// dx0[img, t] in image order (row 0 is d cls as well); one thread per (token, column)
__global__ __launch_bounds__(256) void pd_vt_assemble_bwd_kernel(const float *__restrict__ dx0, int n, int T, int D, float *__restrict__ dpatch,
                                                                 float *__restrict__ dpos) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= T * D) return;
    const int t = idx / D, c = idx - t * D;
    double s = 0.0;
    for (int im = 0; im < n; ++im) {
        const float v = dx0[((size_t)im * T + t) * D + c];
        if (t > 0) dpatch[((size_t)im * (T - 1) + (t - 1)) * D + c] = v;
        s += (double)v;
    }
    dpos[idx] = (float)s;
}

// nn.GELU(), exact erf form, of the stashed fc1 pre-activation (total = rows x hidden, a multiple of 4)
__device__ __forceinline__ float pd_vt_gelu(float a) { return 0.5f * a * (1.0f + erff(a * 0.70710678118654752f)); }
__global__ __launch_bounds__(256) void pd_vt_gelu_kernel(const float4 *__restrict__ pre, float4 *__restrict__ out, size_t total4) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
        const float4 a = pre[i];
        out[i] = make_float4(pd_vt_gelu(a.x), pd_vt_gelu(a.y), pd_vt_gelu(a.z), pd_vt_gelu(a.w));
    }
}
// dy <- dy (Phi(a) + a phi(a)), Phi / phi the standard normal's distribution / density, in place on the data gradient of fc2's input
__device__ __forceinline__ float pd_vt_gelu_grad(float a) {
    const float cdf = 0.5f * (1.0f + erff(a * 0.70710678118654752f));
    return fmaf(a * 0.3989422804014327f, expf(-0.5f * a * a), cdf);
}
__global__ __launch_bounds__(256) void pd_vt_gelu_bwd_kernel(const float4 *__restrict__ pre, float4 *__restrict__ dy, size_t total4) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
        const float4 a = pre[i];
        float4 g = dy[i];
        g.x *= pd_vt_gelu_grad(a.x); g.y *= pd_vt_gelu_grad(a.y); g.z *= pd_vt_gelu_grad(a.z); g.w *= pd_vt_gelu_grad(a.w);
        dy[i] = g;
    }
}

// Final LayerNorm (eps) of the CLS rows x[img T] and the average over the scales, one wave per image:
//   z = (first ? 0 : z) + LN(x[img T]);  the last scale divides the sum by n_scales (the reference sums the features, then divides).
// stats[img] = (mean, rstd) is kept for the backward.
__global__ __launch_bounds__(256) void pd_vt_final_kernel(const float *__restrict__ x, int n, int T, int D, const float *__restrict__ gamma,
                                                          const float *__restrict__ beta, float eps, int first, int last, int n_scales,
                                                          float *__restrict__ z, float *__restrict__ stats) {
    const int im = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (im >= n) return;
    const float *src = x + (size_t)im * T * D;
    float mean, rstd;
    pd_wave_row_stats(src, D, lane, eps, &mean, &rstd);
    float *dst = z + (size_t)im * D;
    for (int c = lane; c < D; c += 64) {
        const float f = (src[c] - mean) * rstd * gamma[c] + beta[c];
        const float acc = first ? f : dst[c] + f;
        dst[c] = last ? acc / (float)n_scales : acc;
    }
    if (lane == 0) {
        stats[2 * (size_t)im] = mean;
        stats[2 * (size_t)im + 1] = rstd;
    }
}

// Its data gradient, one wave per token row of the scale: the CLS row of image img receives the LayerNorm backward of g = g_z[img] /
// n_scales, every other row of the last residual gradient is written as exactly zero.
__global__ __launch_bounds__(256) void pd_vt_final_bwd_kernel(const float *__restrict__ g_z, const float *__restrict__ x, const float *__restrict__ stats,
                                                              const float *__restrict__ gamma, int n, int T, int D, int n_scales,
                                                              float *__restrict__ dres) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n * T) return;
    float *o = dres + (size_t)row * D;
    const int im = row / T;
    if (row != im * T) {
        for (int c = lane; c < D; c += 64) o[c] = 0.0f;
        return;
    }
    const float *xr = x + (size_t)row * D, *gr = g_z + (size_t)im * D;
    const float mean = stats[2 * (size_t)im], rstd = stats[2 * (size_t)im + 1], ns = (float)n_scales;
    float s1 = 0.0f, s2 = 0.0f;
    for (int c = lane; c < D; c += 64) {
        const float g = gr[c] / ns * gamma[c], xh = (xr[c] - mean) * rstd;
        s1 += g;
        s2 = fmaf(g, xh, s2);
    }
    const float m1 = pd_wave_sum(s1) / (float)D, m2 = pd_wave_sum(s2) / (float)D;
    for (int c = lane; c < D; c += 64) {
        const float g = gr[c] / ns * gamma[c], xh = (xr[c] - mean) * rstd;
        o[c] = rstd * (g - m1 - xh * m2);
    }
}

// ... and its parameter gradients, one thread per column, the images added in image order (in double, as pd_tr_colsum_kernel adds rows):
// dgamma (+)= sum_img g xhat, dbeta (+)= sum_img g; either may be null
__global__ __launch_bounds__(256) void pd_vt_final_param_kernel(const float *__restrict__ g_z, const float *__restrict__ x, const float *__restrict__ stats,
                                                                int n, int T, int D, int n_scales, int accumulate, float *__restrict__ dgamma,
                                                                float *__restrict__ dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= D) return;
    const float ns = (float)n_scales;
    double a = 0.0, b = 0.0;
    for (int im = 0; im < n; ++im) {
        const float g = g_z[(size_t)im * D + c] / ns;
        const float xh = (x[(size_t)im * T * D + c] - stats[2 * (size_t)im]) * stats[2 * (size_t)im + 1];
        a += (double)g * (double)xh;
        b += (double)g;
    }
    if (dgamma) dgamma[c] = accumulate ? dgamma[c] + (float)a : (float)a;
    if (dbeta) dbeta[c] = accumulate ? dbeta[c] + (float)b : (float)b;
}

// torch's bicubic kernel (A = -0.75) at distance x from a tap: |x| <= 1 and 1 < |x| < 2
__device__ __forceinline__ float pd_vt_cubic1(float x) { return ((1.25f * x - 2.25f) * x) * x + 1.0f; }
__device__ __forceinline__ float pd_vt_cubic2(float x) { return ((-0.75f * x + 3.75f) * x - 6.0f) * x + 3.0f; }
// the four taps of output index o along one axis of a g-long source: rows clamped to [0, g - 1], weights as upsample_bicubic2d forms them
// (source coordinate rscale (o + 0.5) - 0.5, rscale = float(1 / scale_factor), not clamped; t = its fractional part)
__device__ __forceinline__ void pd_vt_cubic_taps(int o, int g, float rscale, int *rows, float *wts) {
    const float src = rscale * ((float)o + 0.5f) - 0.5f;
    const float fl = floorf(src), t = src - fl;
    const int i0 = (int)fl;
    wts[0] = pd_vt_cubic2(t + 1.0f);
    wts[1] = pd_vt_cubic1(t);
    wts[2] = pd_vt_cubic1(1.0f - t);
    wts[3] = pd_vt_cubic2(2.0f - t);
#pragma unroll
    for (int k = 0; k < 4; ++k) rows[k] = min(max(i0 - 1 + k, 0), g - 1);
}

// d pos_embed [1 + g g, D] and d cls_token [D] from ONE scale's dpos [1 + gh gw, D] (pd_vt_assemble_bwd_kernel), written (accumulate = 0: the
// first scale of the call) or added.  Row 0 -- the CLS position, and d cls_token with it -- is dpos[0].  A scale on the trained grid
// (resampled = 0) adds dpos[1 + cell] directly; a resampled one gathers the adjoint of DINO's interpolate_pos_encoding: thread (cell, column)
// walks the outputs (oy, ox) in output order and adds wy wx dpos[1 + oy gw + ox] for every tap pair that lands on its cell.  The tap tables
// of both axes are built once per workgroup in LDS.  Either destination may be null.
__global__ __launch_bounds__(256) void pd_vt_posgrid_kernel(const float *__restrict__ dpos, int gh, int gw, int g, int D, int resampled, int accumulate,
                                                            float rscale_y, float rscale_x, float *__restrict__ dpos_embed, float *__restrict__ dcls) {
    __shared__ int yrow[PD_VT_MAX_TOKENS * 4], xrow[PD_VT_MAX_TOKENS * 4];
    __shared__ float ywt[PD_VT_MAX_TOKENS * 4], xwt[PD_VT_MAX_TOKENS * 4];
    if (resampled) {
        for (int o = threadIdx.x; o < gh; o += blockDim.x) pd_vt_cubic_taps(o, g, rscale_y, yrow + 4 * o, ywt + 4 * o);
        for (int o = threadIdx.x; o < gw; o += blockDim.x) pd_vt_cubic_taps(o, g, rscale_x, xrow + 4 * o, xwt + 4 * o);
        __syncthreads();
    }
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (1 + g * g) * D) return;
    const int r = idx / D, c = idx - r * D;
    float v;
    if (r == 0) {
        v = dpos[c];
        if (dcls) dcls[c] = accumulate ? dcls[c] + v : v;
    } else if (!resampled) {
        v = dpos[(size_t)r * D + c];
    } else {
        const int cy = (r - 1) / g, cx = (r - 1) - cy * g;
        v = 0.0f;
        for (int oy = 0; oy < gh; ++oy)
            for (int i = 0; i < 4; ++i) {
                if (yrow[4 * oy + i] != cy) continue;
                const float wy = ywt[4 * oy + i];
                for (int ox = 0; ox < gw; ++ox)
                    for (int j = 0; j < 4; ++j)
                        if (xrow[4 * ox + j] == cx) v = fmaf(wy * xwt[4 * ox + j], dpos[(size_t)(1 + oy * gw + ox) * D + c], v);
            }
    }
    if (dpos_embed) dpos_embed[idx] = accumulate ? dpos_embed[idx] + v : v;
}
