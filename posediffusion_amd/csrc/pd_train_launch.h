// pd_train_launch.h -- what the two trainers share on the host side (pd_train.hip; pd_vit_train.hip, section 3.10): the
// limits their allocations are sized by, the chunk rule of a reduction over token rows, the argument structs of the shared kernels and
// the launch helpers.  The pd_tr_* kernels (pd_train_kernels.h) are compiled ONCE, in pd_train.hip, which also defines every helper
// declared here; pd_vit_train.hip reaches those kernels through the helpers alone, so the library holds one device copy of each and one
// kernel handle (with its dynamic-LDS bound) per instantiation.  The helpers are internal to the library (hidden visibility).
#pragma once
#include <algorithm>
#include <stddef.h>

#define PD_TR_MAX_CHUNKS 16
#define PD_TR_MAX_HD 128
#define PD_TR_LA_MAX_N 256          // frames of a sequence / tokens of an image the key-tiled attention takes (pd_train_lattn.h: 4 tiles of 64 keys)
#define PD_TR_LA_STATS 4            // floats per (b, h, i) between its backward's phases: row maximum, 1 / sum, rs of lanes 0 .. 31, rs of lanes 32 .. 63

// the chunks of a reduction over M token rows: a function of M alone
static inline void pd_tr_chunks(int M, int *n_chunks, int *rows) {
    int n = std::min(PD_TR_MAX_CHUNKS, (M + 255) / 256);
    int r = (M + n - 1) / n;
    r = (r + 31) / 32 * 32;
    *rows = r;
    *n_chunks = (M + r - 1) / r;
}

#ifndef PD_TR_LAUNCH_HOST_ONLY      // (a plain C++ translation unit may include this file for what stands above)
#include "pd_internal.h"

// one site of one layer in one call; philox = 0: no mask, the scale alone (the data gradient behind a masked ReLU stash)
struct PdTrDrop {
    unsigned int thr, key0, key1, step, ctr2;   // ctr2 = 4 layer + site
    float scale;                                // 1 / (1 - p), fp32, from the host
    int philox;
};

struct PdTrGemm {
    const float *A;                 // A(i, r) = A[i * a_rs + r * a_cs]
    long long a_rs, a_cs;
    const float *B;                 // B(r, j) = B[r * b_rs + j * b_cs]
    long long b_rs, b_cs;
    float *C;                       // C(i, j) = C[i * ldc + j]; slice z of a split reduction starts at C + z * I * ldc
    long long ldc;
    const float *bias;              // [J] added per column, or null
    const float *resid;             // [I, ldr] added last (a residual stream, or C itself to accumulate), or null
    long long ldr;
    const float *aux;               // [I, ldaux] the mask operand, or null
    long long ldaux;
    int mask_mode;                  // 1: result kept where aux > 0 (ReLU backward from the stashed post-ReLU values); 2: times SiLU'(aux)
    int relu;                       // ReLU after the bias
    int I, J, R;
    int r_chunk;                    // reduction indices per blockIdx.z
    int a_rfast, b_rfast;           // 1: the reduction index is the contiguous one of that operand in memory (picks the coalesced staging pattern)
};

// the scratch of a trainer that the helpers write
struct PdTrWork {
    float *ws;                      // split-reduction workspace: weight-gradient partials [chunks][Nout x K]
    double *ws_col;                 // column-sum partials [2][chunks][C]
    float *la_stats;                // [rows nhead, PD_TR_LA_STATS] between the two phases of the key-tiled attention backward
};

#define PD_TR_LOCAL __attribute__((visibility("hidden")))

// the dynamic-LDS bound of every attention instantiation (a per-process attribute of the kernel): the family's limits, 64 / 256 frames at
// head dim 128, never a trainer's own shape.  Both *_create functions call it.
PD_TR_LOCAL int pd_tr_set_attention_lds();

// nz slices of g.r_chunk reduction indices each; dr: the epilogue's dropout, or null
PD_TR_LOCAL void pd_tr_gemm_launch(const PdTrGemm &g, int nz, hipStream_t s, const PdTrDrop *dr = nullptr);
// Y[M, Nout] = X[M, K] W[Nout, K]^T + b (+ ReLU) (+ dropout `dr`) (+ resid)
PD_TR_LOCAL void pd_tr_linear(const float *X, const float *W, const float *b, float *Y, int M, int Nout, int K, int relu, const float *resid,
                              hipStream_t s, const PdTrDrop *dr = nullptr);
// dW[Nout, K] (+)= sum_m dY[m, :]^T X[m, :] over the chunks of M, partials added in chunk order; db[Nout] (+)= sum_m dY[m, :] likewise.
// acc adds to what dW / db hold: one chunk through the GEMM's resid = C path, several through the accumulating reduce.  Either may be null
PD_TR_LOCAL void pd_tr_wgrad(const PdTrWork &wk, const float *dY, const float *X, float *dW, float *db, int M, int Nout, int K, bool acc, hipStream_t s);
// LayerNorm's dgamma (+)= sum_m dy xhat, dbeta (+)= sum_m dy; either may be null
PD_TR_LOCAL void pd_tr_ln_param_grads(const PdTrWork &wk, const float *dy, const float *x, const float *stats, float *dgamma, float *dbeta, int M, int D,
                                      bool acc, hipStream_t s);
// out[e] = ws[0][e] + ... + ws[nz - 1][e] over `total` elements (the slices of a split pd_tr_gemm_launch)
PD_TR_LOCAL void pd_tr_reduce_launch(const float *ws, long long total, int nz, float *out, hipStream_t s);
// LayerNorm over rows [M, D] with its affine; stats[m] = (mean, rstd) unless stats is null
PD_TR_LOCAL void pd_tr_ln_launch(const float *in, float *out, const float *gamma, const float *beta, int M, int D, float eps, float *stats, hipStream_t s);
// its data gradient, ADDED to dres
PD_TR_LOCAL void pd_tr_ln_bwd_launch(const float *dy, const float *x, const float *stats, const float *gamma, int M, int D, float *dres, hipStream_t s);
// attention forward of one layer: the short kernel (a sequence whole in LDS, N <= 64) or the key-tiled one.  nf: DEVICE [B] frame counts per
// sequence (pd_trainer_set_frame_counts; N is then the row stride alone), key-tiled kernels only; null = uniform, the call as it always was
PD_TR_LOCAL void pd_tr_attn_launch(bool tiled, const float *qkv, float *ctx, int B, int N, int nhead, int hd, int d, float scale, const PdTrDrop *dr,
                                   hipStream_t s, const int *nf = nullptr);
// attention backward of one layer: dqkv from qkv and dctx; tiled = phase A (dQ, row statistics into la_stats) then phase B (dK, dV)
PD_TR_LOCAL void pd_tr_attn_bwd_launch(bool tiled, const float *qkv, const float *dctx, float *dqkv, float *la_stats, int B, int N, int nhead, int hd,
                                       int d, float scale, const PdTrDrop *dr, hipStream_t s, const int *nf = nullptr);

#endif
