// pd_gemm_split.h -- split-precision GEMM on the bf16 matrix pipe, shared by the image feature extractor (pd_vit.hip) and the
// denoiser's fast mode (pd_denoiser.hip): every fp32 operand is carried as bf16 hi + bf16 lo (x ~= hi + lo, 16 mantissa bits),
// x * w ~= hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 (16 x the rate of the f32 instruction per product, three
// products), fp32 accumulation.  Activations between kernels are one 32-bit word per element {hi | lo << 16}
// (pd_split_word, pd_gemm_stream.h).
//
// F16 (the denoiser's fp16-plane mode): the same kernel with fp16 halves (pd_split_word_h) on v_mfma_f32_32x32x16_f16 -- 11 + 11
// mantissa bits, the dropped lo*lo term is 2^-22 of the product: with fp32 accumulation the result is as close to the fp64 product
// as the exact-fp32 kernel's (tools/split3_probe.hip).  fp16's narrow exponent range is handled by the caller with POWER-OF-TWO
// scales fixed at engine creation from provable bounds on every operand (pd_denoiser_build_split): A arrives as words of
// a * 2^ea, W was split as w * 2^ew, the epilogue multiplies the accumulator by c_scale = 2^-(ea + ew) (exact) and, where it
// writes split words itself (EPI 3 / 4), by out_scale = 2^e of the next GEMM's operand.
//
// The strip kernel (pd_gemm_strip.h: the large-batch denoiser's and the ViT's launches, the same operands delivered differently) multiplies on
// v_mfma_f32_16x16x32_f16 instead: 32 k per instruction, so a sum's rounding differs in the last bit from two chained 16-k instructions -- the same operands,
// products and order otherwise.
#pragma once
#include "pd_gemm_stream.h"

// GELU for the split-precision path: erf by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7, below the 2^-17 the split operands
// keep), a dozen instructions instead of erff's ~35 -- the epilogue of fc1 is as long as its matrix loop otherwise.
// 0.5 v (1 + erf(v / sqrt 2)) = v (1 - q / 2) for v >= 0 and v q / 2 for v < 0, q = erfc(|v| / sqrt 2) (no cancellation).
__device__ __forceinline__ float vit_gelu_fast(float v) {
    const float x = fabsf(v) * 0.70710678118654752f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, x, 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float q = 0.5f * p * t * __expf(-x * x);
    return v * (v >= 0.0f ? 1.0f - q : q);
}

struct VitSplitArgs {
    const unsigned *A, *W;      // A: split words [M][lda]; W: pd_frag_split_kernel's fragment order (pd_weight_prep.hip)
    const float *bias;
    void *C;                    // EPI 0 / 2: fp32 [M][Nout]; EPI 3 (gelu) / 4 (relu): split words [M][Nout]
    int M, Nout, K, lda;
    float c_scale, out_scale;   // F16 only (see the header): accumulator scale, scale of split-word outputs
#ifdef PD_STRIP_LEGS
    long long *legs;            // tools/strip_legs_probe.hip only: [workgroup][8] = {wall start, wall end, cycles: entry, operands landed, K loop done, end, XCC id, CU id}
#endif
};

// A rows stream through LDS (un-zipped into hi / lo fragments on the way, shared by the waves of a row block); the weight
// fragments go straight from global memory / L2 to registers, one chunk ahead (they are already in operand order, and
// keeping them out of LDS halves its traffic -- the LDS array, not the matrix pipe, limited the first version).
// BARE (tools/split3_probe.hip only): 1 no weight-fragment loads after the first chunk, 2 no A loads / LDS stores after it, 3 both,
// 4 all of that and no barrier, 5 no MFMAs (everything else as in production) -- what bounds the kernel
template <int EPI, int WM, int WN, bool F16 = false, int BARE = 0>
__global__ __launch_bounds__(256) void vit_gemm_split_kernel(VitSplitArgs g) {
    constexpr int KC = PD_STREAM_KC, LR = PD_STREAM_LR, TM = 64 * WM, TN = 64 * WN, GROUP = 2048 / TM;
    static_assert(KC == 32 && WM <= 2 && WN <= 2, "staging: 4 groups of 8 per row chunk, passes of 64 rows");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    unsigned *As = (unsigned *)lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5, wm = wave & 1, wn = wave >> 1;
    const int MT = (g.M + TM - 1) / TM, NT = g.Nout / TN;
    int mtile, ntile;
    {
        const int b = blockIdx.x, full = (MT / GROUP) * GROUP * NT;
        if (b < full) {
            const int grp = b / (NT * GROUP), r = b - grp * (NT * GROUP);
            ntile = r / GROUP;
            mtile = grp * GROUP + r % GROUP;
        } else {
            const int r = b - full, rest = MT % GROUP;
            ntile = r / rest;
            mtile = (MT / GROUP) * GROUP + r % rest;
        }
    }
    const int m0 = mtile * TM, n0 = ntile * TN;
    const int sr = tid >> 2, sg = tid & 3, st = sr * LR + 8 * sg;      // 4 threads per row chunk, one group of 8 each
    const int KS = g.K / 16;
#define VP_EACH(X) X(0) X(1)
#define VP_DECL(j)                                                                                                            \
    const uint4 *ap##j = (const uint4 *)(g.A + (size_t)min(m0 + sr + 64 * (j < WM ? j : 0), g.M - 1) * g.lda) + 2 * sg;        \
    const uint4 *wq##j = (const uint4 *)g.W + (size_t)(n0 / 32 + wn * WN + (j < WN ? j : 0)) * KS * 128 + lane;                 \
    uint4 ra##j##a, ra##j##b, cw##j##0h, cw##j##0l, cw##j##1h, cw##j##1l, nw##j##0h, nw##j##0l, nw##j##1h, nw##j##1l;
#define VP_LOAD(j)                                  \
    if constexpr (j < WM) {                         \
        ra##j##a = ap##j[nx];                       \
        ra##j##b = ap##j[nx + 1];                   \
    }                                               \
    if constexpr (j < WN) {                         \
        nw##j##0h = wq##j[(size_t)(nc * 4 + 0) * 64]; \
        nw##j##0l = wq##j[(size_t)(nc * 4 + 1) * 64]; \
        nw##j##1h = wq##j[(size_t)(nc * 4 + 2) * 64]; \
        nw##j##1l = wq##j[(size_t)(nc * 4 + 3) * 64]; \
    }
#define VP_LOAD_A(j)                                \
    if constexpr (j < WM) {                         \
        ra##j##a = ap##j[nx];                       \
        ra##j##b = ap##j[nx + 1];                   \
    }
#define VP_LOAD_W(j)                                \
    if constexpr (j < WN) {                         \
        nw##j##0h = wq##j[(size_t)(nc * 4 + 0) * 64]; \
        nw##j##0l = wq##j[(size_t)(nc * 4 + 1) * 64]; \
        nw##j##1h = wq##j[(size_t)(nc * 4 + 2) * 64]; \
        nw##j##1l = wq##j[(size_t)(nc * 4 + 3) * 64]; \
    }
#define VP_ROLL(j)             \
    if constexpr (j < WN) {    \
        cw##j##0h = nw##j##0h; \
        cw##j##0l = nw##j##0l; \
        cw##j##1h = nw##j##1h; \
        cw##j##1l = nw##j##1l; \
    }
#define VP_STORE(j)                                                                                       \
    if constexpr (j < WM) {                                                                               \
        uint4 h, l;                                                                                       \
        h.x = __builtin_amdgcn_perm(ra##j##a.y, ra##j##a.x, 0x05040100u);                                 \
        l.x = __builtin_amdgcn_perm(ra##j##a.y, ra##j##a.x, 0x07060302u);                                 \
        h.y = __builtin_amdgcn_perm(ra##j##a.w, ra##j##a.z, 0x05040100u);                                 \
        l.y = __builtin_amdgcn_perm(ra##j##a.w, ra##j##a.z, 0x07060302u);                                 \
        h.z = __builtin_amdgcn_perm(ra##j##b.y, ra##j##b.x, 0x05040100u);                                 \
        l.z = __builtin_amdgcn_perm(ra##j##b.y, ra##j##b.x, 0x07060302u);                                 \
        h.w = __builtin_amdgcn_perm(ra##j##b.w, ra##j##b.z, 0x05040100u);                                 \
        l.w = __builtin_amdgcn_perm(ra##j##b.w, ra##j##b.z, 0x07060302u);                                 \
        *(uint4 *)(da + st + j * 64 * LR) = h;                                                            \
        *(uint4 *)(da + st + j * 64 * LR + 4) = l;                                                        \
    }
// the three products of one (column tile j, k step s) against every row tile
#define VP_MMA(j, s)                                                                                                         \
    if constexpr (j < WN) {                                                                                                  \
        _Pragma("unroll") for (int mi = 0; mi < WM; ++mi) {                                                                  \
            acc[mi][j < WN ? j : 0] = mma(al##s[mi], cw##j##s##h, acc[mi][j < WN ? j : 0]);                                    \
            acc[mi][j < WN ? j : 0] = mma(ah##s[mi], cw##j##s##l, acc[mi][j < WN ? j : 0]);                                    \
            acc[mi][j < WN ? j : 0] = mma(ah##s[mi], cw##j##s##h, acc[mi][j < WN ? j : 0]);                                    \
        }                                                                                                                    \
    }
    auto mma = [](const uint4 &a, const uint4 &b, const f32x16 &c) {
        if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
        else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    };
    VP_EACH(VP_DECL)
    {
        const int nx = 0, nc = 0;
        unsigned *da = As;
        VP_EACH(VP_LOAD)
        VP_EACH(VP_STORE)
        VP_EACH(VP_ROLL)
    }
    __syncthreads();
    f32x16 acc[WM][WN];
#pragma unroll
    for (int mi = 0; mi < WM; ++mi)
#pragma unroll
        for (int ni = 0; ni < WN; ++ni)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mi][ni][i] = 0.0f;
    const int nk = g.K / KC;
    const int aoff = (wm * 32 * WM + l31) * LR + 8 * hi;
    for (int kc = 0; kc < nk; ++kc) {
        const int nc = min(kc + 1, nk - 1), nx = nc * (KC / 4);       // the chunk after the last is the last again
        if constexpr (BARE == 0 || BARE == 5) { VP_EACH(VP_LOAD) }
        else if constexpr (BARE == 1) { VP_EACH(VP_LOAD_A) }
        else if constexpr (BARE == 2) { VP_EACH(VP_LOAD_W) }
        __builtin_amdgcn_sched_barrier(0);
        const unsigned *a = As + (kc & 1) * TM * LR + aoff;
        uint4 ah0[WM], al0[WM], ah1[WM], al1[WM];     // 16 k per step: lanes 0-31 take group 2 s, lanes 32-63 group 2 s + 1
#pragma unroll
        for (int mi = 0; mi < WM; ++mi) {
            ah0[mi] = *(const uint4 *)(a + mi * 32 * LR);
            al0[mi] = *(const uint4 *)(a + mi * 32 * LR + 4);
            ah1[mi] = *(const uint4 *)(a + mi * 32 * LR + 16);
            al1[mi] = *(const uint4 *)(a + mi * 32 * LR + 20);
        }
        if constexpr (BARE != 5) {
            VP_MMA(0, 0)
            VP_MMA(1, 0)
            VP_MMA(0, 1)
            VP_MMA(1, 1)
        }
        __builtin_amdgcn_sched_barrier(0);
        unsigned *da = As + ((kc + 1) & 1) * TM * LR;
        if constexpr (BARE == 0 || BARE == 1 || BARE == 5) { VP_EACH(VP_STORE) }
        if constexpr (BARE == 0 || BARE == 2 || BARE == 5) { VP_EACH(VP_ROLL) }
        if constexpr (BARE != 4) __syncthreads();
    }
#undef VP_DECL
#undef VP_LOAD
#undef VP_LOAD_A
#undef VP_LOAD_W
#undef VP_ROLL
#undef VP_STORE
#undef VP_MMA
#pragma unroll
    for (int mi = 0; mi < WM; ++mi)
#pragma unroll
        for (int ni = 0; ni < WN; ++ni) {
            const int col = n0 + (wn * WN + ni) * 32 + l31, r0 = m0 + (wm * WM + mi) * 32 + 4 * hi;
            const float bias = g.bias[col];
            float res[16];
            if constexpr (EPI == 2) {
#pragma unroll
                for (int i = 0; i < 16; ++i) res[i] = ((const float *)g.C)[(size_t)min(r0 + (i & 3) + 8 * (i >> 2), g.M - 1) * g.Nout + col];
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = r0 + (i & 3) + 8 * (i >> 2);
                float v = F16 ? fmaf(acc[mi][ni][i], g.c_scale, bias) : acc[mi][ni][i] + bias;
                if constexpr (EPI == 3) v = vit_gelu_fast(v);
                if constexpr (EPI == 4) v = pd_relu(v);
                if constexpr (EPI == 2) v += res[i];
                if (row < g.M) {
                    if constexpr (EPI == 3 || EPI == 4)
                        ((unsigned *)g.C)[(size_t)row * g.Nout + col] = pd_split_word_as<F16 ? 2 : 1>(v, g.out_scale);
                    else
                        ((float *)g.C)[(size_t)row * g.Nout + col] = v;
                }
            }
        }
}

static constexpr size_t pd_split_lds(int WM) { return (size_t)2 * 64 * WM * PD_STREAM_LR * sizeof(float); }
template <int EPI, int WM, int WN, bool F16 = false>
static inline void pd_gemm_split(const unsigned *A, int lda, const unsigned *W, int K, const float *bias, void *C, int M, int Nout, hipStream_t s,
                                 float c_scale = 1.0f, float out_scale = 1.0f) {
    VitSplitArgs g{A, W, bias, C, M, Nout, K, lda, c_scale, out_scale};
    constexpr int TM = 64 * WM, TN = 64 * WN;
    hipLaunchKernelGGL((vit_gemm_split_kernel<EPI, WM, WN, F16>), dim3(((M + TM - 1) / TM) * (Nout / TN)), dim3(256), pd_split_lds(WM), s, g);
}
