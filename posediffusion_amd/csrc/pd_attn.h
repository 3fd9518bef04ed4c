// pd_attn.h -- the attention core of the default-shape denoiser as kernels of its own (the fp16-plane mode's fused in_proj + attention kernel
// is pd_qkv_attn.h): one query row per wave (small batches), whole sequences per workgroup (large batches), and on the matrix pipe (N <= 32).
#pragma once
#include "pd_gemm_small.h"      // PD_STAMP
#include "pd_gemm_stream.h"     // pd_split_word, pd_split_word_as

// --------------------------------------------------------------------------------------------
// attention core: softmax(q k^T / sqrt(dh)) v for one (sequence, head), N <= 64 frames, no mask
// (nn.MultiheadAttention inside the encoder layer).  grid = (B*heads, ceil(N/4)): every
// workgroup stages K and V of its (sequence, head) and each of its 4 waves owns ONE query row:
// lane j scores key j, softmax is a wave reduction, lanes then own 2 of the 128 output dims.
// --------------------------------------------------------------------------------------------
// SPLIT_OUT: ctx is written as split words {bf16 hi | bf16 lo << 16} for pd_gemm_split (the fast mode)
template <bool SPLIT_OUT>
__global__ __launch_bounds__(256) void pd_attn_kernel(const float *__restrict__ qkv, float *__restrict__ ctx, int N
#ifdef PD_DEN_STAMPS
                                                      , long long *stamps
#endif
) {
    PD_STAMP(stamps, 0);
    constexpr int LD = DH + 4;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *Kk = lds, *V = Kk + N * LD, *Q = V + N * LD, *P = Q + 4 * LD;   // P [4][64]
    const int b = blockIdx.x / NH, h = blockIdx.x % NH, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.y * 4 + wave;        // this wave's query row
    const float scale = 0.08838834764831845f;   // 1/sqrt(128)
    const float *base = qkv + (size_t)b * N * (3 * DM) + h * DH;
    for (int idx = tid; idx < N * (DH / 4); idx += 256) {
        const int j = idx / (DH / 4), d4 = idx % (DH / 4);
        const float *row = base + (size_t)j * (3 * DM) + d4 * 4;
        *(float4 *)(Kk + j * LD + d4 * 4) = *(const float4 *)(row + DM);
        *(float4 *)(V + j * LD + d4 * 4) = *(const float4 *)(row + 2 * DM);
    }
    if (lane < DH / 4) {
        const int ii = i < N ? i : N - 1;
        float4 q = *(const float4 *)(base + (size_t)ii * (3 * DM) + lane * 4);
        q.x *= scale; q.y *= scale; q.z *= scale; q.w *= scale;
        *(float4 *)(Q + wave * LD + lane * 4) = q;
    }
    __syncthreads();
    PD_STAMP(stamps, 2);                  // K, V, Q staged
    const int jj = lane < N ? lane : N - 1;
    const float4 *qa = (const float4 *)(Q + wave * LD), *kb = (const float4 *)(Kk + jj * LD);
    float s = 0.0f;
#pragma unroll 8
    for (int d = 0; d < DH / 4; ++d) {
        const float4 a = qa[d], c = kb[d];
        s = fmaf(a.x, c.x, s);
        s = fmaf(a.y, c.y, s);
        s = fmaf(a.z, c.z, s);
        s = fmaf(a.w, c.w, s);
    }
    const float sv = lane < N ? s : -INFINITY;
    const float mx = pd_wave_max(sv);
    const float e = lane < N ? expf(sv - mx) : 0.0f;
    const float inv = 1.0f / pd_wave_sum(e);
    P[wave * 64 + lane] = e * inv;
    __syncthreads();
    if (i < N) {
        const float *p = P + wave * 64;
        float o0 = 0.0f, o1 = 0.0f;
        for (int j = 0; j < N; ++j) {
            const float pj = p[j];
            o0 = fmaf(pj, V[j * LD + lane], o0);
            o1 = fmaf(pj, V[j * LD + 64 + lane], o1);
        }
        float *out = ctx + (size_t)(b * N + i) * DM + h * DH;
        if constexpr (SPLIT_OUT) {
            ((unsigned *)out)[lane] = pd_split_word(o0);
            ((unsigned *)out)[64 + lane] = pd_split_word(o1);
        } else {
            out[lane] = o0;
            out[64 + lane] = o1;
        }
    }
    PD_STAMP(stamps, 5);
    PD_STAMP_DRAIN();
    PD_STAMP(stamps, 6);
}

// The same attention for large batches: ONE workgroup per (sequence, head) stages K, V and all N query rows once (pd_attn_kernel
// stages K and V ceil(N / 4) times, once per group of four query rows: 5 120 workgroups per layer at the bench shape, 9 - 15 % of the
// denoiser's kernel time for ~1 % of its FLOPs), and every wave works on PD_ATTN_RPW query rows AT ONCE: one K (V) read from LDS serves
// all of them and their serial fmaf chains (128 deep for a score) interleave -- a wave with one row at a time is bound by exactly that
// chain's latency.  Per row the arithmetic is pd_attn_kernel's, operation for operation: the same bits.
#define PD_ATTN_RPW 5
// SPLIT_OUT: 0 fp32, 1 bf16 split words, 2 fp16 split words of ctx * out_scale (pd_split_word_as)
template <int SPLIT_OUT>
__global__ __launch_bounds__(256) void pd_attn_seq_kernel(const float *__restrict__ qkv, float *__restrict__ ctx, int N, float out_scale) {
    constexpr int LD = DH + 4, R = PD_ATTN_RPW;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *Kk = lds, *V = Kk + N * LD, *Q = V + N * LD, *P = Q + N * LD;   // P [4 waves][R][64]
    const int b = blockIdx.x / NH, h = blockIdx.x % NH, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float scale = 0.08838834764831845f;   // 1/sqrt(128)
    const float *base = qkv + (size_t)b * N * (3 * DM) + h * DH;
    for (int idx = tid; idx < N * (DH / 4); idx += 256) {
        const int j = idx / (DH / 4), d4 = idx % (DH / 4);
        const float *row = base + (size_t)j * (3 * DM) + d4 * 4;
        float4 q = *(const float4 *)row;
        q.x *= scale; q.y *= scale; q.z *= scale; q.w *= scale;
        *(float4 *)(Q + j * LD + d4 * 4) = q;
        *(float4 *)(Kk + j * LD + d4 * 4) = *(const float4 *)(row + DM);
        *(float4 *)(V + j * LD + d4 * 4) = *(const float4 *)(row + 2 * DM);
    }
    __syncthreads();
    const int jj = lane < N ? lane : N - 1;
    const float4 *kb = (const float4 *)(Kk + jj * LD);
    float *pw = P + wave * (R * 64);
    for (int i0 = 0; i0 < N; i0 += 4 * R) {       // rows i0 + wave * R + t, t < R; every wave takes part in every round (workgroup barriers)
        const int ib = i0 + wave * R;
        const float4 *qa[R];
        float s[R];
#pragma unroll
        for (int t = 0; t < R; ++t) {
            qa[t] = (const float4 *)(Q + min(ib + t, N - 1) * LD);
            s[t] = 0.0f;
        }
#pragma unroll 4
        for (int d = 0; d < DH / 4; ++d) {
            const float4 c = kb[d];
#pragma unroll
            for (int t = 0; t < R; ++t) {
                const float4 a = qa[t][d];
                s[t] = fmaf(a.x, c.x, s[t]);
                s[t] = fmaf(a.y, c.y, s[t]);
                s[t] = fmaf(a.z, c.z, s[t]);
                s[t] = fmaf(a.w, c.w, s[t]);
            }
        }
#pragma unroll
        for (int t = 0; t < R; ++t) {
            const float sv = lane < N ? s[t] : -INFINITY;
            const float mx = pd_wave_max(sv);
            const float e = lane < N ? expf(sv - mx) : 0.0f;
            const float inv = 1.0f / pd_wave_sum(e);
            pw[t * 64 + lane] = e * inv;
        }
        __syncthreads();
        float o0[R], o1[R];
#pragma unroll
        for (int t = 0; t < R; ++t) o0[t] = o1[t] = 0.0f;
        for (int j = 0; j < N; ++j) {
            const float v0 = V[j * LD + lane], v1 = V[j * LD + 64 + lane];
#pragma unroll
            for (int t = 0; t < R; ++t) {
                const float pj = pw[t * 64 + j];
                o0[t] = fmaf(pj, v0, o0[t]);
                o1[t] = fmaf(pj, v1, o1[t]);
            }
        }
#pragma unroll
        for (int t = 0; t < R; ++t) {
            const int i = ib + t;
            if (i < N) {
                float *out = ctx + (size_t)(b * N + i) * DM + h * DH;
                if constexpr (SPLIT_OUT != 0) {
                    ((unsigned *)out)[lane] = pd_split_word_as<SPLIT_OUT>(o0[t], out_scale);
                    ((unsigned *)out)[64 + lane] = pd_split_word_as<SPLIT_OUT>(o1[t], out_scale);
                } else {
                    out[lane] = o0[t];
                    out[64 + lane] = o1[t];
                }
            }
        }
        __syncthreads();                          // P is rewritten by the next round
    }
}
// The same attention on the matrix pipe, for sequences of <= 32 frames (round 3): pd_attn_seq_kernel keeps 20 of 64 lanes busy in
// its score loop (lane = key) and is compute-bound at 19 - 20 us per layer against a ~10 us floor for moving 31 MB of QKV.  Here
// S = (Q / sqrt(dh)) K^T is four 16 x 16 tiles, one per wave, on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation, K = 128:
// 32 instructions per wave); softmax runs 8 lanes per row over S in LDS (max, expf, sum: the same formulas); O = P V is 2 x 8 tiles of
// 16 x 16, four per wave, K = 32 (32 instructions).  Rows and keys beyond N are zero / masked.  Same mathematics as pd_attn_kernel;
// the sums are MFMA-ordered instead of fmaf chains, so results agree to fp32 rounding (tests/test_gpu_parity_r3.py), not bit for bit.
template <int SPLIT_OUT>
__global__ __launch_bounds__(256) void pd_attn_mma_kernel(const float *__restrict__ qkv, float *__restrict__ ctx, int N, float out_scale) {
    constexpr int LD = DH + 4, LS = 36;
    extern __shared__ __attribute__((aligned(16))) float sm[];                   // Q, K, V: N + 1 rows each (row N is zero: every row / key
    const int NR = N + 1;                                                       // index beyond N reads it), S [32][36]: scores, then probabilities
    float *Q = sm, *Kk = Q + NR * LD, *V = Kk + NR * LD, *S = V + NR * LD;
    const int b = blockIdx.x / NH, h = blockIdx.x % NH, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float scale = 0.08838834764831845f;   // 1/sqrt(128)
    const float *base = qkv + (size_t)b * N * (3 * DM) + h * DH;
    for (int idx = tid; idx < NR * (DH / 4); idx += 256) {
        const int j = idx / (DH / 4), d4 = idx % (DH / 4);
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f), k = q, v = q;
        if (j < N) {
            const float *row = base + (size_t)j * (3 * DM) + d4 * 4;
            q = *(const float4 *)row;
            k = *(const float4 *)(row + DM);
            v = *(const float4 *)(row + 2 * DM);
            q.x *= scale; q.y *= scale; q.z *= scale; q.w *= scale;
        }
        *(float4 *)(Q + j * LD + d4 * 4) = q;
        *(float4 *)(Kk + j * LD + d4 * 4) = k;
        *(float4 *)(V + j * LD + d4 * 4) = v;
    }
    __syncthreads();
    {   // scores: wave w owns the tile rows 16 (w >> 1) .., keys 16 (w & 1) ..; lane = (row or key) % 16 + 16 g feeds k = 16 c + 4 g + e
        const float *qa = Q + min(16 * (wave >> 1) + (lane & 15), N) * LD + 4 * (lane >> 4);
        const float *kb = Kk + min(16 * (wave & 1) + (lane & 15), N) * LD + 4 * (lane >> 4);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < DH / 16; ++c) {
            const float4 a = *(const float4 *)(qa + 16 * c), k = *(const float4 *)(kb + 16 * c);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, k.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, k.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, k.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, k.w, acc, 0, 0, 0);
        }
        const int j = 16 * (wave & 1) + (lane & 15);
#pragma unroll
        for (int e = 0; e < 4; ++e) S[(16 * (wave >> 1) + 4 * (lane >> 4) + e) * LS + j] = acc[e];
    }
    __syncthreads();
    {   // softmax: 8 lanes per row, 4 keys per lane
        const int i = tid >> 3, sub = tid & 7;
        float4 sv = *(const float4 *)(S + i * LS + 4 * sub);
        const int j0 = 4 * sub;
        sv.x = j0 + 0 < N ? sv.x : -INFINITY;
        sv.y = j0 + 1 < N ? sv.y : -INFINITY;
        sv.z = j0 + 2 < N ? sv.z : -INFINITY;
        sv.w = j0 + 3 < N ? sv.w : -INFINITY;
        float mx = fmaxf(fmaxf(sv.x, sv.y), fmaxf(sv.z, sv.w));
        mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 4, 64));
        float4 e;
        e.x = j0 + 0 < N ? expf(sv.x - mx) : 0.0f;
        e.y = j0 + 1 < N ? expf(sv.y - mx) : 0.0f;
        e.z = j0 + 2 < N ? expf(sv.z - mx) : 0.0f;
        e.w = j0 + 3 < N ? expf(sv.w - mx) : 0.0f;
        const float inv = 1.0f / pd_sum8((e.x + e.y) + (e.z + e.w));
        e.x *= inv; e.y *= inv; e.z *= inv; e.w *= inv;
        *(float4 *)(S + i * LS + 4 * sub) = e;
    }
    __syncthreads();
    {   // O = P V: wave w owns the output columns [32 w, 32 w + 32) (two tiles) of both row tiles; k = key j = 16 c + 4 g + e
        f32x4 acc[2][2];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float *pa = S + (lane & 15) * LS + 4 * (lane >> 4);
        const float *vb = V + 32 * wave + (lane & 15);
        const int jg = 4 * (lane >> 4);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float4 p0 = *(const float4 *)(pa + 16 * c), p1 = *(const float4 *)(pa + 16 * LS + 16 * c);
            float v0[4], v1[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v0[e] = vb[min(16 * c + jg + e, N) * LD];
                v1[e] = vb[min(16 * c + jg + e, N) * LD + 16];
            }
            const float a0[4] = {p0.x, p0.y, p0.z, p0.w}, a1[4] = {p1.x, p1.y, p1.z, p1.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], v0[e], acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], v1[e], acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], v0[e], acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], v1[e], acc[1][1], 0, 0, 0);
            }
        }
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = 16 * rt + 4 * (lane >> 4) + e;
                if (i < N) {
                    float *out = ctx + (size_t)(b * N + i) * DM + h * DH + 32 * wave + (lane & 15);
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) {
                        if constexpr (SPLIT_OUT != 0) ((unsigned *)out)[16 * ct] = pd_split_word_as<SPLIT_OUT>(acc[rt][ct][e], out_scale);
                        else out[16 * ct] = acc[rt][ct][e];
                    }
                }
            }
    }
}
static size_t attn_mma_lds(int N) { return ((size_t)3 * (N + 1) * (DH + 4) + 32 * 36) * sizeof(float); }
static size_t attn_seq_lds(int N) { return ((size_t)3 * N * (DH + 4) + 4 * PD_ATTN_RPW * 64) * sizeof(float); }
static size_t attn_lds(int N) { return ((size_t)(2 * N + 4) * (DH + 4) + 4 * 64) * sizeof(float); }      // pd_attn_kernel
