// pd_gemm_small.h -- the small-batch GEMM of the default-shape denoiser (fewer than PD_STREAM_MIN_ROWS token rows): the kernel, its launch
// with the per-GEMM 32- / 16-wide tile choice, and the -DPD_DEN_STAMPS latency stamps that the small-batch chain's kernels share.
//
// GEMM structure (M = B*N tokens is tiny: 20..1280; weights are [out,in] row-major = "B^T"):
//   * one workgroup (4 waves) per 32x32 output tile; the four waves split K (each SIMD's matrix
//     pipe works on a quarter of K) and their accumulators are summed through LDS in fixed order;
//   * the 32 activation rows are staged once in LDS in full 128-B lines (row stride K+4 floats:
//     ds_read_b128 fragment reads are conflict-free) with LayerNorm / the harmonic+time+z
//     embedding fused into the staging pass, so no normalised activations ever touch HBM;
//   * weights are re-packed at engine creation into MFMA-fragment order
//     Wp[n_tile][k_chunk][lane][4] so every wave-level load is one fully coalesced 1 KiB line
//     streamed straight to VGPRs (each weight byte is read by exactly one wave per M-tile);
//   * bias / ReLU / residual are fused into the epilogue.
#pragma once
#include "pd_denoiser_dev.h"

// --------------------------------------------------------------------------------------------
// fused 32x32-tile GEMM:  C[m, n] = epi( sum_k A'[m, k] * W[n, k] + bias[n] )
//   AMODE 0: A' = A                      (plain rows of a [M, K] activation)
//   AMODE 1: A' = LayerNorm(A) (K = 512) (norm_first encoder layer, eps 1e-5)
//   AMODE 2: A' = [z | t_emb | harmonic(x) | x | pivot | 0 0]  (K = 704, denoiser.py:56-68; the engine's column order pd_first_col_all)
//   AMODE 3: AMODE 2 with one timestep per token row: t_emb is row t_row[m] of the whole time table (pd_denoise_step_t, pd_p_losses)
//   EPI   0: + bias     1: relu(+ bias)     2: + bias + residual (in place on C)
// --------------------------------------------------------------------------------------------
// -DPD_DEN_STAMPS (tools/den_small_legs.py; never in the product build): every launch of the small-batch chain records, from lane 0 of
// wave 0 of its block 0, the constant 100 MHz clock (s_memrealtime: comparable across kernels and CUs) at the legs of its latency chain
#ifdef PD_DEN_STAMPS
#define PD_STAMP(ptr, i)                                                                          \
    do {                                                                                          \
        if ((ptr) && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) (ptr)[i] = (long long)__builtin_amdgcn_s_memrealtime(); \
    } while (0)
#define PD_STAMP_DRAIN() asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory")
#else
#define PD_STAMP(ptr, i) do { } while (0)
#define PD_STAMP_DRAIN() do { } while (0)
#endif
struct GemmArgs {
#ifdef PD_DEN_STAMPS
    long long *stamps;     // [8] of this launch, or null
#endif
    const float *A;        // [M, K] (AMODE 0/1)
    const float *Wp;       // packed weights
    const float *bias;     // [Nout]
    float *C;              // [M, Nout]
    // AMODE 2
    const float *x, *z, *temb;   // x [M,9], z [M,384], temb [128] (row of the table for this t; AMODE 3: the whole table [T,128])
    int n_frames;
    int M, Nout;
    int MT;                // number of 32-row M tiles (XCD-aware block mapping)
    const int *t_row;      // AMODE 3: [M] timestep of every token row, already inside [0, T)
};

template <int K, int AMODE, int EPI, int NT>
__global__ __launch_bounds__(256) void pd_gemm_kernel(GemmArgs g) {
    constexpr int LDA = K + 4;            // padded row stride (floats): conflict-free ds_read_b128
    constexpr int CW = (NT == 32) ? 8 : 16;   // k-chunk width per float4 fragment load
    constexpr int KC = K / CW;
    constexpr int CPW = KC / 4;           // chunks per wave (split-K over the 4 waves)
    constexpr int NB = (CPW > 16) ? 2 : 1;   // weight batches held in registers
    constexpr int BATCH = CPW / NB;
    constexpr int NACC = (NT == 32) ? 16 : 8;
    static_assert(KC % 4 == 0 && CPW % NB == 0, "chunk batching");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *As = lds;                      // [32][LDA]; later aliased by the cross-wave reduction
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#ifdef PD_DEN_STAMPS
    long long *const stamps = g.stamps;
    PD_STAMP(stamps, 0);                  // entered
#endif
    // XCD-aware tile mapping (guide T1): the dispatcher places block id on XCD id % 8; all M-tiles that share
    // an N-tile are given ids with the same id % 8, so each weight tile is fetched into ONE L2 once and the
    // other M-tile workgroups hit it there (the naive (m + MT*n) order spread them over MT different XCDs
    // and re-fetched every weight byte MT times).  Needs (Nout / NT) % 8 == 0 -- true for every layer here.
    const int bid = blockIdx.x, slot = bid >> 3;
    const int ntile = (bid & 7) + 8 * (slot / g.MT), mtile = slot % g.MT;
    const int m0 = mtile * 32, n0 = ntile * NT;
    const float4 *wp = (const float4 *)g.Wp + ((size_t)ntile * KC + (size_t)wave * CPW) * 64 + lane;

    // ---- weights first: the whole first batch of this wave's fragments goes in flight before the
    // activation staging, so the HBM/MALL latency of the weight stream hides under it --------------
    float4 w0[BATCH];
#pragma unroll
    for (int c = 0; c < BATCH; ++c) w0[c] = wp[(size_t)c * 64];
    // ... and the bias the epilogue adds (requested behind the two barriers below it is a dependent L2 round trip at the very end: -3.5 us per
    // step at B = 1).  The residual values (EPI 2) stay where they are: requested up here they cost +4 us per kernel (measured, tools/den_ab.py).
    constexpr int RPW = NACC / 4;          // accumulator registers finished per wave
    const int col = n0 + ((NT == 32) ? (lane & 31) : (lane & 15));
    const float bias = g.bias[col];

    // ---- stage the 32 activation rows (fused LN / embedding); no predicated loads ---------------
    {
        const int r = tid >> 3, sub = tid & 7;
        const int m = m0 + r;
        const bool live = m < g.M;
        const int mr = live ? m : g.M - 1;   // clamp: padded rows load a valid row and are zeroed
        float *dst = As + r * LDA;
        if constexpr (AMODE == 2 || AMODE == 3) {
            // engine column order (pd_first_col_all): z | t_emb | harmonic | x | pivot | pad
            const float4 *zr = (const float4 *)(g.z + (size_t)mr * ZD);
            const float4 *te = (const float4 *)g.temb;
            if constexpr (AMODE == 3) te += (size_t)g.t_row[mr] * 32;      // this row's own timestep: the same 128 values a single-t launch stages
            float4 zv[ZD / 32], tv[4];
#pragma unroll
            for (int i = 0; i < ZD / 32; ++i) zv[i] = zr[sub + 8 * i];
#pragma unroll
            for (int i = 0; i < 4; ++i) tv[i] = te[sub + 8 * i];
            float xv[9];
#pragma unroll
            for (int d = 0; d < 9; ++d) xv[d] = g.x[(size_t)mr * 9 + d];
            const float keep = live ? 1.0f : 0.0f;
#pragma unroll
            for (int i = 0; i < ZD / 32; ++i) {
                float4 v = zv[i];
                v.x *= keep; v.y *= keep; v.z *= keep; v.w *= keep;
                *(float4 *)(dst + 4 * (sub + 8 * i)) = v;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float4 v = tv[i];
                v.x *= keep; v.y *= keep; v.z *= keep; v.w *= keep;
                *(float4 *)(dst + 384 + 4 * (sub + 8 * i)) = v;
            }
            // harmonic embedding: idx = s*90 + d*10 + k -> sin(x_d * 2^k + s * pi/2)  (pytorch3d 0.7.x)
            for (int idx = sub; idx < 180; idx += 8) {
                const int s = idx / 90, rem = idx - s * 90, d = rem / 10, kk = rem - d * 10;
                float xd = xv[0];
#pragma unroll
                for (int q = 1; q < 9; ++q) xd = (d == q) ? xv[q] : xd;
                const float e = xd * (float)(1 << kk);
                dst[512 + idx] = keep * sinf(s ? e + 1.5707963267948966f : e);
            }
            if (sub == 0) {
#pragma unroll
                for (int d = 0; d < 9; ++d) dst[692 + d] = keep * xv[d];
                dst[701] = (live && (m % g.n_frames == 0)) ? 1.0f : 0.0f;   // pivot one-hot on frame 0
                dst[702] = 0.0f;
                dst[703] = 0.0f;
            }
        } else if constexpr (AMODE == 1) {
            // LayerNorm without affine: gamma is folded into the packed weights, beta into the bias
            static_assert(AMODE != 1 || K == 512, "LayerNorm staging is built for d_model = 512");
            float4 v[K / 32];
            const float4 *src = (const float4 *)(g.A + (size_t)mr * K);
#pragma unroll
            for (int i = 0; i < K / 32; ++i) v[i] = src[sub + 8 * i];
            float s = 0.0f;
#pragma unroll
            for (int i = 0; i < K / 32; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
            const float mean = pd_sum8(s) * (1.0f / K);
            float q = 0.0f;
#pragma unroll
            for (int i = 0; i < K / 32; ++i) {
                const float a = v[i].x - mean, b2 = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
                q += (a * a + b2 * b2) + (c * c + d * d);
            }
            const float rstd = live ? 1.0f / sqrtf(pd_sum8(q) * (1.0f / K) + 1e-5f) : 0.0f;
#pragma unroll
            for (int i = 0; i < K / 32; ++i) {
                float4 o;
                o.x = (v[i].x - mean) * rstd;
                o.y = (v[i].y - mean) * rstd;
                o.z = (v[i].z - mean) * rstd;
                o.w = (v[i].w - mean) * rstd;
                *(float4 *)(dst + 4 * (sub + 8 * i)) = o;
            }
        } else {
            const float4 *src = (const float4 *)(g.A + (size_t)mr * K);
            const float keep = live ? 1.0f : 0.0f;
            constexpr int NV = K / 32;
            constexpr int VB = NV < 16 ? NV : 16;        // loads in flight per pass
            static_assert(NV % VB == 0, "passes of VB float4 per thread");
#pragma unroll
            for (int i0 = 0; i0 < NV; i0 += VB) {
                float4 v[VB];
#pragma unroll
                for (int i = 0; i < VB; ++i) v[i] = src[sub + 8 * (i0 + i)];
#pragma unroll
                for (int i = 0; i < VB; ++i) {
                    float4 o = v[i];
                    o.x *= keep; o.y *= keep; o.z *= keep; o.w *= keep;
                    *(float4 *)(dst + 4 * (sub + 8 * (i0 + i))) = o;
                }
            }
        }
    }
    PD_STAMP(stamps, 1);                  // this thread's share of the A rows loaded (arrived from L2 / MALL), normalised, written to LDS
    __syncthreads();
    PD_STAMP(stamps, 2);                  // every wave's share staged
#ifdef PD_DEN_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    PD_STAMP(stamps, 3);                  // ... and the first batch of weight fragments + the bias have landed (stamps build only: the wait)
#endif

    // ---- split-K MFMA loop: wave w owns k-chunks [w*CPW, (w+1)*CPW) --------------------------
    float4 w1[NB == 2 ? BATCH : 1];
    if constexpr (NB == 2) {
#pragma unroll
        for (int c = 0; c < BATCH; ++c) w1[c] = wp[(size_t)(BATCH + c) * 64];
        __builtin_amdgcn_sched_barrier(0);   // keep the second batch's loads ahead of the first MFMAs
    }
    float accv[NACC];
    if constexpr (NT == 32) {
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
        const float *arow = As + (lane & 31) * LDA + wave * CPW * 8 + 4 * (lane >> 5);
#pragma unroll
        for (int c = 0; c < CPW; ++c) {
            const float4 wf = (c < BATCH) ? w0[c < BATCH ? c : 0] : w1[(NB == 2 && c >= BATCH) ? c - BATCH : 0];
            const float4 af = *(const float4 *)(arow + c * 8);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.x, wf.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.y, wf.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.z, wf.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af.w, wf.w, acc, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) accv[i] = acc[i];
    } else {
        // two 16x16 tiles (rows 0-15, 16-31) share each weight fragment; independent accumulators
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        const float *arow = As + (lane & 15) * LDA + wave * CPW * 16 + 4 * (lane >> 4);
#pragma unroll
        for (int c = 0; c < CPW; ++c) {
            const float4 wf = (c < BATCH) ? w0[c < BATCH ? c : 0] : w1[(NB == 2 && c >= BATCH) ? c - BATCH : 0];
            const float4 a0 = *(const float4 *)(arow + c * 16);
            const float4 a1 = *(const float4 *)(arow + 16 * LDA + c * 16);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, wf.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, wf.x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, wf.y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, wf.y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, wf.z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, wf.z, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, wf.w, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, wf.w, acc1, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            accv[i] = acc0[i];
            accv[4 + i] = acc1[i];
        }
    }
    PD_STAMP(stamps, 4);                  // this wave's MFMA chain issued (its results are awaited by the stores below)
    __syncthreads();   // every wave is done reading As; reuse it for the reduction

    // ---- cross-wave reduction in fixed order + fused epilogue ---------------------------------
    float *red = lds;   // [4][NACC][64]
#pragma unroll
    for (int i = 0; i < NACC; ++i) red[(wave * NACC + i) * 64 + lane] = accv[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        const int reg = wave * RPW + i;
        float v = red[(0 * NACC + reg) * 64 + lane];
        v += red[(1 * NACC + reg) * 64 + lane];
        v += red[(2 * NACC + reg) * 64 + lane];
        v += red[(3 * NACC + reg) * 64 + lane];
        v += bias;
        int row;
        if constexpr (NT == 32) row = m0 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
        else row = m0 + 16 * (reg >> 2) + 4 * (lane >> 4) + (reg & 3);
        if (row < g.M) {
            float *cp = g.C + (size_t)row * g.Nout + col;
            if constexpr (EPI == 1) v = pd_relu(v);
            if constexpr (EPI == 2) v += *cp;
            *cp = v;
        }
    }
    PD_STAMP(stamps, 5);                  // reduced + epilogue issued
    PD_STAMP_DRAIN();
    PD_STAMP(stamps, 6);                  // the stores have left the CU (stamps build only: the wait)
}

// one GEMM launch; the tile width is chosen per problem: 16-wide tiles double the workgroup count (and
// halve each wave's serial MFMA chain) whenever 32-wide tiles would leave most of the 256 CUs idle
#ifdef PD_DEN_STAMPS
static long long *g_den_stamps = nullptr;      // [PD_DEN_STAMP_SLOTS][8], device memory; the slot of the next small-batch launch
static int g_den_stamp_slot = 0;
#define PD_DEN_STAMP_SLOTS 256
static long long *next_stamp_slot() {
    if (!g_den_stamps) {
        if (hipMalloc((void **)&g_den_stamps, sizeof(long long) * 8 * PD_DEN_STAMP_SLOTS) != hipSuccess) return nullptr;
        (void)hipMemset(g_den_stamps, 0, sizeof(long long) * 8 * PD_DEN_STAMP_SLOTS);
    }
    long long *p = g_den_stamps + 8 * (g_den_stamp_slot % PD_DEN_STAMP_SLOTS);
    g_den_stamp_slot += 1;
    return p;
}
// out[n_slots][8]: the stamps of the last launches (slot = launch index mod 256); restarts the slot counter
extern "C" int pd_debug_den_stamps(long long *out, int n_slots) {
    if (!out || n_slots <= 0 || n_slots > PD_DEN_STAMP_SLOTS || !g_den_stamps) return PD_ERR_INVALID_ARG;
    PD_HIP_CHECK(hipDeviceSynchronize());
    PD_HIP_CHECK(hipMemcpy(out, g_den_stamps, sizeof(long long) * 8 * n_slots, hipMemcpyDeviceToHost));
    PD_HIP_CHECK(hipMemset(g_den_stamps, 0, sizeof(long long) * 8 * PD_DEN_STAMP_SLOTS));
    g_den_stamp_slot = 0;
    return PD_OK;
}
#endif
template <int K, int AMODE, int EPI>
static void launch_gemm(GemmArgs &g, float *const wp[2], int MT, int wide_min, hipStream_t s) {
    const int tiles32 = MT * (g.Nout / 32);
    g.MT = MT;
#ifdef PD_DEN_STAMPS
    g.stamps = next_stamp_slot();
#endif
    // the XCD-aware block mapping of pd_gemm_kernel needs a multiple of 8 N-tiles (128-wide _last.0 has only 4 of 32)
    if (tiles32 >= wide_min && (g.Nout / 32) % 8 == 0) {
        g.Wp = wp[0];
        hipLaunchKernelGGL((pd_gemm_kernel<K, AMODE, EPI, 32>), dim3(MT * (g.Nout / 32)), dim3(256), 32 * (K + 4) * 4, s, g);
    } else {
        g.Wp = wp[1];
        hipLaunchKernelGGL((pd_gemm_kernel<K, AMODE, EPI, 16>), dim3(MT * (g.Nout / 16)), dim3(256), 32 * (K + 4) * 4, s, g);
    }
}
