// pd_weight_prep.hip -- creation-time weight preparation shared by the denoiser paths and the ViT (declarations: pd_weight_prep.h).
#include "pd_weight_prep.h"

#include <algorithm>
#include <math.h>

#include "pd_denoiser_dev.h"   // pd_first_col_all
#include "pd_gemm_stream.h"    // pd_split_word, pd_split_word_h

// --------------------------------------------------------------------------------------------
// weight repack: W[Nout][K] (row stride ldw, first column koff) -> MFMA-fragment order (zero padded), optionally with a LayerNorm
// gamma folded in as a column scale (W' = W diag(gamma): LN(x) W^T = xhat (W diag(gamma))^T + W beta)
//   NT = 32 (v_mfma_f32_32x32x2_f32):  Wp[nt][kc][lane][4] = W[nt*32 + (l & 31)][kc*8  + 4*(l >> 5) + e]
//   NT = 16 (v_mfma_f32_16x16x4_f32):  Wp[nt][kc][lane][4] = W[nt*16 + (l & 15)][kc*16 + 4*(l >> 4) + e]
// --------------------------------------------------------------------------------------------
__global__ void pd_repack_kernel(const float *__restrict__ W, int Nout, int K, int ldw, int koff, int KC, float *__restrict__ Wp,
                                 size_t total, int first_perm, int nt_width, const float *__restrict__ colscale) {
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int e = idx & 3;
        const int l = (idx >> 2) & 63;
        const size_t rest = idx >> 8;
        const int kc = (int)(rest % KC);
        const int nt = (int)(rest / KC);
        int n, k;
        if (nt_width == 32) {
            n = nt * 32 + (l & 31);
            k = kc * 8 + 4 * (l >> 5) + e;
        } else {
            n = nt * 16 + (l & 15);
            k = kc * 16 + 4 * (l >> 4) + e;
        }
        if (first_perm) k = pd_first_col_all(k);
        float v = (n < Nout && k < K) ? W[(size_t)n * ldw + koff + k] : 0.0f;
        if (colscale && k < K) v *= colscale[k];
        Wp[idx] = v;
    }
}

// b'[n] = b[n] + sum_k W[n][k] beta[k]   (the LayerNorm shift folded into the following bias)
__global__ void pd_fold_bias_kernel(const float *__restrict__ W, const float *__restrict__ beta, const float *__restrict__ b,
                                    int Nout, int K, float *__restrict__ out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= Nout) return;
    float a = 0.0f;
    for (int k = 0; k < K; ++k) a = fmaf(W[(size_t)n * K + k], beta[k], a);
    out[n] = b[n] + a;
}

// W[n][k] * gamma[k] -> Wf (row-major copy with the LayerNorm scale folded in)
__global__ void pd_scale_cols_kernel(const float *__restrict__ W, const float *__restrict__ gamma, int K, size_t total, float *__restrict__ Wf) {
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x)
        Wf[idx] = gamma ? W[idx] * gamma[idx % K] : W[idx];
}

// W[n][k] * gamma[k] -> split and packed in MFMA fragment order: [n / 32][k / 16][hi | lo][lane] x 16 B, lane = (n % 32) +
// 32 * ((k / 8) % 2), 8 consecutive k per lane: one wave-wide 16-byte load is 1 KB contiguous
// f16: fp16 halves of w * scale instead of bf16 halves of w
__global__ void pd_frag_split_kernel(const float *__restrict__ W, const float *__restrict__ gamma, int K, size_t total, uint4 *__restrict__ out,
                                     int f16, float scale) {
    const int KS = K / 16;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int lane = (int)(idx & 63);
        const size_t t = idx >> 6;
        const int ks = (int)(t % KS), nt = (int)(t / KS);
        const int n = nt * 32 + (lane & 31), k0 = ks * 16 + 8 * (lane >> 5);
        unsigned w[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = W[(size_t)n * K + k0 + e];
            w[e] = f16 ? pd_split_word_h(v * scale) : pd_split_word(gamma ? v * gamma[k0 + e] : v);
        }
        uint4 hi, lo;
        hi.x = __builtin_amdgcn_perm(w[1], w[0], 0x05040100u); lo.x = __builtin_amdgcn_perm(w[1], w[0], 0x07060302u);
        hi.y = __builtin_amdgcn_perm(w[3], w[2], 0x05040100u); lo.y = __builtin_amdgcn_perm(w[3], w[2], 0x07060302u);
        hi.z = __builtin_amdgcn_perm(w[5], w[4], 0x05040100u); lo.z = __builtin_amdgcn_perm(w[5], w[4], 0x07060302u);
        hi.w = __builtin_amdgcn_perm(w[7], w[6], 0x05040100u); lo.w = __builtin_amdgcn_perm(w[7], w[6], 0x07060302u);
        out[(t * 2) * 64 + lane] = hi;
        out[(t * 2 + 1) * 64 + lane] = lo;
    }
}

// --------------------------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------------------------
PdDevAllocs::~PdDevAllocs() {
    for (void *p : ptrs) (void)hipFree(p);
}

int PdDevAllocs::alloc_bytes(void **p, size_t bytes, bool zero) {
    PD_HIP_CHECK(hipMalloc(p, bytes));
    ptrs.push_back(*p);
    if (zero) PD_HIP_CHECK(hipMemset(*p, 0, bytes));
    return PD_OK;
}

void PdDevAllocs::release(void *p) {
    if (!p) return;
    (void)hipFree(p);
    const auto it = std::find(ptrs.begin(), ptrs.end(), p);
    if (it != ptrs.end()) ptrs.erase(it);
}

static int null_weight(const char *who) {
    pd_set_error("%s: a weight pointer is NULL", who);
    return PD_ERR_INVALID_ARG;
}

int PdDevAllocs::copy(float **dst, const float *src, size_t n) {
    if (!src) return null_weight(who);
    PD_TRY(alloc(dst, n));
    PD_HIP_CHECK(hipMemcpy(*dst, src, n * sizeof(float), hipMemcpyDeviceToDevice));
    return PD_OK;
}

int PdDevAllocs::pack(float **dst, const float *W, int Nout, int K, int Kpad, int nt, const float *gamma, int first_perm, int ldw, int koff) {
    if (!W) return null_weight(who);
    const int NT = (Nout + nt - 1) / nt, KC = Kpad / (nt == 32 ? 8 : 16);
    const size_t total = (size_t)NT * KC * 256;
    PD_TRY(alloc(dst, total));
    hipLaunchKernelGGL(pd_repack_kernel, dim3(512), dim3(256), 0, 0, W, Nout, K, ldw ? ldw : K, koff, KC, *dst, total, first_perm, nt, gamma);
    PD_HIP_CHECK(hipGetLastError());
    return PD_OK;
}

int PdDevAllocs::fold_bias(float **dst, const float *W, const float *beta, const float *b, int Nout, int K) {
    if (!W || !beta || !b) return null_weight(who);
    PD_TRY(alloc(dst, Nout));
    hipLaunchKernelGGL(pd_fold_bias_kernel, dim3((Nout + 127) / 128), dim3(128), 0, 0, W, beta, b, Nout, K, *dst);
    PD_HIP_CHECK(hipGetLastError());
    return PD_OK;
}

int PdDevAllocs::rowmajor(float **dst, const float *W, int Nout, int K, const float *gamma) {
    if (!W) return null_weight(who);
    const size_t total = (size_t)Nout * K;
    PD_TRY(alloc(dst, total));
    hipLaunchKernelGGL(pd_scale_cols_kernel, dim3(512), dim3(256), 0, 0, W, gamma, K, total, *dst);
    PD_HIP_CHECK(hipGetLastError());
    return PD_OK;
}

int PdDevAllocs::planes(unsigned **dst, const float *W, int Nout, int K, const float *gamma, bool f16, int ew) {
    if (!W) return null_weight(who);
    const size_t total = (size_t)(Nout / 32) * (K / 16) * 64;   // one thread per (32-column tile, 16-k step, lane)
    PD_TRY(alloc(dst, (size_t)Nout * K));
    hipLaunchKernelGGL(pd_frag_split_kernel, dim3(512), dim3(256), 0, 0, W, gamma, K, total, (uint4 *)*dst, f16 ? 1 : 0, ldexpf(1.0f, ew));
    PD_HIP_CHECK(hipGetLastError());
    return PD_OK;
}

// fp16 keeps 11 bits and five exponent bits, so every operand of the fp16-plane GEMMs (the denoiser's PD_OPT_DENOISER_SPLIT = 2, the ViT's
// default at >= 1 024 rows) gets a POWER-OF-TWO scale, exact to apply and to undo, fixed at creation from bounds that hold for every input:
//   * LayerNorm output without affine: sum of squares <= D, so |x^| <= sqrt(D).  Its exponent is the caller's: 2^9 in the denoiser
//     (D = 512, |x^| <= 22.6: <= 11 585), 2^floor(log2(32768 / sqrt(384))) = 2^10 in the ViT;
//   * a Linear fed by it: |x^ . w + b| <= sqrt(D) ||w||_2 + |b| (Cauchy-Schwarz) -- the V rows the attention averages (a convex
//     combination: same bound) and the hidden rows, of which ReLU / GELU keep |act(v)| <= |v|;     scale 2^floor(log2(32768 / bound))
//   * weights (LayerNorm gamma folded): 2^floor(log2(16384 / max |w|)).
// Nothing can overflow (fp16 max 65 504), and hi + lo keeps 22 bits for every value above 2^-18 of its bound.  Weights with inf / NaN
// have no bound: the callers keep them on the exact-fp32 kernels, which propagate the values like the reference does.
int pd_floor_log2_ratio(double cap, double v) {
    if (!(v > 0.0)) return 0;
    double e = floor(log2(cap / v));                       // clamped as a double: the cast below is always defined
    e = e < -60.0 ? -60.0 : (e > 60.0 ? 60.0 : e);
    return (int)e;
}

int pd_plane_exponents(const float *qkv_w, const float *qkv_b, const float *out_w, const float *ff1_w, const float *ff1_b,
                       const float *ff2_w, int D, int F, PdPlaneExps *e, bool *finite) {
    std::vector<float> w, b;
    auto fetch = [&](const float *Wf, const float *bias, int Nout, int K) -> int {
        w.resize((size_t)Nout * K);
        PD_HIP_CHECK(hipMemcpy(w.data(), Wf, w.size() * sizeof(float), hipMemcpyDeviceToHost));
        if (bias) {
            b.resize(Nout);
            PD_HIP_CHECK(hipMemcpy(b.data(), bias, b.size() * sizeof(float), hipMemcpyDeviceToHost));
        }
        return PD_OK;
    };
    bool ok = true;
    auto max_abs = [&]() { double m = 0; for (float v : w) { ok = ok && isfinite(v); m = fmax(m, fabs((double)v)); } return m; };
    auto row_bound = [&](int r0, int r1, int K) {            // max over rows of sqrt(D) ||w_r||_2 + |b_r|
        double bound = 0;
        for (int r = r0; r < r1; ++r) {
            double q = 0;
            for (int k = 0; k < K; ++k) q += (double)w[(size_t)r * K + k] * w[(size_t)r * K + k];
            bound = fmax(bound, sqrt((double)D) * sqrt(q) + fabs((double)b[r]));
            ok = ok && isfinite(q) && isfinite(b[r]);
        }
        return bound;
    };
    PD_HIP_CHECK(hipDeviceSynchronize());
    PD_TRY(fetch(qkv_w, qkv_b, 3 * D, D));
    e->ctx = pd_floor_log2_ratio(32768.0, row_bound(2 * D, 3 * D, D));
    e->qkv = pd_floor_log2_ratio(16384.0, max_abs());
    PD_TRY(fetch(out_w, nullptr, D, D));
    e->out = pd_floor_log2_ratio(16384.0, max_abs());
    PD_TRY(fetch(ff1_w, ff1_b, F, D));
    e->hid = pd_floor_log2_ratio(32768.0, row_bound(0, F, D));
    e->ff1 = pd_floor_log2_ratio(16384.0, max_abs());
    PD_TRY(fetch(ff2_w, nullptr, D, F));
    e->ff2 = pd_floor_log2_ratio(16384.0, max_abs());
    *finite = ok;
    return PD_OK;
}
