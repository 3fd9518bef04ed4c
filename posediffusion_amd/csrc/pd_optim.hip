// pd_optim.hip -- the optimiser step of training (include/pd_engine_optim.h): global-norm gradient clipping and AdamW.
//
// Replaces (paths relative to the reference's pose_diffusion/): train.py:247-250, accelerator.clip_grad_norm_(model.parameters(), 1.0) and
// torch.optim.AdamW.step() -- a dozen passes of PyTorch's multi-tensor kernels over the 258 live tensors -- by two passes.
//
// Launches of one pd_optim_adamw_step with clipping, in stream order:
//   pd_opt_set_entries_kernel x ceil(n / 64)   the call's tensor table, by value in kernel arguments (the pointers change every step)
//   pd_opt_set_hypers_kernel  x ceil(k / 64)   the fp32 scalars of the k distinct (group, step) pairs (k = 1 in an ordinary step)
//   pd_opt_sqnorm_kernel                        one fp64 partial sum of g^2 per chunk
//   pd_opt_finish_norm_kernel (one workgroup)   partial sums -> norm (fp32) and clip coefficient, both on the device
//   pd_opt_adamw_kernel                         g * coef, m, v, p per element
// Work decomposition: tensor i of n elements is ceil(n / PD_OPTIM_CHUNK) chunks; chunk c of the call belongs to the tensor with the largest
// first_chunk <= c (a binary search in the table, uniform per workgroup) and a workgroup takes chunks blockIdx.x, + gridDim.x, ...  A
// thread's elements of a chunk and the order it adds them in are the same on the 16-byte and on the 4-byte load path, and all arithmetic is
// in pd_opt_sq4 / pd_opt_adamw_elem, which both paths call: the two give the same bits.  This unit is built with -ffp-contract=on (Makefile)
// and every fused multiply-add below is written as one, so the backend has no choice to make.
#include "pd_internal.h"
#include "../../include/pd_engine_optim.h"

#include <cmath>
#include <math.h>
#include <string.h>

#define PD_OPT_THREADS 256
#define PD_OPT_MAX_GRID 2048      // a memory-bound kernel: 8 workgroups on each of 256 CUs, the chunks beyond are strided over
#define PD_OPT_TAB_CHUNK 64       // table entries per upload launch (kernel arguments hold 4 KiB)
#define PD_OPT_QUADS (PD_OPTIM_CHUNK / 4 / PD_OPT_THREADS)   // 16-byte groups of one thread in a whole chunk
static_assert(PD_OPTIM_CHUNK % (4 * PD_OPT_THREADS) == 0, "a whole chunk is a whole number of 16-byte groups per thread");

struct PdOptEntry {
    float *p, *g, *m, *v;
    long long numel;
    int first_chunk;              // chunks of the tensors before this one
    int hyper;                    // index of its (group, step) scalars
};
struct PdOptHyper {
    float decay;                  // 1 - lr wd
    float b1, omb1, b2, omb2;     // beta, 1 - beta
    float step_size;              // lr / (1 - beta1^step)
    float bc2_sqrt;               // sqrt(1 - beta2^step)
    float eps;
};
struct PdOptEntryChunk {
    PdOptEntry e[PD_OPT_TAB_CHUNK];
};
struct PdOptHyperChunk {
    PdOptHyper h[PD_OPT_TAB_CHUNK];
};

struct pd_optimizer {
    int max_tensors = 0, max_chunks = 0;
    long long max_numel = 0;
    PdOptEntry *d_tab = nullptr;      // [max_tensors]
    PdOptHyper *d_hyp = nullptr;      // [max_tensors]
    double *d_part = nullptr;         // [max_chunks]
    float *d_coef = nullptr;          // [1] the clip coefficient of the call in flight
    std::vector<PdOptEntry> tab;      // host staging of one call (reserved at creation)
    std::vector<PdOptHyper> hyp;
    std::vector<long long> hyp_key;   // group << 32 | step
};

// ---- kernels ----------------------------------------------------------------------------------
__global__ void pd_opt_set_entries_kernel(PdOptEntryChunk v, int first, int n, PdOptEntry *__restrict__ dst) {
    const int i = threadIdx.x;
    if (i < n) dst[first + i] = v.e[i];
}

__global__ void pd_opt_set_hypers_kernel(PdOptHyperChunk v, int first, int n, PdOptHyper *__restrict__ dst) {
    const int i = threadIdx.x;
    if (i < n) dst[first + i] = v.h[i];
}

// the tensor of chunk c: the last entry whose first_chunk is <= c (entries hold at least one chunk each, first_chunk[0] = 0)
__device__ __forceinline__ int pd_opt_find(const PdOptEntry *__restrict__ tab, int n, int c) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].first_chunk <= c) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// elements i .. i + 3 of a chunk of len values; those past the end read as 0
__device__ __forceinline__ void pd_opt_load4_tail(const float *__restrict__ p, int i, int len, float x[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = (i + j < len) ? p[i + j] : 0.0f;
}
__device__ __forceinline__ void pd_opt_load4_vec(const float *__restrict__ p, int i, float x[4]) {
    const float4 q = *reinterpret_cast<const float4 *>(p + i);
    x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
}
__device__ __forceinline__ void pd_opt_store4_tail(float *__restrict__ p, int i, int len, const float x[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (i + j < len) p[i + j] = x[j];
}
__device__ __forceinline__ void pd_opt_store4_vec(float *__restrict__ p, int i, const float x[4]) {
    *reinterpret_cast<float4 *>(p + i) = make_float4(x[0], x[1], x[2], x[3]);
}

// acc + x0^2 + x1^2 + x2^2 + x3^2, left to right; a square of an fp32 value is exact in fp64
__device__ __forceinline__ double pd_opt_sq4(double acc, const float x[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double d = (double)x[j];
        acc = fma(d, d, acc);
    }
    return acc;
}

// the sum of `acc` over the workgroup in a fixed order (xor butterfly inside a wave, then the four waves in order), valid in thread 0
__device__ __forceinline__ double pd_opt_block_sum(double acc, double *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, PD_WAVE);
    const int wave = threadIdx.x / PD_WAVE;
    __syncthreads();                       // red's readers of the previous turn are done
    if ((threadIdx.x & (PD_WAVE - 1)) == 0) red[wave] = acc;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < PD_OPT_THREADS / PD_WAVE; ++w) s += red[w];
    return s;
}

// the chunk c of the call: its tensor, where it starts in it and how many values it holds
struct PdOptChunk {
    int ti, len;
    long long off;
};
__device__ __forceinline__ PdOptChunk pd_opt_chunk(const PdOptEntry *__restrict__ tab, int n, int c) {
    PdOptChunk k;
    k.ti = pd_opt_find(tab, n, c);
    k.off = (long long)(c - tab[k.ti].first_chunk) * PD_OPTIM_CHUNK;
    const long long rest = tab[k.ti].numel - k.off;
    k.len = rest < PD_OPTIM_CHUNK ? (int)rest : PD_OPTIM_CHUNK;
    return k;
}
__device__ __forceinline__ bool pd_opt_aligned16(const void *p) { return ((unsigned long long)p & 15ull) == 0; }

// part[c] = sum of g^2 over chunk c, in fp64.  Thread t adds the 16-byte groups t, t + 256, ... of the chunk, each left to right.
__global__ __launch_bounds__(PD_OPT_THREADS) void pd_opt_sqnorm_kernel(const PdOptEntry *__restrict__ tab, int n, int n_chunks,
                                                                       double *__restrict__ part) {
    __shared__ double red[PD_OPT_THREADS / PD_WAVE];
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const PdOptChunk k = pd_opt_chunk(tab, n, c);
        const float *__restrict__ g = tab[k.ti].g + k.off;
        double acc = 0.0;
        float x[4];
        if (k.len == PD_OPTIM_CHUNK && pd_opt_aligned16(g)) {
#pragma unroll
            for (int r = 0; r < PD_OPT_QUADS; ++r) {
                pd_opt_load4_vec(g, 4 * ((int)threadIdx.x + r * PD_OPT_THREADS), x);
                acc = pd_opt_sq4(acc, x);
            }
        } else {
            for (int i = 4 * (int)threadIdx.x; i < k.len; i += 4 * PD_OPT_THREADS) {
                pd_opt_load4_tail(g, i, k.len, x);
                acc = pd_opt_sq4(acc, x);
            }
        }
        const double s = pd_opt_block_sum(acc, red);
        if (threadIdx.x == 0) part[c] = s;
    }
}

// One workgroup: thread t adds partial sums t, t + 256, ... in that order, then the fixed order of pd_opt_block_sum.  norm = fp32 rounding
// of the fp64 square root; coef = clamp(max_norm / (norm + 1e-6), max = 1) as torch.clamp does it: a NaN stays a NaN (fminf would give 1).
__global__ __launch_bounds__(PD_OPT_THREADS) void pd_opt_finish_norm_kernel(const double *__restrict__ part, int n_chunks, float max_norm,
                                                                            float *__restrict__ norm_out, float *__restrict__ coef_out) {
    __shared__ double red[PD_OPT_THREADS / PD_WAVE];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_chunks; i += PD_OPT_THREADS) acc += part[i];
    const double s = pd_opt_block_sum(acc, red);
    if (threadIdx.x == 0) {
        const float nrm = (float)sqrt(s);
        if (norm_out) *norm_out = nrm;
        const float c = __fdiv_rn(max_norm, __fadd_rn(nrm, 1e-6f));
        *coef_out = c > 1.0f ? 1.0f : c;
    }
}

// the update of one element; `clip` is uniform over the launch
__device__ __forceinline__ void pd_opt_adamw_elem(float &p, float g, float &m, float &v, const PdOptHyper &h, float coef, bool clip) {
    if (clip) g = __fmul_rn(g, coef);
    const float pd = __fmul_rn(p, h.decay);
    const float gs = __fmul_rn(h.omb1, g);
    m = fmaf(h.b1, m, gs);
    const float g2 = __fmul_rn(g, g);
    const float g2s = __fmul_rn(h.omb2, g2);
    v = fmaf(h.b2, v, g2s);
    const float root = __fsqrt_rn(v);
    const float den = __fadd_rn(__fdiv_rn(root, h.bc2_sqrt), h.eps);
    const float q = __fdiv_rn(m, den);
    p = fmaf(-h.step_size, q, pd);
}

__global__ __launch_bounds__(PD_OPT_THREADS) void pd_opt_adamw_kernel(const PdOptEntry *__restrict__ tab, int n, int n_chunks,
                                                                      const PdOptHyper *__restrict__ hyp, const float *__restrict__ coef_in,
                                                                      int clip) {
    const float coef = clip ? *coef_in : 1.0f;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const PdOptChunk k = pd_opt_chunk(tab, n, c);
        const PdOptEntry e = tab[k.ti];
        const PdOptHyper h = hyp[e.hyper];
        float *__restrict__ p = e.p + k.off;
        const float *__restrict__ g = e.g + k.off;
        float *__restrict__ m = e.m + k.off;
        float *__restrict__ v = e.v + k.off;
        float xp[4], xg[4], xm[4], xv[4];
        if (k.len == PD_OPTIM_CHUNK && pd_opt_aligned16(p) && pd_opt_aligned16(g) && pd_opt_aligned16(m) && pd_opt_aligned16(v)) {
#pragma unroll 2
            for (int r = 0; r < PD_OPT_QUADS; ++r) {
                const int i = 4 * ((int)threadIdx.x + r * PD_OPT_THREADS);
                pd_opt_load4_vec(p, i, xp);
                pd_opt_load4_vec(g, i, xg);
                pd_opt_load4_vec(m, i, xm);
                pd_opt_load4_vec(v, i, xv);
#pragma unroll
                for (int j = 0; j < 4; ++j) pd_opt_adamw_elem(xp[j], xg[j], xm[j], xv[j], h, coef, clip != 0);
                pd_opt_store4_vec(p, i, xp);
                pd_opt_store4_vec(m, i, xm);
                pd_opt_store4_vec(v, i, xv);
            }
        } else {
            for (int i = 4 * (int)threadIdx.x; i < k.len; i += 4 * PD_OPT_THREADS) {
                pd_opt_load4_tail(p, i, k.len, xp);
                pd_opt_load4_tail(g, i, k.len, xg);
                pd_opt_load4_tail(m, i, k.len, xm);
                pd_opt_load4_tail(v, i, k.len, xv);
#pragma unroll
                for (int j = 0; j < 4; ++j) pd_opt_adamw_elem(xp[j], xg[j], xm[j], xv[j], h, coef, clip != 0);
                pd_opt_store4_tail(p, i, k.len, xp);
                pd_opt_store4_tail(m, i, k.len, xm);
                pd_opt_store4_tail(v, i, k.len, xv);
            }
        }
    }
}

// grad <- grad * coef in place (pd_optim_clip_grad_norm); a coefficient of exactly 1 changes nothing and is not applied
__global__ __launch_bounds__(PD_OPT_THREADS) void pd_opt_scale_kernel(const PdOptEntry *__restrict__ tab, int n, int n_chunks,
                                                                      const float *__restrict__ coef_in) {
    const float coef = *coef_in;
    if (coef == 1.0f) return;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const PdOptChunk k = pd_opt_chunk(tab, n, c);
        float *__restrict__ g = tab[k.ti].g + k.off;
        float x[4];
        if (k.len == PD_OPTIM_CHUNK && pd_opt_aligned16(g)) {
#pragma unroll
            for (int r = 0; r < PD_OPT_QUADS; ++r) {
                const int i = 4 * ((int)threadIdx.x + r * PD_OPT_THREADS);
                pd_opt_load4_vec(g, i, x);
#pragma unroll
                for (int j = 0; j < 4; ++j) x[j] = __fmul_rn(x[j], coef);
                pd_opt_store4_vec(g, i, x);
            }
        } else {
            for (int i = 4 * (int)threadIdx.x; i < k.len; i += 4 * PD_OPT_THREADS) {
                pd_opt_load4_tail(g, i, k.len, x);
#pragma unroll
                for (int j = 0; j < 4; ++j) x[j] = __fmul_rn(x[j], coef);
                pd_opt_store4_tail(g, i, k.len, x);
            }
        }
    }
}

// ---- host -------------------------------------------------------------------------------------
extern "C" int pd_optimizer_create(int max_tensors, int64_t max_numel_total, pd_optimizer **out) {
    if (!out) {
        pd_set_error("pd_optimizer_create: invalid argument out=NULL");
        return PD_ERR_INVALID_ARG;
    }
    *out = nullptr;
    if (max_tensors < 1 || max_numel_total < 1) {
        pd_set_error("pd_optimizer_create: invalid arguments max_tensors=%d max_numel_total=%lld: both must be positive", max_tensors,
                     (long long)max_numel_total);
        return PD_ERR_INVALID_ARG;
    }
    const long long chunks = (long long)(max_numel_total / PD_OPTIM_CHUNK) + max_tensors;   // >= sum of ceil(numel / chunk)
    if (chunks > 0x7fffffffLL) {
        pd_set_error("pd_optimizer_create: max_numel_total=%lld is beyond the limit of 2^31 chunks of %d elements", (long long)max_numel_total,
                     PD_OPTIM_CHUNK);
        return PD_ERR_UNSUPPORTED;
    }
    pd_optimizer *o = new pd_optimizer();
    o->max_tensors = max_tensors;
    o->max_numel = max_numel_total;
    o->max_chunks = (int)chunks;
    o->tab.reserve(max_tensors);
    o->hyp.reserve(max_tensors);
    o->hyp_key.reserve(max_tensors);
    hipError_t e = hipMalloc((void **)&o->d_tab, sizeof(PdOptEntry) * (size_t)max_tensors);
    if (e == hipSuccess) e = hipMalloc((void **)&o->d_hyp, sizeof(PdOptHyper) * (size_t)max_tensors);
    if (e == hipSuccess) e = hipMalloc((void **)&o->d_part, sizeof(double) * (size_t)o->max_chunks);
    if (e == hipSuccess) e = hipMalloc((void **)&o->d_coef, sizeof(float));
    if (e != hipSuccess) {
        pd_set_error("pd_optimizer_create: a HIP call failed: %s", hipGetErrorString(e));
        pd_optimizer_destroy(o);
        return PD_ERR_HIP;
    }
    *out = o;
    return PD_OK;
}

extern "C" void pd_optimizer_destroy(pd_optimizer *o) {
    if (!o) return;
    (void)hipFree(o->d_tab);
    (void)hipFree(o->d_hyp);
    (void)hipFree(o->d_part);
    (void)hipFree(o->d_coef);
    delete o;
}

// Checks the call's tensors and lays out o->tab (tensors of no element hold no chunk and are left out).  need_all: param, exp_avg and
// exp_avg_sq are used as well (pd_optim_adamw_step).  *n_chunks = chunks of the call.
static int opt_layout(pd_optimizer *o, const pd_optim_tensor *t, int n, bool need_all, const char *who, int *n_chunks) {
    if (!o) {
        pd_set_error("%s: invalid argument o=NULL (no optimizer object)", who);
        return PD_ERR_INVALID_ARG;
    }
    if (n < 0 || (n > 0 && !t)) {
        pd_set_error("%s: invalid argument %s", who, n < 0 ? "n < 0" : "t=NULL with n > 0");
        return PD_ERR_INVALID_ARG;
    }
    long long total = 0;
    for (int i = 0; i < n; ++i) {
        if (t[i].numel < 0) {
            pd_set_error("%s: invalid argument t[%d].numel=%lld: must not be negative", who, i, (long long)t[i].numel);
            return PD_ERR_INVALID_ARG;
        }
        if (t[i].numel > 0 && (!t[i].grad || (need_all && (!t[i].param || !t[i].exp_avg || !t[i].exp_avg_sq)))) {
            pd_set_error("%s: invalid argument t[%d]: %s=NULL", who, i,
                         !t[i].grad ? "grad" : !t[i].param ? "param" : !t[i].exp_avg ? "exp_avg" : "exp_avg_sq");
            return PD_ERR_INVALID_ARG;
        }
        total += t[i].numel;
        if (total > o->max_numel) break;
    }
    if (n > o->max_tensors) {
        pd_set_error("%s: n=%d tensors exceed this optimizer's max_tensors=%d (pd_optimizer_create)", who, n, o->max_tensors);
        return PD_ERR_UNSUPPORTED;
    }
    if (total > o->max_numel) {
        pd_set_error("%s: the tensors hold more than this optimizer's max_numel_total=%lld elements (pd_optimizer_create)", who, o->max_numel);
        return PD_ERR_UNSUPPORTED;
    }
    o->tab.clear();
    long long chunks = 0;
    for (int i = 0; i < n; ++i) {
        if (t[i].numel == 0) continue;
        PdOptEntry e;
        e.p = t[i].param; e.g = t[i].grad; e.m = t[i].exp_avg; e.v = t[i].exp_avg_sq;
        e.numel = t[i].numel;
        e.first_chunk = (int)chunks;
        e.hyper = 0;
        o->tab.push_back(e);
        chunks += (t[i].numel + PD_OPTIM_CHUNK - 1) / PD_OPTIM_CHUNK;
    }
    *n_chunks = (int)chunks;   // <= max_chunks by the two checks above
    return PD_OK;
}

static int opt_grid(int n_chunks) { return n_chunks < PD_OPT_MAX_GRID ? n_chunks : PD_OPT_MAX_GRID; }

// the table of the call, by value in kernel arguments: ordered on the stream like every launch that reads it
static void opt_upload(pd_optimizer *o, hipStream_t s) {
    const int n = (int)o->tab.size(), k = (int)o->hyp.size();
    for (int first = 0; first < n; first += PD_OPT_TAB_CHUNK) {
        const int cnt = n - first < PD_OPT_TAB_CHUNK ? n - first : PD_OPT_TAB_CHUNK;
        PdOptEntryChunk c;
        memset(&c, 0, sizeof(c));
        memcpy(c.e, o->tab.data() + first, sizeof(PdOptEntry) * (size_t)cnt);
        hipLaunchKernelGGL(pd_opt_set_entries_kernel, dim3(1), dim3(PD_OPT_TAB_CHUNK), 0, s, c, first, cnt, o->d_tab);
    }
    for (int first = 0; first < k; first += PD_OPT_TAB_CHUNK) {
        const int cnt = k - first < PD_OPT_TAB_CHUNK ? k - first : PD_OPT_TAB_CHUNK;
        PdOptHyperChunk c;
        memset(&c, 0, sizeof(c));
        memcpy(c.h, o->hyp.data() + first, sizeof(PdOptHyper) * (size_t)cnt);
        hipLaunchKernelGGL(pd_opt_set_hypers_kernel, dim3(1), dim3(PD_OPT_TAB_CHUNK), 0, s, c, first, cnt, o->d_hyp);
    }
}

// norm pass + finish: d_coef and *norm_out (nullable) on the device
static void opt_norm(pd_optimizer *o, int n_chunks, double max_norm, float *norm_out, hipStream_t s) {
    if (n_chunks > 0)
        hipLaunchKernelGGL(pd_opt_sqnorm_kernel, dim3(opt_grid(n_chunks)), dim3(PD_OPT_THREADS), 0, s, o->d_tab, (int)o->tab.size(), n_chunks,
                           o->d_part);
    hipLaunchKernelGGL(pd_opt_finish_norm_kernel, dim3(1), dim3(PD_OPT_THREADS), 0, s, o->d_part, n_chunks, (float)max_norm, norm_out, o->d_coef);
}

extern "C" int pd_optim_grad_norm(pd_optimizer *o, const pd_optim_tensor *t, int n, float *norm_out, void *stream) {
    int n_chunks = 0;
    PD_TRY(opt_layout(o, t, n, false, "pd_optim_grad_norm", &n_chunks));
    if (!norm_out) {
        pd_set_error("pd_optim_grad_norm: invalid argument norm_out=NULL");
        return PD_ERR_INVALID_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    o->hyp.clear();
    opt_upload(o, s);
    opt_norm(o, n_chunks, 0.0, norm_out, s);
    PD_HIP_CHECK(hipGetLastError());
    return PD_OK;
}

extern "C" int pd_optim_clip_grad_norm(pd_optimizer *o, const pd_optim_tensor *t, int n, double max_norm, float *norm_out, void *stream) {
    int n_chunks = 0;
    PD_TRY(opt_layout(o, t, n, false, "pd_optim_clip_grad_norm", &n_chunks));
    if (!(max_norm > 0.0)) {
        pd_set_error("pd_optim_clip_grad_norm: invalid argument max_norm=%g: must be positive", max_norm);
        return PD_ERR_INVALID_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    o->hyp.clear();
    opt_upload(o, s);
    opt_norm(o, n_chunks, max_norm, norm_out, s);
    if (n_chunks > 0)
        hipLaunchKernelGGL(pd_opt_scale_kernel, dim3(opt_grid(n_chunks)), dim3(PD_OPT_THREADS), 0, s, o->d_tab, (int)o->tab.size(), n_chunks,
                           o->d_coef);
    PD_HIP_CHECK(hipGetLastError());
    return PD_OK;
}

extern "C" int pd_optim_adamw_step(pd_optimizer *o, const pd_optim_tensor *t, int n, const pd_optim_group *g, int n_groups, double max_norm,
                                   float *norm_out, void *stream) {
    const char *who = "pd_optim_adamw_step";
    int n_chunks = 0;
    PD_TRY(opt_layout(o, t, n, true, who, &n_chunks));
    if (n_groups < 0 || (n > 0 && (!g || n_groups < 1))) {
        pd_set_error("%s: invalid argument %s", who, !g ? "g=NULL" : "n_groups: at least one group is needed");
        return PD_ERR_INVALID_ARG;
    }
    if (max_norm != max_norm) {
        pd_set_error("%s: invalid argument max_norm=NaN", who);
        return PD_ERR_INVALID_ARG;
    }
    for (int j = 0; g && j < n_groups; ++j) {
        const char *bad = nullptr;
        double val = 0.0;
        if (!(g[j].lr >= 0.0) || std::isinf(g[j].lr)) bad = "lr", val = g[j].lr;
        else if (!(g[j].beta1 >= 0.0 && g[j].beta1 < 1.0)) bad = "beta1", val = g[j].beta1;
        else if (!(g[j].beta2 >= 0.0 && g[j].beta2 < 1.0)) bad = "beta2", val = g[j].beta2;
        else if (!(g[j].eps >= 0.0) || std::isinf(g[j].eps)) bad = "eps", val = g[j].eps;
        else if (!(g[j].weight_decay >= 0.0) || std::isinf(g[j].weight_decay)) bad = "weight_decay", val = g[j].weight_decay;
        if (bad) {
            pd_set_error("%s: invalid argument g[%d].%s=%g: lr, eps and weight_decay must be finite and not negative, a beta in [0, 1)", who, j, bad,
                         val);
            return PD_ERR_INVALID_ARG;
        }
    }
    for (int i = 0; i < n; ++i) {
        if (t[i].group < 0 || t[i].group >= n_groups) {
            pd_set_error("%s: invalid argument t[%d].group=%d: outside [0, n_groups=%d)", who, i, (int)t[i].group, n_groups);
            return PD_ERR_INVALID_ARG;
        }
        if (t[i].step < 1) {
            pd_set_error("%s: invalid argument t[%d].step=%d: the step count after this step is at least 1", who, i, (int)t[i].step);
            return PD_ERR_INVALID_ARG;
        }
    }
    // the fp32 scalars of every distinct (group, step) pair, formed in double
    o->hyp.clear();
    o->hyp_key.clear();
    size_t e = 0;
    int last = -1;
    for (int i = 0; i < n; ++i) {
        if (t[i].numel == 0) continue;
        const long long key = ((long long)t[i].group << 32) | (unsigned)t[i].step;
        int idx = -1;
        if (last >= 0 && o->hyp_key[last] == key) idx = last;
        for (int j = 0; idx < 0 && j < (int)o->hyp_key.size(); ++j)
            if (o->hyp_key[j] == key) idx = j;
        if (idx < 0) {
            const pd_optim_group &gg = g[t[i].group];
            const double bc1 = 1.0 - pow(gg.beta1, (double)t[i].step), bc2 = 1.0 - pow(gg.beta2, (double)t[i].step);
            PdOptHyper h;
            h.decay = (float)(1.0 - gg.lr * gg.weight_decay);
            h.b1 = (float)gg.beta1; h.omb1 = (float)(1.0 - gg.beta1);
            h.b2 = (float)gg.beta2; h.omb2 = (float)(1.0 - gg.beta2);
            h.step_size = (float)(gg.lr / bc1);
            h.bc2_sqrt = (float)sqrt(bc2);
            h.eps = (float)gg.eps;
            idx = (int)o->hyp.size();
            o->hyp.push_back(h);
            o->hyp_key.push_back(key);
        }
        last = idx;
        o->tab[e++].hyper = idx;
    }
    hipStream_t s = (hipStream_t)stream;
    const int clip = max_norm > 0.0 ? 1 : 0;
    opt_upload(o, s);
    if (clip || norm_out) opt_norm(o, n_chunks, clip ? max_norm : 0.0, norm_out, s);
    if (n_chunks > 0)
        hipLaunchKernelGGL(pd_opt_adamw_kernel, dim3(opt_grid(n_chunks)), dim3(PD_OPT_THREADS), 0, s, o->d_tab, (int)o->tab.size(), n_chunks,
                           o->d_hyp, o->d_coef, clip);
    PD_HIP_CHECK(hipGetLastError());
    return PD_OK;
}
