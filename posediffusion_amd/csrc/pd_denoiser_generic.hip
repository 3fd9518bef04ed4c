// pd_denoiser_generic.hip -- the shape-generic denoiser path: every Denoiser / TransformerEncoderWrapper configuration of the
// family documented on pd_weights (include/pd_engine.h), pre-norm or post-norm, with or without the pivot column.
//
// The default shape (d_model 512, 4 heads, FF 1024, z 384, hidden 128, pre-norm, pivot) keeps its own kernels (pd_denoiser.hip); this
// path serves every other legal configuration, and the default one too under PD_WEIGHTS_GENERIC (comparison / testing).
//
// Numerics: everything is fp32.  The GEMMs are pd_gemm_dma (pd_gemm_stream.h): 64 x 64 tiles on the exact-fp32 matrix instruction
// v_mfma_f32_32x32x2_f32, A and W staged into LDS by LDS-DMA.  That kernel needs K a multiple of 32 and N_out a multiple of 64, so every
// width here is padded once at creation: weights are copied into zero-padded row-major [N_out_pad, K_pad] arrays (the layout that kernel
// stages), biases into zero-padded vectors, and the activations live in arrays of the padded width whose padding columns hold zeros for
// the whole life of the engine (zeroed at creation; every kernel writes only the live columns, or zeros).  Padded products are then
// exact zeros and the live columns are the unpadded GEMM.
//
//   _first       embedding rows [harmonic(x) 180 | x 9 | t_emb 128 | z | pivot?] in the reference's column order (pd_gen_embed_kernel),
//                then one GEMM over all K = 189 + 128 + z_dim + pivot columns.  The z columns are NOT hoisted out of the step (unlike the
//                default path's pd_denoiser_prepare): pd_denoiser_prepare is a no-op for a generic engine.
//   encoder      pre-norm : h += out(attn(LN1(h)));  h += W2 relu(W1 LN2(h))
//                post-norm: h = LN1(h + out(attn(h))); h = LN2(h + W2 relu(W1 h))      (nn.TransformerEncoderLayer, eps 1e-5, ReLU)
//                LayerNorm over the runtime width with its affine (pd_gen_ln_kernel); attention one workgroup per (sequence, head)
//                for a runtime head dim and N <= 64 (pd_gen_attn_kernel); above 64 frames, or under PD_OPT_DENOISER_LONG_ATTN = 1, the
//                key-tiled pd_gen_attn_long_kernel (pd_attn_long.h), up to PD_MAX_DENOISER_FRAMES = 256.
//   _last        _last.0 as a GEMM, then LayerNorm(hidden) -> ReLU -> Linear(hidden, 9) fused with the DDPM update (pd_gen_tail_kernel,
//                the outputs of pd_tail_kernel).
#include "pd_denoiser_dev.h"
#include "pd_gemm_stream.h"
#include "pd_attn_long.h"

#include <math.h>
#include <string.h>

#define PD_GEN_FIRST_FIXED 317      // harmonic (180) + x (9) + t_emb (128): the columns of _first before z
#define PD_GEN_ATTN_THREADS 256

static inline int pd_round_up(int v, int m) { return ((v + m - 1) / m) * m; }

struct PdGenLayer {
    float *norm1_w, *norm1_b, *norm2_w, *norm2_b;   // [d] each
    float *qkv_w, *qkv_b;                           // [3 Dp, Dp]: q | k | v sections of Dp rows each, [3 Dp]
    float *out_w, *out_b;                           // [Dp, Dp], [Dp]
    float *ff1_w, *ff1_b;                           // [Fp, Dp], [Fp]
    float *ff2_w, *ff2_b;                           // [Dp, Fp], [Dp]
};

struct PdGenericDen {
    int d = 0, nhead = 0, hd = 0, ff = 0, z = 0, hid = 0, layers = 0, timesteps = 0;
    int post_norm = 0, pivot = 1;
    int Dp = 0, Fp = 0, Kf = 0, Kfp = 0, Hp = 0;    // padded widths (multiples of 64; Kfp: of 32)
    int m_cap = 0;
    float *t_table = nullptr;                       // [T, 128] time embeddings (pd_time_table)
    float *first_w = nullptr, *first_b = nullptr;   // [Dp, Kfp], [Dp]
    PdGenLayer L[PD_MAX_LAYERS];
    float *last0_w = nullptr, *last0_b = nullptr;   // [Hp, Dp], [Hp]
    float *last_ln_w = nullptr, *last_ln_b = nullptr, *last3_w = nullptr, *last3_b = nullptr;   // [hid], [hid], [9, hid], [9]
    float *emb = nullptr, *h = nullptr, *hn = nullptr, *qkv = nullptr, *ctx = nullptr, *ffa = nullptr, *hida = nullptr;
    PdDevAllocs mem{"pd_engine_create"};            // every buffer above, zero-filled
};

// --------------------------------------------------------------------------------------------
// creation-time copies: W [sections x src_rows, K] row-major -> [sections x dst_rows, Kp], zero padded (rows and columns)
// --------------------------------------------------------------------------------------------
__global__ void pd_gen_pad_kernel(const float *__restrict__ W, int src_rows, int K, float *__restrict__ out, int dst_rows, int Kp,
                                  int sections) {
    const size_t total = (size_t)sections * dst_rows * Kp;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % Kp);
        const size_t r = idx / Kp;
        const int sec = (int)(r / dst_rows), rr = (int)(r % dst_rows);
        out[idx] = (rr < src_rows && c < K) ? W[((size_t)sec * src_rows + rr) * K + c] : 0.0f;
    }
}

// --------------------------------------------------------------------------------------------
// _first's input rows in the reference's column order (models/denoiser.py:56-68):
//   [0,180) harmonic(x) | [180,189) x | [189,317) t_emb(t) | [317,317+z) z | pivot (frame 0 of a sequence; when enabled) | 0 padding
// the harmonic expressions are those of pd_embed_rows_kernel (pytorch3d HarmonicEmbedding, n = 10, append_input)
// TSEQ: one timestep per sequence -- temb is the whole table [T, 128] and row m takes its row t_row[m] (else temb is the row of the launch's t)
// --------------------------------------------------------------------------------------------
template <bool TSEQ>
__global__ __launch_bounds__(256) void pd_gen_embed_kernel(const float *__restrict__ x, const float *__restrict__ z, const float *__restrict__ temb,
                                                           int M, int n_frames, int zdim, int pivot, int Kfp, float *__restrict__ out,
                                                           const int *__restrict__ t_row) {
    const size_t total = (size_t)M * Kfp;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(idx % Kfp);
        const int row = (int)(idx / Kfp);
        float v = 0.0f;
        if (c < 180) {
            const int s = c / 90, rem = c - s * 90, d = rem / 10, kk = rem - d * 10;
            const float a = x[(size_t)row * 9 + d] * (float)(1 << kk);
            v = sinf(s ? a + 1.5707963267948966f : a);
        } else if (c < 189) {
            v = x[(size_t)row * 9 + (c - 180)];
        } else if (c < PD_GEN_FIRST_FIXED) {
            v = TSEQ ? temb[(size_t)t_row[row] * 128 + (c - 189)] : temb[c - 189];
        } else if (c < PD_GEN_FIRST_FIXED + zdim) {
            v = z[(size_t)row * zdim + (c - PD_GEN_FIRST_FIXED)];
        } else if (pivot && c == PD_GEN_FIRST_FIXED + zdim) {
            v = (row % n_frames == 0) ? 1.0f : 0.0f;
        }
        out[idx] = v;
    }
}

// --------------------------------------------------------------------------------------------
// LayerNorm over the first D columns of rows of stride ld, with its affine, eps 1e-5: one wave per row, two passes over the row for the
// statistics, a third for the output.  out may be in (post-norm: in place) -- every lane writes only the columns it has just read itself.
// --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pd_gen_ln_kernel(const float *in, float *out, const float *__restrict__ gamma,
                                                        const float *__restrict__ beta, int M, int D, int ld) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;
    const float *src = in + (size_t)row * ld;
    float s = 0.0f;
    for (int c = lane; c < D; c += 64) s += src[c];
    const float mean = pd_wave_sum(s) / (float)D;
    float q = 0.0f;
    for (int c = lane; c < D; c += 64) {
        const float e = src[c] - mean;
        q = fmaf(e, e, q);
    }
    const float rstd = 1.0f / sqrtf(pd_wave_sum(q) / (float)D + 1e-5f);
    float *dst = out + (size_t)row * ld;
    for (int c = lane; c < D; c += 64) {
        const float v = src[c];
        dst[c] = (v - mean) * rstd * gamma[c] + beta[c];
    }
}

// --------------------------------------------------------------------------------------------
// attention: softmax(q k^T / sqrt(hd)) v for one (sequence, head) per workgroup, N <= 64 frames, head dim hd (multiple of 4, <= 256).
// K and V of the head are staged in LDS ([N][hd + 4] each); wave w owns the query rows w, w + 4, ...: lane j scores key j (an fmaf chain
// over hd), softmax is a wave reduction, then lane l accumulates output dims l, l + 64, ... with the probabilities broadcast by shuffles.
// qkv rows: [q (Dp) | k (Dp) | v (Dp)], head h at columns h hd ..; ctx rows of stride Dp (columns >= d are never written).
// --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PD_GEN_ATTN_THREADS) void pd_gen_attn_kernel(const float *__restrict__ qkv, float *__restrict__ ctx, int N, int nhead,
                                                                          int hd, int Dp, float scale) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int LD = hd + 4;
    float *Kk = lds, *V = lds + (size_t)N * LD;
    const int b = blockIdx.x / nhead, h = blockIdx.x % nhead, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t ld3 = (size_t)3 * Dp;
    const float *base = qkv + (size_t)b * N * ld3 + (size_t)h * hd;
    const int hd4 = hd / 4;
    for (int idx = tid; idx < N * hd4; idx += PD_GEN_ATTN_THREADS) {
        const int j = idx / hd4, d4 = idx - j * hd4;
        const float *row = base + (size_t)j * ld3 + 4 * d4;
        *(float4 *)(Kk + j * LD + 4 * d4) = *(const float4 *)(row + Dp);
        *(float4 *)(V + j * LD + 4 * d4) = *(const float4 *)(row + 2 * Dp);
    }
    __syncthreads();
    const int jj = lane < N ? lane : N - 1;
    const float4 *kb = (const float4 *)(Kk + jj * LD);
    for (int i = wave; i < N; i += PD_GEN_ATTN_THREADS / 64) {
        const float4 *qa = (const float4 *)(base + (size_t)i * ld3);
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
        const float p = e * (1.0f / pd_wave_sum(e));
        float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int j = 0; j < N; ++j) {
            const float pj = __shfl(p, j, 64);
            const float *vr = V + j * LD;
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                const int dd = lane + 64 * cc;
                if (dd < hd) o[cc] = fmaf(pj, vr[dd], o[cc]);
            }
        }
        float *out = ctx + (size_t)(b * N + i) * Dp + (size_t)h * hd;
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            const int dd = lane + 64 * cc;
            if (dd < hd) out[dd] = o[cc];
        }
    }
}
static size_t pd_gen_attn_lds(int N, int hd) { return (size_t)2 * N * (hd + 4) * sizeof(float); }
#define PD_GEN_MAX_HD 256           // the family's head-dim bound (pd_denoiser_generic_shape_ok)

// --------------------------------------------------------------------------------------------
// tail: LayerNorm(hidden) -> ReLU -> Linear(hidden, 9) (_last.1 .. 3) fused with predict_start_from_noise / q_posterior / the sample
// update (gaussian_diffuser.py:190-209, :280): one wave per token, lane l holds hidden values l, l + 64, ... (hidden <= 1024).
// --------------------------------------------------------------------------------------------
#define PD_GEN_TAIL_PER 16          // 1024 / 64
struct PdGenTailArgs {
    const float *hid;               // [M, Hp] = _last.0 output (bias included)
    const float *lnw, *lnb, *w3, *b3;
    const float *x, *noise;         // [M, 9]; noise may be null
    float *eps_out, *mean_out, *x0_out, *xnext_out;
    float c_recip, c_recipm1, coef1, coef2, sigma;
    int M, H, Hp, pred_x0;
    const int *nf;                  // frame counts per sequence (pd_engine_set_frame_counts) or null; n_frames rows per sequence block
    int n_frames;
    // TSEQ (pd_denoise_step_t, pd_p_losses): every row's own coefficients from device tables, and the loss (gaussian_diffuser.py:312-327)
    const int *t_row;                     // [M]
    const float *c_recip_tab, *c_recipm1_tab;
    const float *target;                  // [M, 9], null without loss_out
    float *loss_out;
    int loss_type;                        // 1 = l1, 2 = l2
};
template <bool TSEQ>
__global__ __launch_bounds__(256) void pd_gen_tail_kernel(PdGenTailArgs g) {
    const int lane = threadIdx.x & 63, m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= g.M) return;
    if (!TSEQ && g.nf) {            // a padding row (wave-uniform): every output gets +0, nothing of the row is read
        const int sb = m / g.n_frames;
        if (m - sb * g.n_frames >= g.nf[sb]) {
            if (lane < 9) {
                const size_t at = (size_t)m * 9 + lane;
                if (g.eps_out) g.eps_out[at] = 0.0f;
                if (g.x0_out) g.x0_out[at] = 0.0f;
                if (g.mean_out) g.mean_out[at] = 0.0f;
                if (g.xnext_out) g.xnext_out[at] = 0.0f;
            }
            return;
        }
    }
    const float *row = g.hid + (size_t)m * g.Hp;
    float v[PD_GEN_TAIL_PER];
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < PD_GEN_TAIL_PER; ++i) {
        const int c = lane + 64 * i;
        v[i] = c < g.H ? row[c] : 0.0f;
        s += v[i];
    }
    const float mean = pd_wave_sum(s) / (float)g.H;
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < PD_GEN_TAIL_PER; ++i) {
        const float e = lane + 64 * i < g.H ? v[i] - mean : 0.0f;
        q = fmaf(e, e, q);
    }
    const float rstd = 1.0f / sqrtf(pd_wave_sum(q) / (float)g.H + 1e-5f);
#pragma unroll
    for (int i = 0; i < PD_GEN_TAIL_PER; ++i) {
        const int c = lane + 64 * i;
        v[i] = c < g.H ? pd_relu((v[i] - mean) * rstd * g.lnw[c] + g.lnb[c]) : 0.0f;
    }
    float e = 0.0f;
    for (int o = 0; o < 9; ++o) {
        float part = 0.0f;
#pragma unroll
        for (int i = 0; i < PD_GEN_TAIL_PER; ++i) {
            const int c = lane + 64 * i;
            if (c < g.H) part = fmaf(v[i], g.w3[(size_t)o * g.H + c], part);
        }
        part = pd_wave_sum(part);
        e = (lane == o) ? part : e;
    }
    if (lane < 9) {
        const size_t at = (size_t)m * 9 + lane;
        const float xv = g.x[at];
        e += g.b3[lane];
        if constexpr (TSEQ) {
            const int t = g.t_row[m];
            if (g.eps_out) g.eps_out[at] = e;
            if (g.x0_out) g.x0_out[at] = g.pred_x0 ? e : g.c_recip_tab[t] * xv - g.c_recipm1_tab[t] * e;   // :316, :319
            if (g.loss_out) {
                const float d = e - g.target[at];
                g.loss_out[at] = g.loss_type == 2 ? d * d : fabsf(d);                                      // :323, reduction "none"
            }
            return;
        }
        const float x0 = g.pred_x0 ? e : g.c_recip * xv - g.c_recipm1 * e;   // gaussian_diffuser.py:190-194, :221-227
        const float mu = g.coef1 * x0 + g.coef2 * xv;                     // :201-205
        if (g.eps_out) g.eps_out[at] = e;
        if (g.x0_out) g.x0_out[at] = x0;
        if (g.mean_out) g.mean_out[at] = mu;
        if (g.xnext_out) g.xnext_out[at] = g.noise ? mu + g.sigma * g.noise[at] : mu;   // :280
    }
}

// --------------------------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------------------------
// [sections x src_rows, K] -> [sections x dst_rows, Kp], zero padded (a bias: K = Kp = 1)
static int gen_pad(PdGenericDen *G, float **dst, const float *W, int src_rows, int K, int dst_rows, int Kp, int sections = 1) {
    if (!W) {
        pd_set_error("pd_engine_create: a weight pointer is NULL");
        return PD_ERR_INVALID_ARG;
    }
    const size_t total = (size_t)sections * dst_rows * Kp;
    PD_TRY(G->mem.alloc(dst, total, true));
    hipLaunchKernelGGL(pd_gen_pad_kernel, dim3(512), dim3(256), 0, 0, W, src_rows, K, *dst, dst_rows, Kp, sections);
    PD_HIP_CHECK(hipGetLastError());
    return PD_OK;
}

bool pd_denoiser_generic_shape_ok(const pd_weights *w, char *why, size_t why_len) {
    const int d = w->d_model, nh = w->nhead;
    const char *msg = nullptr;
    if (d < 32 || d > 2048 || d % 32) msg = "d_model must be a multiple of 32 in [32, 2048]";
    else if (nh < 1 || d % nh) msg = "nhead must divide d_model";
    else if ((d / nh) % 4 || d / nh < 8 || d / nh > 256) msg = "the head dim d_model / nhead must be a multiple of 4 in [8, 256]";
    else if (w->dim_ff < 1 || w->dim_ff > 8192) msg = "dim_feedforward must be in [1, 8192]";
    else if (w->num_layers < 1 || w->num_layers > PD_MAX_LAYERS) msg = "num_encoder_layers must be in [1, PD_MAX_LAYERS = 16]";
    else if (w->z_dim < 1 || w->z_dim > 4096) msg = "z_dim must be in [1, 4096]";
    else if (w->mlp_hidden < 1 || w->mlp_hidden > 1024) msg = "mlp_hidden_dim must be in [1, 1024]";
    else if (w->n_harmonic != 10 || w->t_emb_dim != 256) msg = "the pose / time embeddings must be the reference's (10 harmonics, t_emb 256)";
    if (msg && why) snprintf(why, why_len, "%s (d_model=%d nhead=%d ff=%d layers=%d z=%d hidden=%d harmonics=%d t_emb=%d)", msg, d, nh, w->dim_ff,
                             w->num_layers, w->z_dim, w->mlp_hidden, w->n_harmonic, w->t_emb_dim);
    return msg == nullptr;
}

int pd_denoiser_generic_create(pd_engine *eng, const pd_weights *w) {
    char why[256];
    if (!pd_denoiser_generic_shape_ok(w, why, sizeof(why))) {
        pd_set_error("pd_engine_create: unsupported denoiser configuration: %s", why);
        return PD_ERR_UNSUPPORTED;
    }
    PdGenericDen *G = new PdGenericDen();
    eng->gden = G;
    G->d = w->d_model;
    G->nhead = w->nhead;
    G->hd = w->d_model / w->nhead;
    G->ff = w->dim_ff;
    G->z = w->z_dim;
    G->hid = w->mlp_hidden;
    G->layers = w->num_layers;
    G->timesteps = w->timesteps;
    G->post_norm = (w->reserved & PD_WEIGHTS_POST_NORM) ? 1 : 0;
    G->pivot = (w->reserved & PD_WEIGHTS_NO_PIVOT) ? 0 : 1;
    G->Dp = pd_round_up(G->d, 64);
    G->Fp = pd_round_up(G->ff, 64);
    G->Kf = PD_GEN_FIRST_FIXED + G->z + G->pivot;
    G->Kfp = pd_round_up(G->Kf, 32);
    G->Hp = pd_round_up(G->hid, 64);
    G->m_cap = eng->max_B * eng->max_N;
    // pd_gemm_dma addresses its rows with 32-bit byte offsets: the widest activation array must stay below 2 GiB
    const int widest = std::max(std::max(3 * G->Dp, G->Fp), G->Kfp);
    if ((size_t)G->m_cap * widest * sizeof(float) >= ((size_t)1 << 31)) {
        pd_set_error("pd_engine_create: max_B x max_N = %d token rows at a %d-float activation row exceed the generic denoiser's 2 GiB "
                     "per-array limit", G->m_cap, widest);
        return PD_ERR_UNSUPPORTED;
    }
    // the attention kernel's dynamic-LDS limit is a per-process attribute of the kernel, shared by every engine: it is set to the family's
    // bound (N = 64 frames, head dim 256: 133 120 bytes), never from this engine's shape, so a later engine cannot lower it below what an
    // earlier one launches with
    PD_TRY(pd_set_lds(pd_gen_attn_kernel, pd_gen_attn_lds(PD_MAX_FRAMES, PD_GEN_MAX_HD)));
    PD_TRY(pd_set_lds(pd_gen_attn_long_kernel<0>, pd_attn_long_lds(PD_MAX_DENOISER_FRAMES, PD_GEN_MAX_HD)));

    PD_TRY(G->mem.alloc(&G->t_table, (size_t)w->timesteps * 128, true));
    PD_TRY(pd_time_table(w, G->t_table));
    const int d = G->d, Dp = G->Dp, Fp = G->Fp;
    PD_TRY(gen_pad(G, &G->first_w, w->first_w, d, G->Kf, Dp, G->Kfp));
    PD_TRY(gen_pad(G, &G->first_b, w->first_b, d, 1, Dp, 1));
    for (int l = 0; l < G->layers; ++l) {
        const pd_layer_weights &s = w->layers[l];
        PdGenLayer &L = G->L[l];
        PD_TRY(gen_pad(G, &L.norm1_w, s.norm1_w, d, 1, d, 1));
        PD_TRY(gen_pad(G, &L.norm1_b, s.norm1_b, d, 1, d, 1));
        PD_TRY(gen_pad(G, &L.norm2_w, s.norm2_w, d, 1, d, 1));
        PD_TRY(gen_pad(G, &L.norm2_b, s.norm2_b, d, 1, d, 1));
        PD_TRY(gen_pad(G, &L.qkv_w, s.in_proj_w, d, d, Dp, Dp, 3));     // q | k | v: three sections of d rows -> Dp rows
        PD_TRY(gen_pad(G, &L.qkv_b, s.in_proj_b, d, 1, Dp, 1, 3));
        PD_TRY(gen_pad(G, &L.out_w, s.out_proj_w, d, d, Dp, Dp));
        PD_TRY(gen_pad(G, &L.out_b, s.out_proj_b, d, 1, Dp, 1));
        PD_TRY(gen_pad(G, &L.ff1_w, s.linear1_w, G->ff, d, Fp, Dp));
        PD_TRY(gen_pad(G, &L.ff1_b, s.linear1_b, G->ff, 1, Fp, 1));
        PD_TRY(gen_pad(G, &L.ff2_w, s.linear2_w, d, G->ff, Dp, Fp));
        PD_TRY(gen_pad(G, &L.ff2_b, s.linear2_b, d, 1, Dp, 1));
    }
    PD_TRY(gen_pad(G, &G->last0_w, w->last0_w, G->hid, d, G->Hp, Dp));
    PD_TRY(gen_pad(G, &G->last0_b, w->last0_b, G->hid, 1, G->Hp, 1));
    PD_TRY(gen_pad(G, &G->last_ln_w, w->last_ln_w, G->hid, 1, G->hid, 1));
    PD_TRY(gen_pad(G, &G->last_ln_b, w->last_ln_b, G->hid, 1, G->hid, 1));
    PD_TRY(gen_pad(G, &G->last3_w, w->last3_w, 9, G->hid, 9, G->hid));
    PD_TRY(gen_pad(G, &G->last3_b, w->last3_b, 9, 1, 9, 1));
    const size_t rows = (size_t)G->m_cap;
    PD_TRY(G->mem.alloc(&G->emb, rows * G->Kfp, true));
    PD_TRY(G->mem.alloc(&G->h, rows * Dp, true));
    PD_TRY(G->mem.alloc(&G->hn, rows * Dp, true));
    PD_TRY(G->mem.alloc(&G->qkv, rows * 3 * Dp, true));
    PD_TRY(G->mem.alloc(&G->ctx, rows * Dp, true));
    PD_TRY(G->mem.alloc(&G->ffa, rows * Fp, true));
    PD_TRY(G->mem.alloc(&G->hida, rows * G->Hp, true));
    PD_HIP_CHECK(hipDeviceSynchronize());
    return PD_OK;
}

void pd_denoiser_generic_destroy(pd_engine *eng) {
    delete eng->gden;
    eng->gden = nullptr;
}

int pd_denoiser_generic_launch(pd_engine *eng, const float *x, const float *z, int t, int B, int N, float *eps_out, float *mean_out,
                               float *x0_out, const float *noise, float *x_next_out, hipStream_t s, const PdTSeq *ts) {
    PdGenericDen *G = eng->gden;
    if (!x || !z || B <= 0 || N <= 0 || B > eng->max_B || N > eng->max_N || N > PD_MAX_DENOISER_FRAMES || t < 0 || t >= G->timesteps) {
        pd_set_error("denoiser: invalid arguments (B=%d N=%d t=%d; max_B=%d max_N=%d, N <= %d, 0 <= t < %d)", B, N, t, eng->max_B, eng->max_N,
                     PD_MAX_DENOISER_FRAMES, G->timesteps);
        return PD_ERR_INVALID_ARG;
    }
    const int *nf = nullptr;        // frame counts per sequence: the key-tiled attention kernel takes them, the tail zeroes the padding rows
    if (!ts) PD_TRY(pd_frame_counts(eng, B, N, "denoiser", &nf));
    const int M = B * N, Dp = G->Dp, Fp = G->Fp;
    const int rows_blocks = (M + 3) / 4;
    {
        const size_t total = (size_t)M * G->Kfp;
        const int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
        if (ts) hipLaunchKernelGGL(pd_gen_embed_kernel<true>, dim3(blocks), dim3(256), 0, s, x, z, G->t_table, M, N, G->z, G->pivot, G->Kfp, G->emb, ts->t_row);
        else hipLaunchKernelGGL(pd_gen_embed_kernel<false>, dim3(blocks), dim3(256), 0, s, x, z, G->t_table + (size_t)t * 128, M, N, G->z, G->pivot, G->Kfp, G->emb, nullptr);
    }
    pd_gemm_dma<0>(G->emb, G->Kfp, G->first_w, G->Kfp, G->first_b, G->h, M, Dp, s);
    const float scale = 1.0f / sqrtf((float)G->hd);
    const size_t attn_lds = pd_gen_attn_lds(N, G->hd);
    // more than 64 frames (or PD_OPT_DENOISER_LONG_ATTN = 1): K and V through LDS in tiles of 64 keys
    const bool long_attn = N > PD_MAX_FRAMES || eng->den_long_attn || nf;
    const auto attention = [&]() {
        if (long_attn)
            hipLaunchKernelGGL(pd_gen_attn_long_kernel<0>, dim3(B * G->nhead, (N + PD_ATTN_LONG_ROWS - 1) / PD_ATTN_LONG_ROWS), dim3(256),
                               pd_attn_long_lds(N, G->hd), s, G->qkv, G->ctx, N, G->nhead, G->hd, Dp, scale, nf);
        else
            hipLaunchKernelGGL(pd_gen_attn_kernel, dim3(B * G->nhead), dim3(PD_GEN_ATTN_THREADS), attn_lds, s, G->qkv, G->ctx, N, G->nhead, G->hd, Dp, scale);
    };
    for (int l = 0; l < G->layers; ++l) {
        const PdGenLayer &L = G->L[l];
        if (!G->post_norm) {
            // h += out_proj(attn(LN1(h)));  h += W2 relu(W1 LN2(h))
            hipLaunchKernelGGL(pd_gen_ln_kernel, dim3(rows_blocks), dim3(256), 0, s, G->h, G->hn, L.norm1_w, L.norm1_b, M, G->d, Dp);
            pd_gemm_dma<0>(G->hn, Dp, L.qkv_w, Dp, L.qkv_b, G->qkv, M, 3 * Dp, s);
            attention();
            PD_HIP_CHECK(hipGetLastError());      // the one launch whose dynamic LDS depends on the call's shape: its status, not a later one's
            pd_gemm_dma<2>(G->ctx, Dp, L.out_w, Dp, L.out_b, G->h, M, Dp, s);
            hipLaunchKernelGGL(pd_gen_ln_kernel, dim3(rows_blocks), dim3(256), 0, s, G->h, G->hn, L.norm2_w, L.norm2_b, M, G->d, Dp);
            pd_gemm_dma<1>(G->hn, Dp, L.ff1_w, Dp, L.ff1_b, G->ffa, M, Fp, s);
            pd_gemm_dma<2>(G->ffa, Fp, L.ff2_w, Fp, L.ff2_b, G->h, M, Dp, s);
        } else {
            // h = LN1(h + out_proj(attn(h)));  h = LN2(h + W2 relu(W1 h))
            pd_gemm_dma<0>(G->h, Dp, L.qkv_w, Dp, L.qkv_b, G->qkv, M, 3 * Dp, s);
            attention();
            PD_HIP_CHECK(hipGetLastError());
            pd_gemm_dma<2>(G->ctx, Dp, L.out_w, Dp, L.out_b, G->h, M, Dp, s);
            hipLaunchKernelGGL(pd_gen_ln_kernel, dim3(rows_blocks), dim3(256), 0, s, G->h, G->h, L.norm1_w, L.norm1_b, M, G->d, Dp);
            pd_gemm_dma<1>(G->h, Dp, L.ff1_w, Dp, L.ff1_b, G->ffa, M, Fp, s);
            pd_gemm_dma<2>(G->ffa, Fp, L.ff2_w, Fp, L.ff2_b, G->h, M, Dp, s);
            hipLaunchKernelGGL(pd_gen_ln_kernel, dim3(rows_blocks), dim3(256), 0, s, G->h, G->h, L.norm2_w, L.norm2_b, M, G->d, Dp);
        }
    }
    pd_gemm_dma<0>(G->h, Dp, G->last0_w, Dp, G->last0_b, G->hida, M, G->Hp, s);
    PdGenTailArgs ta;
    memset(&ta, 0, sizeof(ta));
    ta.hid = G->hida; ta.lnw = G->last_ln_w; ta.lnb = G->last_ln_b; ta.w3 = G->last3_w; ta.b3 = G->last3_b;
    ta.x = x; ta.noise = noise;
    ta.eps_out = eps_out; ta.mean_out = mean_out; ta.x0_out = x0_out; ta.xnext_out = x_next_out;
    ta.c_recip = eng->c_recip[t]; ta.c_recipm1 = eng->c_recipm1[t]; ta.coef1 = eng->coef1[t]; ta.coef2 = eng->coef2[t];
    ta.sigma = expf(0.5f * eng->logvar[t]);
    ta.M = M; ta.H = G->hid; ta.Hp = G->Hp; ta.pred_x0 = eng->pred_x0;
    ta.nf = nf; ta.n_frames = N;
    if (ts) {
        ta.t_row = ts->t_row; ta.c_recip_tab = eng->d_c_recip; ta.c_recipm1_tab = eng->d_c_recipm1;
        ta.target = ts->target; ta.loss_out = ts->loss_out; ta.loss_type = ts->loss_type;
        hipLaunchKernelGGL(pd_gen_tail_kernel<true>, dim3(rows_blocks), dim3(256), 0, s, ta);
    } else {
        hipLaunchKernelGGL(pd_gen_tail_kernel<false>, dim3(rows_blocks), dim3(256), 0, s, ta);
    }
    PD_HIP_CHECK(hipGetLastError());
    return PD_OK;
}
