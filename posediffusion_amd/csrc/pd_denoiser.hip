// pd_denoiser.hip -- the transformer Denoiser + DDPM posterior update as hand-written gfx950 kernels.
//
// Replaces (paths relative to /root/reference/pose_diffusion/):
//   models/denoiser.py:53-76        Denoiser.forward (embed -> _first -> 8 encoder layers -> _last)
//   models/denoiser.py:79-98        nn.TransformerEncoderLayer, pre-norm, ReLU, eps 1e-5, eval mode
//   util/embedding.py:13-50         TimeStepEmbedding (hoisted into a [T,128] table) + PoseEmbedding
//   models/gaussian_diffuser.py:190-209, :231-246, :280   x0 / posterior mean / sample update
//
// Numerics: everything is fp32.  GEMMs run on the exact-fp32 matrix instruction
// v_mfma_f32_32x32x2_f32 (bitwise an fmaf chain, 157 TF peak) so the engine matches the
// reference's fp32 path to rounding-order differences only (SURVEY.md headline fact 5).
//
// This file is the host side: engine creation, the split-precision weights, and one step's launches.  The kernels are in the headers:
//   pd_gemm_small.h (small batches), pd_gemm_stream.h / pd_gemm_split.h / pd_gemm_strip.h (large batches: exact / split precision / its strip kernel), pd_attn.h,
//   pd_attn_long.h (more than 64 frames) and pd_qkv_attn.h (attention), pd_denoiser_kernels.h (embeddings, tail, probe); pd_denoiser_plan.h decides which of them a step launches.
// One timestep per sequence (pd_denoise_step_t, pd_p_losses) changes _first and the tail only: den_first_small_t, den_first_streamed_t,
// den_tail_t below; the streamed path's per-row-bias GEMM is instantiated in pd_denoiser_first_t.hip.
#include "pd_denoiser_dev.h"
#include "pd_gemm_stream.h"
#include "pd_gemm_strip.h"
#include "pd_qkv_attn.h"
#include "pd_gemm_small.h"
#include "pd_attn.h"
#include "pd_attn_long.h"
#include "pd_denoiser_kernels.h"
#include "pd_denoiser_plan.h"

#include <algorithm>
#include <math.h>
#include <stdlib.h>
#include <string.h>

// --------------------------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------------------------
int pd_time_table(const pd_weights *w, float *table) {
    if (!w->time_w0 || !w->time_b0 || !w->time_w2 || !w->time_b2) {
        pd_set_error("pd_engine_create: a weight pointer is NULL");
        return PD_ERR_INVALID_ARG;
    }
    hipLaunchKernelGGL(pd_time_table_kernel, dim3(w->timesteps), dim3(128), 0, 0, w->time_w0, w->time_b0, w->time_w2, w->time_b2, table);
    PD_HIP_CHECK(hipGetLastError());
    return PD_OK;
}

// the shape the kernels of this file are built for (cfgs/default.yaml); every other legal configuration -- and this one under
// PD_WEIGHTS_GENERIC -- takes the shape-generic path of pd_denoiser_generic.hip
static bool pd_denoiser_default_shape(const pd_weights *w) {
    return w->d_model == DM && w->nhead == NH && w->dim_ff == DFF && w->z_dim == ZD && w->n_harmonic == 10 && w->t_emb_dim == 256 &&
           w->mlp_hidden == HID && w->num_layers >= 1 && w->num_layers <= PD_MAX_LAYERS &&
           !(w->reserved & (PD_WEIGHTS_POST_NORM | PD_WEIGHTS_NO_PIVOT | PD_WEIGHTS_GENERIC));
}

// ---- pd_denoiser_create in steps; their order is the order of the allocations and of the creation-time launches -------------------------
// the weights of the small-batch kernel, re-packed into MFMA-fragment order (pd_gemm_small.h) once per tile width
static int den_create_small_packs(PdDenoiserDev *d, const pd_weights *w) {
    PdDevAllocs &m = d->mem;
    for (int v = 0; v < 2; ++v) {   // v = 0: 32-wide tiles, v = 1: 16-wide tiles
        const int nt = v ? 16 : 32;
        PD_TRY(m.pack(&d->first_wp[v], w->first_w, DM, KFIRST, KFIRST_PAD, nt, nullptr, 1));
        PD_TRY(m.pack(&d->last0_wp[v], w->last0_w, HID, DM, DM, nt, nullptr));
        for (int l = 0; l < w->num_layers; ++l) {
            const pd_layer_weights &s = w->layers[l];
            PdLayerDev &L = d->layers[l];
            // LayerNorm affine folded: W' = W diag(gamma) (packed), b' = b + W beta
            PD_TRY(m.pack(&L.qkv_wp[v], s.in_proj_w, 3 * DM, DM, DM, nt, s.norm1_w));
            PD_TRY(m.pack(&L.out_wp[v], s.out_proj_w, DM, DM, DM, nt, nullptr));
            PD_TRY(m.pack(&L.ff1_wp[v], s.linear1_w, DFF, DM, DM, nt, s.norm2_w));
            PD_TRY(m.pack(&L.ff2_wp[v], s.linear2_w, DM, DFF, DFF, nt, nullptr));
        }
    }
    return PD_OK;
}
// biases (LayerNorm shift folded in), the encoder weights as row-major copies (LayerNorm scale folded in) for the large-batch GEMMs, the tail's weights
static int den_create_biases_rowmajor(PdDenoiserDev *d, const pd_weights *w) {
    PdDevAllocs &m = d->mem;
    PD_TRY(m.copy(&d->first_b, w->first_b, DM));
    for (int l = 0; l < w->num_layers; ++l) {
        const pd_layer_weights &s = w->layers[l];
        PdLayerDev &L = d->layers[l];
        if (!s.norm1_w || !s.norm2_w) {
            pd_set_error("pd_engine_create: a LayerNorm weight pointer is NULL");
            return PD_ERR_INVALID_ARG;
        }
        PD_TRY(m.fold_bias(&L.qkv_b, s.in_proj_w, s.norm1_b, s.in_proj_b, 3 * DM, DM));
        PD_TRY(m.copy(&L.out_b, s.out_proj_b, DM));
        PD_TRY(m.fold_bias(&L.ff1_b, s.linear1_w, s.norm2_b, s.linear1_b, DFF, DM));
        PD_TRY(m.copy(&L.ff2_b, s.linear2_b, DM));
        PD_TRY(m.rowmajor(&L.qkv_wf, s.in_proj_w, 3 * DM, DM, s.norm1_w));
        PD_TRY(m.rowmajor(&L.out_wf, s.out_proj_w, DM, DM, nullptr));
        PD_TRY(m.rowmajor(&L.ff1_wf, s.linear1_w, DFF, DM, s.norm2_w));
        PD_TRY(m.rowmajor(&L.ff2_wf, s.linear2_w, DM, DFF, nullptr));
    }
    PD_TRY(m.copy(&d->last0_b, w->last0_b, HID));
    PD_TRY(m.copy(&d->last_ln_w, w->last_ln_w, HID));
    PD_TRY(m.copy(&d->last_ln_b, w->last_ln_b, HID));
    PD_TRY(m.copy(&d->last3_w, w->last3_w, 9 * HID));
    PD_TRY(m.copy(&d->last3_b, w->last3_b, 9));
    return PD_OK;
}
// activations for m_cap token rows; hn marks an engine large enough for the streamed path
static int den_create_activations(PdDenoiserDev *d) {
    PdDevAllocs &m = d->mem;
    const size_t rows = (size_t)d->m_cap;
    PD_TRY(m.alloc(&d->h, rows * DM));
    PD_TRY(m.alloc(&d->qkv, rows * 3 * DM));
    PD_TRY(m.alloc(&d->ctx, rows * DM));
    PD_TRY(m.alloc(&d->ff, rows * DFF));
    PD_TRY(m.alloc(&d->hid, rows * HID));
    if (rows >= PD_STREAM_MIN_ROWS) PD_TRY(m.alloc(&d->hn, rows * DM));
    return PD_OK;
}
// the streamed path evaluates _first in three pieces (pd_denoiser_dev.h), two of them outside the diffusion steps: its input rows
// (materialised by pd_embed_rows_kernel every step), zproj, and the row-major pieces of _first the GEMMs read
static int den_create_first_pieces(PdDenoiserDev *d, const pd_weights *w) {
    PdDevAllocs &m = d->mem;
    const size_t rows = (size_t)d->m_cap;
    PD_TRY(m.alloc(&d->emb, rows * KFIRST_D));
    PD_TRY(m.alloc(&d->zproj, rows * DM));
    PD_TRY(m.alloc(&d->first_df, (size_t)DM * KFIRST_D));
    PD_TRY(m.alloc(&d->first_zf, (size_t)DM * ZD));
    hipLaunchKernelGGL(pd_first_rowmajor_kernel, dim3((DM * KFIRST_D + 255) / 256), dim3(256), 0, 0, w->first_w, d->first_df, PD_FIRST_D, KFIRST_D);
    hipLaunchKernelGGL(pd_first_rowmajor_kernel, dim3((DM * ZD + 255) / 256), dim3(256), 0, 0, w->first_w, d->first_zf, PD_FIRST_Z, ZD);
    PD_HIP_CHECK(hipGetLastError());
    // the time piece of _first for every step: ttab[t] = W_t t_emb(t)
    PD_TRY(m.alloc(&d->ttab, (size_t)w->timesteps * DM));
    hipLaunchKernelGGL(pd_first_ttab_kernel, dim3(w->timesteps), dim3(DM), 0, 0, w->first_w, d->t_table, d->ttab);
    PD_HIP_CHECK(hipGetLastError());
    return PD_OK;
}
// dynamic LDS beyond 64 KiB is an attribute of the kernel: every kernel of this file that can ask for it, at its largest shape
template <int K, int AMODE, int EPI>
static int den_set_gemm_lds() {     // the 32- / 16-wide pair of a small-batch GEMM shape (launch_gemm chooses between them)
    PD_TRY(pd_set_lds(pd_gemm_kernel<K, AMODE, EPI, 32>, 32 * (K + 4) * 4));
    PD_TRY(pd_set_lds(pd_gemm_kernel<K, AMODE, EPI, 16>, 32 * (K + 4) * 4));
    return PD_OK;
}
static int den_set_lds_attributes() {
    PD_TRY((den_set_gemm_lds<KFIRST_PAD, 2, 0>()));
    PD_TRY((den_set_gemm_lds<KFIRST_PAD, 3, 0>()));
    PD_TRY((den_set_gemm_lds<DM, 1, 0>()));
    PD_TRY((den_set_gemm_lds<DM, 1, 1>()));
    PD_TRY((den_set_gemm_lds<DM, 0, 2>()));
    PD_TRY((den_set_gemm_lds<DFF, 0, 2>()));
    PD_TRY((den_set_gemm_lds<DM, 0, 0>()));
    PD_TRY(pd_set_lds(pd_attn_kernel<false>, attn_lds(64)));
    PD_TRY(pd_set_lds(pd_attn_kernel<true>, attn_lds(64)));
    PD_TRY(pd_set_lds(pd_attn_seq_kernel<0>, attn_seq_lds(64)));
    PD_TRY(pd_set_lds(pd_attn_seq_kernel<1>, attn_seq_lds(64)));
    PD_TRY(pd_set_lds(pd_attn_seq_kernel<2>, attn_seq_lds(64)));
    PD_TRY(pd_set_lds(pd_attn_mma_kernel<2>, attn_mma_lds(32)));
    PD_TRY(pd_set_lds(pd_attn_long_kernel<0>, pd_attn_long_lds(PD_MAX_DENOISER_FRAMES, DH)));
    PD_TRY(pd_set_lds(pd_attn_long_kernel<1>, pd_attn_long_lds(PD_MAX_DENOISER_FRAMES, DH)));
    PD_TRY(pd_set_lds(pd_attn_long_kernel<2>, pd_attn_long_lds(PD_MAX_DENOISER_FRAMES, DH)));
    PD_TRY(pd_set_lds(pd_qkv_attn_kernel<0>, 160 * 1024));
#ifdef PD_DEV_KNOBS
    PD_TRY(pd_set_lds(pd_qkv_attn_kernel<1>, 160 * 1024));
    PD_TRY(pd_set_lds(pd_qkv_attn_kernel<2>, 160 * 1024));
    PD_TRY(pd_set_lds(pd_qkv_attn_kernel<3>, 160 * 1024));
    PD_TRY(pd_set_lds(pd_qkv_attn_kernel<4>, 160 * 1024));
    PD_TRY(pd_set_lds(pd_qkv_attn_kernel<5>, 160 * 1024));
#endif
    return PD_OK;
}

int pd_denoiser_create(pd_engine *eng, const pd_weights *w) {
    if (!pd_denoiser_default_shape(w)) return pd_denoiser_generic_create(eng, w);
    PdDenoiserDev *d = new PdDenoiserDev();
    eng->den = d;
    d->num_layers = w->num_layers;
    d->timesteps = w->timesteps;
    d->m_cap = ((eng->max_B * eng->max_N + 31) / 32) * 32;
    PD_TRY(d->mem.alloc(&d->t_table, (size_t)w->timesteps * 128));
    PD_TRY(pd_time_table(w, d->t_table));
    PD_TRY(den_create_small_packs(d, w));
    PD_TRY(den_create_biases_rowmajor(d, w));
    PD_TRY(den_create_activations(d));
    if (d->hn) PD_TRY(den_create_first_pieces(d, w));
    PD_TRY(d->mem.rowmajor(&d->last0_wf, w->last0_w, HID, DM, nullptr));      // _last.0 for the streamed path
    PD_TRY(den_set_lds_attributes());
    PD_HIP_CHECK(hipDeviceSynchronize());
    return PD_OK;
}

bool pd_denoiser_has_streamed_path(const pd_engine *eng) { return eng->den && eng->den->hn; }   // (a generic engine has no den: none)
bool pd_denoiser_weights_non_finite(const pd_engine *eng) { return eng->den && eng->den->non_finite; }

// The split-precision modes' weights, built when the mode is first switched on from the row-major fp32 copies kept for the streamed
// GEMMs (LayerNorm scale folded): every encoder Linear split into bf16 hi / lo (mode 1, the fast mode) or into fp16 hi / lo of w * 2^e
// (mode 2) in MFMA fragment order.  Mode 2's power-of-two scales come from pd_plane_exponents; the LayerNorm operand takes 2^9.
int pd_denoiser_build_split(pd_engine *eng, int mode) {
    if (eng->gden) {
        pd_set_error("split-precision denoiser: this engine runs the shape-generic denoiser path (a non-default configuration or "
                     "PD_WEIGHTS_GENERIC), which has only the exact-fp32 kernels: PD_OPT_DENOISER_SPLIT stays 0");
        return PD_ERR_UNSUPPORTED;
    }
    PdDenoiserDev *d = eng->den;
    if (!d->hn) {
        pd_set_error("split-precision denoiser: the engine was created for fewer than %d token rows (max_B x max_N); the mode "
                     "applies to the streamed large-batch path only", PD_STREAM_MIN_ROWS);
        return PD_ERR_UNSUPPORTED;
    }
    const bool f16 = mode == 2;
    bool &ready = f16 ? d->split_h_ready : d->split_ready;
    if (ready) return PD_OK;
    PdPlaneExps e[PD_MAX_LAYERS] = {};
    for (int l = 0; f16 && l < d->num_layers; ++l) {
        PdLayerDev &L = d->layers[l];
        bool finite = true;
        PD_TRY(pd_plane_exponents(L.qkv_wf, L.qkv_b, L.out_wf, L.ff1_wf, L.ff1_b, L.ff2_wf, DM, DFF, &e[l], &finite));
        // a checkpoint with inf / NaN has no static bound: the fp16-plane mode is refused (PD_ERR_INVALID_ARG) and the engine stays on
        // the exact-fp32 kernels, which propagate the values like the reference does
        if (!finite) {
            d->non_finite = true;
            pd_set_error("denoiser: encoder layer %d holds non-finite weights or biases: no static operand bound exists, the fp16-plane "
                         "mode (PD_OPT_DENOISER_SPLIT = 2) is not available for these weights", l);
            return PD_ERR_INVALID_ARG;
        }
    }
    const int e_ln = 9;
    for (int l = 0; l < d->num_layers; ++l) {
        PdLayerDev &L = d->layers[l];
        PD_TRY(d->mem.planes(f16 ? &L.qkv_wh : &L.qkv_ws, L.qkv_wf, 3 * DM, DM, nullptr, f16, e[l].qkv));
        PD_TRY(d->mem.planes(f16 ? &L.out_wh : &L.out_ws, L.out_wf, DM, DM, nullptr, f16, e[l].out));
        PD_TRY(d->mem.planes(f16 ? &L.ff1_wh : &L.ff1_ws, L.ff1_wf, DFF, DM, nullptr, f16, e[l].ff1));
        PD_TRY(d->mem.planes(f16 ? &L.ff2_wh : &L.ff2_ws, L.ff2_wf, DM, DFF, nullptr, f16, e[l].ff2));
        if (!f16) continue;
        L.qkv_cs = ldexpf(1.0f, -(e_ln + e[l].qkv));
        L.out_cs = ldexpf(1.0f, -(e[l].ctx + e[l].out));
        L.ff1_cs = ldexpf(1.0f, -(e_ln + e[l].ff1));
        L.ff2_cs = ldexpf(1.0f, -(e[l].hid + e[l].ff2));
        L.ctx_scale = ldexpf(1.0f, e[l].ctx);
        L.ff_scale = ldexpf(1.0f, e[l].hid);
    }
    PD_HIP_CHECK(hipDeviceSynchronize());
    ready = true;
    return PD_OK;
}

void pd_denoiser_destroy(pd_engine *eng) {
    pd_denoiser_generic_destroy(eng);
    delete eng->den;
    eng->den = nullptr;
}

// The step-invariant piece of _first (models/denoiser.py:56-70: z and the pivot flag do not change over the T steps; here the z columns):
// zproj[m] = z[m] W_z^T + b_first, once per sampling call.  Every step then adds its row of the time table and its 192-column GEMM.
int pd_denoiser_prepare(pd_engine *eng, const float *z, int B, int N, hipStream_t s) {
    PdDenoiserDev *d = eng->den;
    if (eng->gden) d = nullptr;          // the generic path hoists nothing (pd_denoiser_generic.hip): only the arguments are checked
    if (!z || B <= 0 || N <= 0 || B > eng->max_B || N > eng->max_N) {
        pd_set_error("denoiser: invalid arguments (B=%d N=%d; max_B=%d max_N=%d)", B, N, eng->max_B, eng->max_N);
        return PD_ERR_INVALID_ARG;
    }
    if (!d) return PD_OK;
    const int M = B * N;
    // (below PD_STREAM_MIN_ROWS token rows _first stays ONE fused launch -- embedding staged in the GEMM's A rows, K = 704: a step there is a
    // chain of 43 latency-bound launches in which the shorter K buys 1 %, and the small-batch results stay bitwise those of rounds 1-4)
    if (M >= PD_STREAM_MIN_ROWS && d->hn) pd_gemm_dma<0>(z, ZD, d->first_zf, ZD, d->first_b, d->zproj, M, DM, s);
    PD_HIP_CHECK(hipGetLastError());
    return PD_OK;
}

// ---- one step's launches: _first, an encoder layer per path of the plan (pd_denoiser_plan.h), the tail -----------------------------------
// _first with the embedding fused into the A staging (one launch over all 702 columns)
static void den_first_small(const pd_engine *eng, const PdDenoiserDev *d, GemmArgs &g, const float *x, const float *z, int t, int N, int MT, hipStream_t s) {
    g.bias = d->first_b; g.C = d->h; g.Nout = DM;
    g.x = x; g.z = z; g.temb = d->t_table + (size_t)t * 128; g.n_frames = N;
    launch_gemm<KFIRST_PAD, 2, 0>(g, d->first_wp, MT, eng->gemm_wide_min_tiles, s);
}
// _first = zproj (z piece + bias, hoisted) + ttab[t] (time piece, a table) + the step piece, K = 192
static void den_first_streamed(const PdDenoiserDev *d, const float *x, int t, int N, int M, hipStream_t s) {
    hipLaunchKernelGGL(pd_embed_rows_kernel, dim3((M + 3) / 4), dim3(256), 0, s, x, N, M, d->emb);
    pd_gemm_dma<4>(d->emb, KFIRST_D, d->first_df, KFIRST_D, d->ttab + (size_t)t * DM, d->h, M, DM, s, nullptr, d->zproj);
}

// the same two with one timestep per token row: the A staging picks row t_row[m] of the time table; the bias becomes ttab[t_row[m]]
static void den_first_small_t(const pd_engine *eng, const PdDenoiserDev *d, GemmArgs &g, const float *x, const float *z, const int *t_row, int N, int MT,
                              hipStream_t s) {
    g.bias = d->first_b; g.C = d->h; g.Nout = DM;
    g.x = x; g.z = z; g.temb = d->t_table; g.t_row = t_row; g.n_frames = N;
    launch_gemm<KFIRST_PAD, 3, 0>(g, d->first_wp, MT, eng->gemm_wide_min_tiles, s);
}
static void den_first_streamed_t(const PdDenoiserDev *d, const float *x, const int *t_row, int N, int M, hipStream_t s) {
    hipLaunchKernelGGL(pd_embed_rows_kernel, dim3((M + 3) / 4), dim3(256), 0, s, x, N, M, d->emb);
    pd_den_first_gemm_t(d, t_row, M, s);
}

// the key-tiled attention kernel (pd_attn_long.h): more than 64 frames on every path, or PD_OPT_DENOISER_LONG_ATTN = 1
// nf: the frame counts per sequence (device, [B]) or null
template <int SPLIT_OUT>
static void den_attn_long(const PdDenoiserDev *d, int B, int N, float out_scale, const int *nf, hipStream_t s) {
    static_assert(PD_MAX_DENOISER_FRAMES == PD_ATTN_LONG_TILE * PD_ATTN_LONG_MAX_TILES, "a lane holds one score per 64-key tile");
    hipLaunchKernelGGL(pd_attn_long_kernel<SPLIT_OUT>, dim3(B * NH, (N + PD_ATTN_LONG_ROWS - 1) / PD_ATTN_LONG_ROWS), dim3(256), pd_attn_long_lds(N, DH), s,
                       d->qkv, d->ctx, N, out_scale, nf);
}

static void den_layer_small(const pd_engine *eng, const PdDenoiserDev *d, const PdLayerDev &L, GemmArgs &g, bool long_attn, const int *nf, int B, int N, int MT,
                            hipStream_t s) {
    // x += MHA(LN1(x))
    g.A = d->h; g.bias = L.qkv_b; g.C = d->qkv; g.Nout = 3 * DM;
    launch_gemm<DM, 1, 0>(g, L.qkv_wp, MT, eng->gemm_wide_min_tiles, s);
    if (long_attn) {
        den_attn_long<0>(d, B, N, 1.0f, nf, s);
    } else {
#ifdef PD_DEN_STAMPS
        hipLaunchKernelGGL(pd_attn_kernel<false>, dim3(B * NH, (N + 3) / 4), dim3(256), attn_lds(N), s, d->qkv, d->ctx, N, next_stamp_slot());
#else
        hipLaunchKernelGGL(pd_attn_kernel<false>, dim3(B * NH, (N + 3) / 4), dim3(256), attn_lds(N), s, d->qkv, d->ctx, N);
#endif
    }
    g.A = d->ctx; g.bias = L.out_b; g.C = d->h; g.Nout = DM;
    launch_gemm<DM, 0, 2>(g, L.out_wp, MT, eng->gemm_wide_min_tiles, s);
    // x += W2 relu(W1 LN2(x))
    g.A = d->h; g.bias = L.ff1_b; g.C = d->ff; g.Nout = DFF;
    launch_gemm<DM, 1, 1>(g, L.ff1_wp, MT, eng->gemm_wide_min_tiles, s);
    g.A = d->ff; g.bias = L.ff2_b; g.C = d->h; g.Nout = DM;
    launch_gemm<DFF, 0, 2>(g, L.ff2_wp, MT, eng->gemm_wide_min_tiles, s);
}
// exact fp32: LayerNorm is fused into the A staging of the streamed GEMMs (statistics pre-pass; affine folded into the weights, as on the small path)
static void den_layer_streamed(const PdDenoiserDev *d, const PdLayerDev &L, bool long_attn, const int *nf, int B, int N, int M, hipStream_t s) {
    float2 *stats = (float2 *)d->hn;           // (mean, rstd) per token row; applied in the A staging of the next GEMM
    hipLaunchKernelGGL(pd_ln_stats_kernel<DM>, dim3((M + 3) / 4), dim3(256), 0, s, d->h, stats, M, 1e-5f);
    pd_gemm_dma<0, true>(d->h, DM, L.qkv_wf, DM, L.qkv_b, d->qkv, M, 3 * DM, s, stats);                // LayerNorm-1 at the fragment reads
    if (long_attn) den_attn_long<0>(d, B, N, 1.0f, nf, s);
    else hipLaunchKernelGGL(pd_attn_seq_kernel<0>, dim3(B * NH), dim3(256), attn_seq_lds(N), s, d->qkv, d->ctx, N, 1.0f);
    pd_gemm_dma<2>(d->ctx, DM, L.out_wf, DM, L.out_b, d->h, M, DM, s);
    hipLaunchKernelGGL(pd_ln_stats_kernel<DM>, dim3((M + 3) / 4), dim3(256), 0, s, d->h, stats, M, 1e-5f);
    pd_gemm_dma<1, true>(d->h, DM, L.ff1_wf, DM, L.ff1_b, d->ff, M, DFF, s, stats);                     // LayerNorm-2 likewise
    pd_gemm_dma<2>(d->ff, DFF, L.ff2_wf, DFF, L.ff2_b, d->h, M, DM, s);
}
// fast mode: the four encoder GEMMs on the bf16 matrix pipe in split precision (pd_gemm_split.h); activations
// between them as split words -- LayerNorm, attention and the FF1 epilogue write them in place of fp32
static void den_layer_bf16(const PdDenoiserDev *d, const PdLayerDev &L, bool long_attn, const int *nf, int B, int N, int M, hipStream_t s) {
    hipLaunchKernelGGL((pd_ln_rows_kernel<DM, 1>), dim3((M + 3) / 4), dim3(256), 0, s, d->h, d->hn, M, 1e-5f, 1.0f);
    pd_gemm_split<0, 1, 2>((const unsigned *)d->hn, DM, L.qkv_ws, DM, L.qkv_b, d->qkv, M, 3 * DM, s);
    if (long_attn) den_attn_long<1>(d, B, N, 1.0f, nf, s);
    else hipLaunchKernelGGL(pd_attn_seq_kernel<1>, dim3(B * NH), dim3(256), attn_seq_lds(N), s, d->qkv, d->ctx, N, 1.0f);
    pd_gemm_split<2, 1, 1>((const unsigned *)d->ctx, DM, L.out_ws, DM, L.out_b, d->h, M, DM, s);
    hipLaunchKernelGGL((pd_ln_rows_kernel<DM, 1>), dim3((M + 3) / 4), dim3(256), 0, s, d->h, d->hn, M, 1e-5f, 1.0f);
    pd_gemm_split<4, 1, 2>((const unsigned *)d->hn, DM, L.ff1_ws, DM, L.ff1_b, d->ff, M, DFF, s);
    pd_gemm_split<2, 1, 1>((const unsigned *)d->ff, DFF, L.ff2_ws, DFF, L.ff2_b, d->h, M, DM, s);
}
// One GEMM of the fp16-plane path, C = epi(A [M, K] W^T): the strip kernel (A by LDS-DMA, no weight fragment fetched twice) at rt 32-row tiles per
// workgroup, or (rt = 0) the round-1 two-plane kernel: the same results but for a sum's last bit (header of pd_gemm_split.h).  Only the row tiles an epilogue is
// launched with exist as kernels: 2 for all, 3 for the residual (2) and FF1 (4) epilogues.
template <int EPI>
static void den_gemm_f16(int rt, const float *A, int K, const unsigned *W, const float *bias, float *C, int M, int Nout, hipStream_t s, float c_scale,
                         float out_scale = 1.0f) {
    const unsigned *Aw = (const unsigned *)A;        // split words
    if constexpr (EPI != 0)
        if (rt == 3) return pd_gemm_strip<EPI, 3>(Aw, K, W, K, bias, C, M, Nout, s, c_scale, out_scale);
    if (rt == 2) return pd_gemm_strip<EPI, 2>(Aw, K, W, K, bias, C, M, Nout, s, c_scale, out_scale);
    pd_gemm_split<EPI, 1, EPI == 2 ? 1 : 2, true>(Aw, K, W, K, bias, C, M, Nout, s, c_scale, out_scale);
}
// fp16-plane mode: the fast mode's kernels with fp16 halves and the static power-of-two scales of pd_denoiser_build_split
// (22 mantissa bits, fp32 accumulation: fp32-grade results at the three-product rate)
static void den_layer_f16(const PdDenoiserDev *d, const PdLayerDev &L, const PdDenStepPlan &p, const int *nf, int B, int N, hipStream_t s) {
    const int M = p.M;
    hipLaunchKernelGGL((pd_ln_rows_kernel<DM, 2>), dim3((M + 3) / 4), dim3(256), 0, s, d->h, d->hn, M, 1e-5f, 512.0f);
    if (p.fused_attn) {
        // in_proj + attention of a head for a group of whole sequences in one workgroup, Q / K / V in LDS only (pd_qkv_attn.h):
        // bitwise the two launches of the else branch
        pd_qkv_attn((const unsigned *)d->hn, L.qkv_wh, L.qkv_b, (unsigned *)d->ctx, B, N, L.qkv_cs, L.ctx_scale, s);
    } else {
        den_gemm_f16<0>(p.strip & 1 ? 2 : 0, d->hn, DM, L.qkv_wh, L.qkv_b, d->qkv, M, 3 * DM, s, L.qkv_cs);
        if (p.long_attn) den_attn_long<2>(d, B, N, L.ctx_scale, nf, s);
        else if (p.attn_mma) hipLaunchKernelGGL(pd_attn_mma_kernel<2>, dim3(B * NH), dim3(256), attn_mma_lds(N), s, d->qkv, d->ctx, N, L.ctx_scale);
        else hipLaunchKernelGGL(pd_attn_seq_kernel<2>, dim3(B * NH), dim3(256), attn_seq_lds(N), s, d->qkv, d->ctx, N, L.ctx_scale);
    }
    den_gemm_f16<2>(p.strip & 2 ? p.rt_res : 0, d->ctx, DM, L.out_wh, L.out_b, d->h, M, DM, s, L.out_cs);
    hipLaunchKernelGGL((pd_ln_rows_kernel<DM, 2>), dim3((M + 3) / 4), dim3(256), 0, s, d->h, d->hn, M, 1e-5f, 512.0f);
    den_gemm_f16<4>(p.strip & 4 ? p.rt_ff1 : 0, d->hn, DM, L.ff1_wh, L.ff1_b, d->ff, M, DFF, s, L.ff1_cs, L.ff_scale);
    den_gemm_f16<2>(p.strip & 8 ? p.rt_res : 0, d->ff, DFF, L.ff2_wh, L.ff2_b, d->h, M, DM, s, L.ff2_cs);
}
// the fused LN / ReLU / Linear(128 -> 9) / DDPM tail on _last.0's output
static void den_tail(const pd_engine *eng, const PdDenoiserDev *d, const float *x, int t, int M, float *eps_out, float *mean_out, float *x0_out,
                     const float *noise, float *x_next_out, bool stamped, const int *nf, int N, hipStream_t s) {
    HeadArgs ha;
    memset(&ha, 0, sizeof(ha));
    ha.hid = d->hid; ha.lnw = d->last_ln_w; ha.lnb = d->last_ln_b;
    ha.w3 = d->last3_w; ha.b3 = d->last3_b; ha.x = x; ha.noise = noise;
    ha.eps_out = eps_out; ha.mean_out = mean_out; ha.x0_out = x0_out; ha.xnext_out = x_next_out;
    ha.c_recip = eng->c_recip[t]; ha.c_recipm1 = eng->c_recipm1[t]; ha.coef1 = eng->coef1[t]; ha.coef2 = eng->coef2[t];
    ha.sigma = expf(0.5f * eng->logvar[t]);
    ha.M = M;
    ha.pred_x0 = eng->pred_x0;
    ha.nf = nf; ha.n_frames = N;
#ifdef PD_DEN_STAMPS
    ha.stamps = stamped ? next_stamp_slot() : nullptr;
#endif
    hipLaunchKernelGGL(pd_tail_kernel, dim3((M + 3) / 4), dim3(256), 0, s, ha);
}

// the tail with every row's own schedule coefficients and the outputs of p_losses
static void den_tail_t(const pd_engine *eng, const PdDenoiserDev *d, const float *x, int M, const PdTSeq &ts, float *eps_out, float *x0_out, hipStream_t s) {
    HeadArgsT a;
    memset(&a, 0, sizeof(a));
    a.h.hid = d->hid; a.h.lnw = d->last_ln_w; a.h.lnb = d->last_ln_b;
    a.h.w3 = d->last3_w; a.h.b3 = d->last3_b; a.h.x = x;
    a.h.eps_out = eps_out; a.h.x0_out = x0_out;
    a.h.M = M;
    a.h.pred_x0 = eng->pred_x0;
    a.t_row = ts.t_row; a.c_recip = eng->d_c_recip; a.c_recipm1 = eng->d_c_recipm1;
    a.target = ts.target; a.loss_out = ts.loss_out; a.loss_type = ts.loss_type;
    hipLaunchKernelGGL(pd_tail_t_kernel, dim3((M + 3) / 4), dim3(256), 0, s, a);
}

// t_seq [B] -> eng->d_t_row [B x N], clamped and checked on the device (bit 3 of the asynchronous error word); B, N checked by the caller
int pd_denoiser_t_rows(pd_engine *eng, const int64_t *t_seq, int B, int N, hipStream_t s) {
    const int M = B * N;
    hipLaunchKernelGGL(pd_t_rows_kernel, dim3((M + 255) / 256), dim3(256), 0, s, t_seq, M, N, eng->timesteps, eng->d_t_row, eng->d_err);
    PD_HIP_CHECK(hipGetLastError());
    return PD_OK;
}
int pd_denoiser_q_sample(pd_engine *eng, const float *x_start, const float *noise, const int64_t *t_seq, int B, int N, float *xt, hipStream_t s) {
    const int M = B * N;
    hipLaunchKernelGGL(pd_q_sample_kernel, dim3((M * 9 + 255) / 256), dim3(256), 0, s, x_start, noise, t_seq, eng->d_q_a, eng->d_q_b, M, N, eng->timesteps,
                       xt, eng->d_t_row, eng->d_err);
    PD_HIP_CHECK(hipGetLastError());
    return PD_OK;
}

// z_prepared: pd_denoiser_prepare ran for this z (the sampling loop calls it once); otherwise it is issued here (the step-level API)
int pd_denoiser_launch(pd_engine *eng, const float *x, const float *z, int t, int B, int N, float *eps_out,
                       float *mean_out, float *x0_out, const float *noise, float *x_next_out, hipStream_t s, bool z_prepared, const PdTSeq *ts) {
    if (eng->gden) return pd_denoiser_generic_launch(eng, x, z, t, B, N, eps_out, mean_out, x0_out, noise, x_next_out, s, ts);
    PdDenoiserDev *d = eng->den;
    if (!x || !z || B <= 0 || N <= 0 || B > eng->max_B || N > eng->max_N || N > PD_MAX_DENOISER_FRAMES || t < 0 || t >= d->timesteps) {
        pd_set_error("denoiser: invalid arguments (B=%d N=%d t=%d; max_B=%d max_N=%d, N <= %d, 0 <= t < %d)", B, N, t,
                     eng->max_B, eng->max_N, PD_MAX_DENOISER_FRAMES, d->timesteps);
        return PD_ERR_INVALID_ARG;
    }
    // frame counts per sequence (pd_engine_set_frame_counts): attention takes the length of every sequence, the tail zeroes the padding rows;
    // everything between is per-row work.  The training branch (ts) is refused by its entry points while counts are set.
    const int *nf = nullptr;
    if (!ts) PD_TRY(pd_frame_counts(eng, B, N, "denoiser", &nf));
    if (!z_prepared) {
        int rc = pd_denoiser_prepare(eng, z, B, N, s);
        if (rc) return rc;
    }
    static const int knob_strip = pd_dev_knob("PD_DEN_STRIP", 15), knob_attn_mma = pd_dev_knob("PD_DEN_ATTN_MMA", 1);     // development A / B
    const PdDenStepPlan p = pd_den_step_plan(B, N, eng->den_split, eng->den_fused_attn, eng->num_cus, d->hn != nullptr, d->split_ready,
                                             d->split_h_ready, knob_strip, knob_attn_mma, eng->den_long_attn, nf != nullptr);
    const bool small = p.path == PD_DEN_SMALL;
    const int M = p.M;
    GemmArgs g;                       // the small path's launches share it
    memset(&g, 0, sizeof(g));
    g.M = M;
    if (small && ts) den_first_small_t(eng, d, g, x, z, ts->t_row, N, p.MT, s);
    else if (small) den_first_small(eng, d, g, x, z, t, N, p.MT, s);
    else if (ts) den_first_streamed_t(d, x, ts->t_row, N, M, s);
    else den_first_streamed(d, x, t, N, M, s);
    for (int l = 0; l < d->num_layers; ++l) {
        const PdLayerDev &L = d->layers[l];
        switch (p.path) {
        case PD_DEN_SMALL: den_layer_small(eng, d, L, g, p.long_attn, nf, B, N, p.MT, s); break;
        case PD_DEN_STREAMED: den_layer_streamed(d, L, p.long_attn, nf, B, N, M, s); break;
        case PD_DEN_BF16_PLANES: den_layer_bf16(d, L, p.long_attn, nf, B, N, M, s); break;
        case PD_DEN_F16_PLANES: den_layer_f16(d, L, p, nf, B, N, s); break;
        }
    }
    // _last.0 as a plain tile GEMM, then the tail
    if (small) {
        g.A = d->h; g.bias = d->last0_b; g.C = d->hid; g.Nout = HID;
        launch_gemm<DM, 0, 0>(g, d->last0_wp, p.MT, eng->gemm_wide_min_tiles, s);
    } else {
        pd_gemm_dma<0>(d->h, DM, d->last0_wf, DM, d->last0_b, d->hid, M, HID, s);
    }
    if (ts) den_tail_t(eng, d, x, M, *ts, eps_out, x0_out, s);
    else den_tail(eng, d, x, t, M, eps_out, mean_out, x0_out, noise, x_next_out, small, nf, N, s);
    PD_HIP_CHECK(hipGetLastError());
    return PD_OK;
}


// ---- rows D2 / D3 as stand-alone operators (the reference's util/embedding.py modules called piecewise) -------------------------------
extern "C" int pd_time_embedding(const float *w0, const float *b0, const float *w2, const float *b2, const float *timesteps, int n,
                                 float *out, void *stream) {
    if (n == 0) return PD_OK;                       // an empty batch: nothing to read or write (the pointers may be NULL)
    if (!w0 || !b0 || !w2 || !b2 || !timesteps || !out || n < 0) {
        pd_set_error("pd_time_embedding: invalid arguments (n=%d)", n);
        return PD_ERR_INVALID_ARG;
    }
    hipLaunchKernelGGL(pd_time_embed_kernel, dim3(n), dim3(128), 0, (hipStream_t)stream, timesteps, w0, b0, w2, b2, out);
    PD_HIP_CHECK(hipGetLastError());
    return PD_OK;
}
extern "C" int pd_pose_embedding(const float *x, long long rows, int dim, float *out, void *stream) {
    if (rows == 0 && dim >= 1) return PD_OK;        // an empty batch (the pointers may be NULL)
    if (!x || !out || rows < 0 || dim < 1 || dim > 4096) {
        pd_set_error("pd_pose_embedding: invalid arguments (rows=%lld dim=%d)", rows, dim);
        return PD_ERR_INVALID_ARG;
    }
    const long long total = rows * 21 * dim;
    const int blocks = (int)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
    hipLaunchKernelGGL(pd_harmonic_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, rows, dim, out);
    PD_HIP_CHECK(hipGetLastError());
    return PD_OK;
}

// ---- probe: fp16-subnormal operands on the fp16 matrix pipe (pd_engine.h pd_debug_mfma_f16_subnormal; the kernel: pd_denoiser_kernels.h) ----
static int mfma_f16_subnormal(bool shape16, const char *who, float *out4_host, void *stream) {
    if (!out4_host) return PD_ERR_INVALID_ARG;
    float *d = nullptr;
    PD_HIP_CHECK(hipMalloc((void **)&d, 8 * sizeof(float)));
    hipStream_t s = (hipStream_t)stream;
    if (shape16) hipLaunchKernelGGL(pd_mfma16_f16_subnormal_kernel, dim3(1), dim3(64), 0, s, d);
    else hipLaunchKernelGGL(pd_mfma_f16_subnormal_kernel, dim3(1), dim3(64), 0, s, d);
    float h[8];
    hipError_t e = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(d);
    if (e != hipSuccess) {
        pd_set_error("%s: %s", who, hipGetErrorString(e));
        return PD_ERR_HIP;
    }
    for (int i = 0; i < 4; ++i) out4_host[i] = h[i];
    if (h[4] == 0.0f) out4_host[0] = -1.0f;   // the fp32 -> fp16 conversion itself flushed 2^-20 (would make the probe meaningless)
    return PD_OK;
}
// out4_host[0] == 32 on entry: the products on v_mfma_f32_16x16x32_f16 (the large-batch planes' shape, 32 k per instruction) instead of 32x32x16
extern "C" int pd_debug_mfma_f16_subnormal(float *out4_host, void *stream) {
    return mfma_f16_subnormal(out4_host && out4_host[0] == 32.0f, "pd_debug_mfma_f16_subnormal", out4_host, stream);
}
