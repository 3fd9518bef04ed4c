// pd_vit_train.hip -- the image backbone with gradients (include/pd_engine_vit_train.h): the multi-scale DINO ViT-S/16
// forward with an activation stash, and its backward from dS/dz to every backbone parameter.  Kernels: pd_vit_train_kernels.h (the ViT's own,
// the only device code of this file) and the denoiser trainer's -- every matrix product, LayerNorm forward and backward, column sums, split
// reductions, key-tiled attention -- through the launch helpers of pd_train_launch.h, which pd_train.hip defines next to the kernels.
//
// Replaces (paths relative to the reference's pose_diffusion/): the autograd graph of models/image_feature_extractor.py:57-87 over the
// torch.hub dino_vits16 backbone (:40-42) that train.py back-propagates when IMAGE_FEATURE_EXTRACTOR.freeze is False (all three configs).
//
// Forward, per scale in call order, on the caller's live weights:
//   im2col of the prepared images -> patch GEMM -> token assembly (+ cls, + pos) -> per block { LN1 (+stats) -> qkv GEMM -> attention ->
//   proj GEMM + residual -> LN2 (+stats) -> fc1 GEMM (pre-activation stashed) -> GELU -> fc2 GEMM + residual } -> final LayerNorm of the CLS
//   rows, added into z; the last scale divides by n_scales.
// The residual stream is never updated in place: hres[i] is the stream at sublayer input i (2 L + 1 arrays per scale), which IS the stash.
// Backward, per scale in REVERSE call order: final LayerNorm -> per block in reverse { GELU recomputed, fc2, GELU', fc1, LN2, proj,
//   attention (two launches), qkv, LN1 } -> token assembly adjoint -> patch GEMM's weight gradient.  The first scale it runs writes every
//   gradient, the later ones add to it (the helpers' acc: the GEMM's resid = C path, the accumulating reduce).  Then cls_token / pos_embed from the
//   scales' per-token position gradients in call order (pd_vt_posgrid_kernel).
#include "pd_vit_train_kernels.h"
#include "../../include/pd_engine_vit_train.h"

#include <algorithm>
#include <string.h>

#define VT_EPS 1e-6f                // DINO's partial(nn.LayerNorm, eps=1e-6)

struct PdVtLayerStash {
    float *stats1, *stats2;         // [rows, 2] (mean, rstd)
    float *qkv, *ctx, *pre;         // [rows, 3 d], [rows, d], [rows, ff] (fc1 output before the GELU)
};

struct PdVtScale {                  // one scale of the pending forward
    int gh, gw, P, T, M;            // token grid, patches and tokens per image, token rows of the scale
    size_t row0;                    // its first row in every stash array
    int resampled;                  // its position table came from the caller (bicubic resampling of the trained grid)
};

struct pd_vit_trainer {
    int d = 0, nhead = 0, hd = 0, ff = 0, layers = 0, grid0 = 0;
    int max_images = 0, max_rows = 0, max_scales = 0;
    // stash
    float *cols = nullptr;                               // [rows, 768] im2col rows (a scale's n P rows at its row0)
    float *hres[2 * 16 + 1] = {};                        // [rows, d] each
    PdVtLayerStash L[16] = {};
    float *fstats = nullptr;                             // [max_scales][max_images][2] final LayerNorm statistics
    // scratch
    float *hn = nullptr, *dres = nullptr, *dhn = nullptr, *act = nullptr, *dff = nullptr, *dqkv = nullptr;
    float *dpos = nullptr;                               // [max_scales][PD_VT_MAX_TOKENS][d] per-token position gradients
    PdTrWork wk = {};                                    // split-reduction workspaces and la_stats [rows nhead, 4], as in pd_trainer
    float *ws_d = nullptr;                               // [VT_DGRAD_MAX_CHUNKS][rows, d] partial data gradients of a long reduction
    int pend_n = 0, pend_scales = 0;                     // images / scales of the pending forward (0: none)
    PdVtScale pend[PD_VIT_TRAIN_MAX_SCALES] = {};
    PdDevAllocs mem{"pd_vit_trainer_create"};
};

// ---- launch helpers: pd_train_launch.h's, and the data gradient's own --------------------------------------------------------------
// dX[M, K] = dY[M, Nout] W (W [Nout, K]).  A reduction of more than VT_DGRAD_SPLIT terms (every layer: 384, qkv's 1152, fc1's 1536) is cut
// into chunks of VT_DGRAD_CHUNK whose partial sums are added in chunk order: one fmaf chain over 1536 terms left norm2 / proj gradients
// 3.4 x further from float64 than torch's blocked sums are, and chains of 384 still left a cancelling column sum behind qkv's data
// gradient twice as far as chains of 96 do (profiles/vit_train_parity.txt sections 1 and 5).  The cut depends on the layer's width alone.
#define VT_DGRAD_SPLIT 128
#define VT_DGRAD_CHUNK 96
#define VT_DGRAD_MAX_CHUNKS 16
static void vt_dgrad(pd_vit_trainer *tr, const float *dY, const float *W, float *dX, int M, int Nout, int K, hipStream_t s) {
    const int nch = Nout > VT_DGRAD_SPLIT ? (Nout + VT_DGRAD_CHUNK - 1) / VT_DGRAD_CHUNK : 1;
    PdTrGemm g;
    memset(&g, 0, sizeof(g));
    g.A = dY; g.a_rs = Nout; g.a_cs = 1; g.a_rfast = 1;
    g.B = W; g.b_rs = K; g.b_cs = 1; g.b_rfast = 0;
    g.C = nch > 1 ? tr->ws_d : dX; g.ldc = K;
    g.I = M; g.J = K; g.R = Nout; g.r_chunk = nch > 1 ? VT_DGRAD_CHUNK : Nout;
    pd_tr_gemm_launch(g, nch, s);
    if (nch > 1) pd_tr_reduce_launch(tr->ws_d, (long long)M * K, nch, dX, s);
}

static unsigned vt_blocks(size_t total, unsigned cap) { return (unsigned)std::min<size_t>((total + 255) / 256, cap); }

// ---- shape checks ----------------------------------------------------------------------------
static int vt_shape_check(const pd_vit_weights *w, const char *who) {
    const char *msg = nullptr;
    if (w->dim != 384) msg = "dim must be 384";
    else if (w->num_heads != 6) msg = "num_heads must be 6 (head dim 64)";
    else if (w->mlp_hidden != 1536) msg = "mlp_hidden must be 1536";
    else if (w->patch_size != PD_VT_PATCH) msg = "patch_size must be 16";
    else if (w->depth < 1 || w->depth > 16) msg = "depth must be in [1, 16]";
    else if (w->pos_grid < 1 || w->pos_grid > 15) msg = "pos_grid must be in [1, 15]";
    if (msg) {
        pd_set_error("%s: unsupported ViT shape: %s (dim=%d heads=%d mlp=%d patch=%d depth=%d pos_grid=%d)", who, msg, w->dim, w->num_heads, w->mlp_hidden,
                     w->patch_size, w->depth, w->pos_grid);
        return PD_ERR_UNSUPPORTED;
    }
    return PD_OK;
}

extern "C" int pd_vit_trainer_create(const pd_vit_weights *shape, int max_images, int max_rows, int max_scales, pd_vit_trainer **out) {
    if (!shape || !out) {
        pd_set_error("pd_vit_trainer_create: invalid argument: NULL shape or out");
        return PD_ERR_INVALID_ARG;
    }
    *out = nullptr;
    if (max_images < 1 || max_rows < 2 || max_scales < 1 || max_scales > PD_VIT_TRAIN_MAX_SCALES) {
        pd_set_error("pd_vit_trainer_create: invalid argument: max_images=%d (>= 1), max_rows=%d (>= 2), max_scales=%d (1 .. %d)", max_images, max_rows,
                     max_scales, PD_VIT_TRAIN_MAX_SCALES);
        return PD_ERR_INVALID_ARG;
    }
    PD_TRY(vt_shape_check(shape, "pd_vit_trainer_create"));
    pd_vit_trainer *tr = new pd_vit_trainer();
    tr->d = shape->dim; tr->nhead = shape->num_heads; tr->hd = tr->d / tr->nhead; tr->ff = shape->mlp_hidden; tr->layers = shape->depth;
    tr->grid0 = shape->pos_grid;
    tr->max_images = max_images; tr->max_rows = max_rows; tr->max_scales = max_scales;
    const size_t rows = (size_t)max_rows, d = tr->d, ff = tr->ff;
    int rc = PD_OK;
#define VT_A(p, n) if (rc == PD_OK) rc = tr->mem.alloc(&(p), (size_t)(n), true)
    VT_A(tr->cols, rows * PD_VT_KP);
    for (int i = 0; i <= 2 * tr->layers; ++i) VT_A(tr->hres[i], rows * d);
    for (int l = 0; l < tr->layers; ++l) {
        VT_A(tr->L[l].stats1, rows * 2); VT_A(tr->L[l].stats2, rows * 2);
        VT_A(tr->L[l].qkv, rows * 3 * d); VT_A(tr->L[l].ctx, rows * d); VT_A(tr->L[l].pre, rows * ff);
    }
    VT_A(tr->fstats, (size_t)max_scales * max_images * 2);
    VT_A(tr->hn, rows * d); VT_A(tr->dres, rows * d); VT_A(tr->dhn, rows * d); VT_A(tr->act, rows * ff); VT_A(tr->dff, rows * ff); VT_A(tr->dqkv, rows * 3 * d);
    VT_A(tr->wk.la_stats, rows * tr->nhead * PD_TR_LA_STATS);
    VT_A(tr->dpos, (size_t)max_scales * PD_VT_MAX_TOKENS * d);
    VT_A(tr->wk.ws, std::max(ff * d, d * (size_t)PD_VT_KP) * PD_TR_MAX_CHUNKS);
    VT_A(tr->wk.ws_col, 2 * std::max(ff, 3 * d) * PD_TR_MAX_CHUNKS);
    VT_A(tr->ws_d, (size_t)VT_DGRAD_MAX_CHUNKS * rows * d);
#undef VT_A
    if (rc == PD_OK) rc = pd_tr_set_attention_lds();
    if (rc == PD_OK && hipDeviceSynchronize() != hipSuccess) rc = PD_ERR_HIP;
    if (rc != PD_OK) {
        if (rc == PD_ERR_HIP) pd_set_error("pd_vit_trainer_create: a HIP call failed: %s", hipGetErrorString(hipGetLastError()));
        delete tr;
        return rc;
    }
    *out = tr;
    return PD_OK;
}

extern "C" void pd_vit_trainer_destroy(pd_vit_trainer *tr) { delete tr; }

static int vt_weights_match(const pd_vit_trainer *tr, const pd_vit_weights *w, const char *who) {
    if (!w) {
        pd_set_error("%s: invalid argument: NULL weights", who);
        return PD_ERR_INVALID_ARG;
    }
    if (w->dim != tr->d || w->num_heads != tr->nhead || w->mlp_hidden != tr->ff || w->depth != tr->layers || w->patch_size != PD_VT_PATCH ||
        w->pos_grid != tr->grid0) {
        pd_set_error("%s: invalid argument w: its shape fields differ from the shape this trainer was created for", who);
        return PD_ERR_INVALID_ARG;
    }
    bool ok = w->patch_w && w->patch_b && w->cls_token && w->pos_embed && w->norm_w && w->norm_b;
    for (int l = 0; l < tr->layers && ok; ++l) {
        const pd_vit_layer_weights &L = w->layers[l];
        ok = L.norm1_w && L.norm1_b && L.qkv_w && L.qkv_b && L.proj_w && L.proj_b && L.norm2_w && L.norm2_b && L.fc1_w && L.fc1_b && L.fc2_w && L.fc2_b;
    }
    if (!ok) {
        pd_set_error("%s: invalid argument w: a weight pointer is NULL", who);
        return PD_ERR_INVALID_ARG;
    }
    return PD_OK;
}

extern "C" int pd_vit_train_forward(pd_vit_trainer *tr, const pd_vit_weights *w, const float *images, int n, int H, int W,
                                    const double *scale_factors, int n_scales, const float *const *pos, float *z_out, void *stream) {
    const char *who = "pd_vit_train_forward";
    if (!tr) {
        pd_set_error("%s: invalid argument: NULL trainer", who);
        return PD_ERR_INVALID_ARG;
    }
    if (!images || !z_out || !scale_factors) {
        pd_set_error("%s: invalid argument: images, scale_factors and z_out must not be NULL", who);
        return PD_ERR_INVALID_ARG;
    }
    if (n < 1 || H < 1 || W < 1 || n_scales < 1) {
        pd_set_error("%s: invalid argument: n=%d, H=%d, W=%d and n_scales=%d must be positive", who, n, H, W, n_scales);
        return PD_ERR_INVALID_ARG;
    }
    PD_TRY(vt_weights_match(tr, w, who));
    if (n_scales > tr->max_scales) {
        pd_set_error("%s: n_scales=%d exceeds the limit of %d scales this trainer was created for", who, n_scales, tr->max_scales);
        return PD_ERR_UNSUPPORTED;
    }
    if (n > tr->max_images) {
        pd_set_error("%s: n=%d exceeds the capacity of %d images this trainer was created for", who, n, tr->max_images);
        return PD_ERR_UNSUPPORTED;
    }
    PdVtScale sc[PD_VIT_TRAIN_MAX_SCALES];
    float inv_sf[PD_VIT_TRAIN_MAX_SCALES];
    int same_size[PD_VIT_TRAIN_MAX_SCALES];
    size_t rows = 0;
    for (int i = 0; i < n_scales; ++i) {
        const double sf = scale_factors[i];
        if (!(sf > 0.0)) {
            pd_set_error("%s: invalid argument scale_factors[%d]=%g: a scale factor must be positive", who, i, sf);
            return PD_ERR_INVALID_ARG;
        }
        const bool identity = sf == 1.0;
        const int hs = identity ? H : (int)floor((double)H * sf), wsz = identity ? W : (int)floor((double)W * sf);   // torch: floor(size * scale) in double
        PdVtScale &S = sc[i];
        S.gh = hs / PD_VT_PATCH; S.gw = wsz / PD_VT_PATCH; S.P = S.gh * S.gw; S.T = S.P + 1;
        if (S.gh < 1 || S.gw < 1) {
            pd_set_error("%s: scale %d (%g) leaves %d x %d pixels: below the limit of one whole 16 x 16 patch", who, i, sf, hs, wsz);
            return PD_ERR_UNSUPPORTED;
        }
        if ((long long)S.gh * S.gw + 1 > PD_VT_MAX_TOKENS) {
            pd_set_error("%s: scale %d (%g) gives %lld tokens per image (%d x %d pixels): the limit is %d tokens per image", who, i, sf,
                         (long long)S.gh * S.gw + 1, hs, wsz, PD_VT_MAX_TOKENS);
            return PD_ERR_UNSUPPORTED;
        }
        // DINO's interpolate_pos_encoding returns pos_embed only for the trained grid AND hs == wsz.  Unequal pixel sizes on the trained grid
        // (224 x 232) are resampled with scale factor (g + 0.1) / g per axis, which is no copy: source coordinates move by up to 0.1 cell
        const bool trained = S.gh == tr->grid0 && S.gw == tr->grid0 && hs == wsz;
        S.resampled = (pos && pos[i] && !trained) ? 1 : 0;
        if (!S.resampled && !trained) {
            pd_set_error("%s: invalid argument pos[%d]: NULL, but the scale's %d x %d token grid is not the trained %d x %d one and needs the "
                         "resampled position table", who, i, S.gh, S.gw, tr->grid0, tr->grid0);
            return PD_ERR_INVALID_ARG;
        }
        S.M = n * S.T;
        S.row0 = rows;
        rows += (size_t)S.M;
        inv_sf[i] = (float)(1.0 / sf);          // torch: float(1 / scale_factor) as the coordinate scale
        same_size[i] = identity ? 1 : 0;
    }
    if (rows > (size_t)tr->max_rows) {
        pd_set_error("%s: %d images give %zu token rows over the %d scales: beyond the capacity of %d token rows this trainer was created for", who, n,
                     rows, n_scales, tr->max_rows);
        return PD_ERR_UNSUPPORTED;
    }
    hipStream_t s = (hipStream_t)stream;
    tr->pend_n = tr->pend_scales = 0;
    const int d = tr->d, ff = tr->ff, Lc = tr->layers;
    const float scale = 1.0f / sqrtf((float)tr->hd);
    for (int i = 0; i < n_scales; ++i) {
        const PdVtScale &S = sc[i];
        const int M = S.M;
        const size_t r0 = S.row0;
        float *cols = tr->cols + r0 * PD_VT_KP;
        hipLaunchKernelGGL(pd_vt_im2col_kernel, dim3(vt_blocks((size_t)n * S.P * PD_VT_KP, 8192)), dim3(256), 0, s, images, n, H, W, S.gh, S.gw, inv_sf[i], same_size[i],
                           cols);
        pd_tr_linear(cols, w->patch_w, w->patch_b, tr->hn, n * S.P, d, PD_VT_KP, 0, nullptr, s);
        hipLaunchKernelGGL(pd_vt_assemble_kernel, dim3(vt_blocks((size_t)M * d, 4096)), dim3(256), 0, s, tr->hn, w->cls_token,
                           S.resampled ? pos[i] : w->pos_embed, n, S.T, d, tr->hres[0] + r0 * d);
        for (int l = 0; l < Lc; ++l) {
            const pd_vit_layer_weights &Wl = w->layers[l];
            const PdVtLayerStash &St = tr->L[l];
            float *h0 = tr->hres[2 * l] + r0 * d, *h1 = tr->hres[2 * l + 1] + r0 * d, *h2 = tr->hres[2 * l + 2] + r0 * d;
            float *qkv = St.qkv + r0 * 3 * d, *ctx = St.ctx + r0 * d, *pre = St.pre + r0 * ff;
            pd_tr_ln_launch(h0, tr->hn, Wl.norm1_w, Wl.norm1_b, M, d, VT_EPS, St.stats1 + r0 * 2, s);
            pd_tr_linear(tr->hn, Wl.qkv_w, Wl.qkv_b, qkv, M, 3 * d, d, 0, nullptr, s);
            pd_tr_attn_launch(true, qkv, ctx, n, S.T, tr->nhead, tr->hd, d, scale, nullptr, s);
            pd_tr_linear(ctx, Wl.proj_w, Wl.proj_b, h1, M, d, d, 0, h0, s);
            pd_tr_ln_launch(h1, tr->hn, Wl.norm2_w, Wl.norm2_b, M, d, VT_EPS, St.stats2 + r0 * 2, s);
            pd_tr_linear(tr->hn, Wl.fc1_w, Wl.fc1_b, pre, M, ff, d, 0, nullptr, s);
            hipLaunchKernelGGL(pd_vt_gelu_kernel, dim3(vt_blocks((size_t)M * ff / 4, 4096)), dim3(256), 0, s, (const float4 *)pre, (float4 *)tr->act,
                               (size_t)M * ff / 4);
            pd_tr_linear(tr->act, Wl.fc2_w, Wl.fc2_b, h2, M, d, ff, 0, h1, s);
        }
        hipLaunchKernelGGL(pd_vt_final_kernel, dim3((n + 3) / 4), dim3(256), 0, s, tr->hres[2 * Lc] + r0 * d, n, S.T, d, w->norm_w, w->norm_b, VT_EPS,
                           i == 0 ? 1 : 0, i == n_scales - 1 ? 1 : 0, n_scales, z_out, tr->fstats + (size_t)i * tr->max_images * 2);
    }
    PD_HIP_CHECK(hipGetLastError());
    memcpy(tr->pend, sc, sizeof(sc[0]) * n_scales);
    tr->pend_n = n;
    tr->pend_scales = n_scales;
    return PD_OK;
}

extern "C" int pd_vit_train_backward(pd_vit_trainer *tr, const pd_vit_weights *w, const float *g_z, const pd_vit_weight_grads *grads, void *stream) {
    const char *who = "pd_vit_train_backward";
    if (!tr || !g_z || !grads) {
        pd_set_error("%s: invalid argument: NULL trainer, g_z or grads", who);
        return PD_ERR_INVALID_ARG;
    }
    if (tr->pend_n < 1 || tr->pend_scales < 1) {
        pd_set_error("%s: no forward is pending (pd_vit_train_forward fills the stash that one backward consumes)", who);
        return PD_ERR_STATE;
    }
    PD_TRY(vt_weights_match(tr, w, who));
    hipStream_t s = (hipStream_t)stream;
    const int n = tr->pend_n, ns = tr->pend_scales, d = tr->d, ff = tr->ff, Lc = tr->layers;
    tr->pend_n = tr->pend_scales = 0;
    const float scale = 1.0f / sqrtf((float)tr->hd);
    for (int i = ns - 1; i >= 0; --i) {
        const PdVtScale &S = tr->pend[i];
        const bool acc = i != ns - 1;                      // the first scale that runs writes, the others add
        const int M = S.M, rb = (M + 3) / 4, T = S.T;
        const size_t r0 = S.row0;
        const float *hl = tr->hres[2 * Lc] + r0 * d, *fst = tr->fstats + (size_t)i * tr->max_images * 2;
        if (grads->norm_w || grads->norm_b)
            hipLaunchKernelGGL(pd_vt_final_param_kernel, dim3((d + 255) / 256), dim3(256), 0, s, g_z, hl, fst, n, T, d, ns, acc ? 1 : 0, grads->norm_w,
                               grads->norm_b);
        hipLaunchKernelGGL(pd_vt_final_bwd_kernel, dim3(rb), dim3(256), 0, s, g_z, hl, fst, w->norm_w, n, T, d, ns, tr->dres);
        for (int l = Lc - 1; l >= 0; --l) {
            const pd_vit_layer_weights &Wl = w->layers[l];
            const pd_vit_layer_grads &G = grads->layers[l];
            const PdVtLayerStash &St = tr->L[l];
            const float *h0 = tr->hres[2 * l] + r0 * d, *h1 = tr->hres[2 * l + 1] + r0 * d;
            const float *qkv = St.qkv + r0 * 3 * d, *ctx = St.ctx + r0 * d, *pre = St.pre + r0 * ff;
            const float *st1 = St.stats1 + r0 * 2, *st2 = St.stats2 + r0 * 2;
            const size_t n4 = (size_t)M * ff / 4;
            // MLP sublayer: dres is the gradient of fc2's output
            if (G.fc2_w) hipLaunchKernelGGL(pd_vt_gelu_kernel, dim3(vt_blocks(n4, 4096)), dim3(256), 0, s, (const float4 *)pre, (float4 *)tr->act, n4);
            pd_tr_wgrad(tr->wk, tr->dres, tr->act, G.fc2_w, G.fc2_b, M, d, ff, acc, s);
            vt_dgrad(tr, tr->dres, Wl.fc2_w, tr->dff, M, d, ff, s);
            hipLaunchKernelGGL(pd_vt_gelu_bwd_kernel, dim3(vt_blocks(n4, 4096)), dim3(256), 0, s, (const float4 *)pre, (float4 *)tr->dff, n4);
            if (G.fc1_w) pd_tr_ln_launch(h1, tr->hn, Wl.norm2_w, Wl.norm2_b, M, d, VT_EPS, nullptr, s);
            pd_tr_wgrad(tr->wk, tr->dff, tr->hn, G.fc1_w, G.fc1_b, M, ff, d, acc, s);
            vt_dgrad(tr, tr->dff, Wl.fc1_w, tr->dhn, M, ff, d, s);
            pd_tr_ln_param_grads(tr->wk, tr->dhn, h1, st2, G.norm2_w, G.norm2_b, M, d, acc, s);
            pd_tr_ln_bwd_launch(tr->dhn, h1, st2, Wl.norm2_w, M, d, tr->dres, s);
            // attention sublayer: dres is the gradient of proj's output
            pd_tr_wgrad(tr->wk, tr->dres, ctx, G.proj_w, G.proj_b, M, d, d, acc, s);
            vt_dgrad(tr, tr->dres, Wl.proj_w, tr->dhn, M, d, d, s);
            pd_tr_attn_bwd_launch(true, qkv, tr->dhn, tr->dqkv, tr->wk.la_stats, n, T, tr->nhead, tr->hd, d, scale, nullptr, s);
            if (G.qkv_w) pd_tr_ln_launch(h0, tr->hn, Wl.norm1_w, Wl.norm1_b, M, d, VT_EPS, nullptr, s);
            pd_tr_wgrad(tr->wk, tr->dqkv, tr->hn, G.qkv_w, G.qkv_b, M, 3 * d, d, acc, s);
            vt_dgrad(tr, tr->dqkv, Wl.qkv_w, tr->dhn, M, 3 * d, d, s);
            pd_tr_ln_param_grads(tr->wk, tr->dhn, h0, st1, G.norm1_w, G.norm1_b, M, d, acc, s);
            pd_tr_ln_bwd_launch(tr->dhn, h0, st1, Wl.norm1_w, M, d, tr->dres, s);
        }
        // token assembly adjoint: dres is the gradient of x0.  dhn receives the patch GEMM's output gradient in compact rows
        hipLaunchKernelGGL(pd_vt_assemble_bwd_kernel, dim3((T * d + 255) / 256), dim3(256), 0, s, tr->dres, n, T, d, tr->dhn,
                           tr->dpos + (size_t)i * PD_VT_MAX_TOKENS * d);
        pd_tr_wgrad(tr->wk, tr->dhn, tr->cols + r0 * PD_VT_KP, grads->patch_w, grads->patch_b, n * S.P, d, PD_VT_KP, acc, s);
    }
    if (grads->cls_token || grads->pos_embed) {
        const int g = tr->grid0;
        for (int i = 0; i < ns; ++i) {                     // call order
            const PdVtScale &S = tr->pend[i];
            const float ry = (float)(1.0 / (((double)S.gh + 0.1) / (double)g)), rx = (float)(1.0 / (((double)S.gw + 0.1) / (double)g));
            hipLaunchKernelGGL(pd_vt_posgrid_kernel, dim3(((1 + g * g) * d + 255) / 256), dim3(256), 0, s, tr->dpos + (size_t)i * PD_VT_MAX_TOKENS * d, S.gh,
                               S.gw, g, d, S.resampled, i > 0 ? 1 : 0, ry, rx, grads->pos_embed, grads->cls_token);
        }
    }
    PD_HIP_CHECK(hipGetLastError());
    return PD_OK;
}
