// pd_train.hip -- the training branch with gradients (include/pd_engine_train.h): GaussianDiffusion.p_losses forward with an activation
// stash, and the backward of the diffusion loss through the Denoiser to every parameter and to z.  Kernels: pd_train_kernels.h.
//
// Replaces (paths relative to the reference's pose_diffusion/): the autograd graph of models/gaussian_diffuser.py:308-327 over
// models/denoiser.py:53-76 that train.py:245-251 back-propagates.  The LR schedule stays PyTorch's; clipping and the optimiser step are pd_optim.hip's.
//
// Forward (the generic path's structure, DESIGN 3.5, on the caller's live weights):
//   q_sample -> time embedding of the B timesteps -> _first's rows -> _first GEMM -> per layer { LN1 (+stats) -> in_proj GEMM -> attention ->
//   out_proj GEMM + residual -> LN2 (+stats) -> linear1 GEMM + ReLU -> linear2 GEMM + residual } -> _last.0 GEMM -> tail (+loss)
// The residual stream is never updated in place: hres[i] is the stream at sublayer input i (2 L + 1 arrays), which IS the stash.
// Backward: tail -> _last.0 -> per layer in reverse { linear2, ReLU mask, linear1, LN2, out_proj, attention, in_proj, LN1 } -> _first
//   (weight gradient over all columns, data gradient for the t_emb and z columns only) -> time embedding.
// Dropout (pd_train_forward_dropout): the four sites of an encoder layer are masked in the epilogues of out_proj / linear1 / linear2 and
// in the attention kernel; the backward recomputes every mask from (seed, step, p) and masks the residual-stream gradient into dres_m
// before the weight, bias and data gradients of out_proj / linear2 read it.  A call without dropout launches the DROP = false kernels.
// Attention: N <= 64 runs pd_tr_attn_kernel / pd_tr_attn_bwd_kernel (a sequence whole in LDS), N > 64 -- admitted once PD_TR_OPT_MAX_FRAMES
// raises the limit -- the key-tiled pd_tr_lattn_* kernels (pd_train_lattn.h); the family a forward ran is remembered with its stash.
// Frame counts (pd_trainer_set_frame_counts): a padded batch whose sequences have their own frame counts.  The key-tiled
// attention then serves every N with the counts as the number of keys and rows, q_sample / embed / tail treat padding rows as absent, and
// everything between is per-row work on rows whose gradient is exactly zero.  A forward copies the counts into its stash's own array.
// This file is the only one that compiles pd_train_kernels.h: the launch helpers below (pd_train_launch.h) are the backbone trainer's way
// to the same kernels (pd_vit_train.hip), with acc = false here and its per-scale accumulate switch there.
#include "pd_train_kernels.h"
#include "pd_train_launch.h"
#include "../../include/pd_engine_train.h"

#include <algorithm>
#include <string.h>

struct PdTrLayerStash {
    float *stats1, *stats2;         // [M, 2] (mean, rstd)
    float *qkv, *ctx, *ffa;         // [M, 3 d], [M, d], [M, ff] (post-ReLU)
};

struct pd_trainer {
    int d = 0, nhead = 0, hd = 0, ff = 0, z = 0, hid = 0, layers = 0, timesteps = 0, pivot = 1, pred_x0 = 0, Kf = 0;
    int max_B = 0, max_N = 0, m_cap = 0;
    // tables (copies)
    float *qa = nullptr, *qb = nullptr, *c_recip = nullptr, *c_recipm1 = nullptr;
    // stash
    float *xt = nullptr, *emb = nullptr;                 // [M, 9], [M, Kf]
    float *hres[2 * PD_MAX_LAYERS + 1] = {};             // [M, d] each
    PdTrLayerStash L[PD_MAX_LAYERS] = {};
    float *hid_pre = nullptr, *hid_post = nullptr, *hid_stats = nullptr, *dl = nullptr;   // [M, hid] x 2, [M, 2], [M, 9]
    float *t_emb256 = nullptr, *t_a0 = nullptr, *t_sact = nullptr, *t_emb = nullptr;      // [B, 256], [B, 128] x 3
    int *t_b = nullptr;                                  // [B]
    // scratch
    float *hn = nullptr, *dres = nullptr, *dhn = nullptr, *dff = nullptr, *dqkv = nullptr;
    float *dres_m = nullptr;                             // [M, d] dres masked at site 1 / 3 (dropout backward)
    float *dy_hid = nullptr, *dhid = nullptr, *gout = nullptr, *demb_t = nullptr, *dtemb = nullptr, *dts = nullptr;
    PdTrWork wk = {};                                    // split-reduction workspaces; la_stats [M nhead, 4] (row maximum, 1 / sum, rs x 2)
    size_t ws_floats = 0, ws_col_floats = 0;
    unsigned int *d_err = nullptr;
    int pend_B = 0, pend_N = 0;                          // B, N of the pending forward (0: none)
    int last_B = 0, last_N = 0;                          // of the last forward (pd_train_debug_relu)
    PdTrDrop pend_drop = {};                             // dropout of the pending forward (ctr2 / philox are set per site) ...
    unsigned pend_sites = 0;                             // ... and its sites (0: none)
    int max_frames = PD_TR_MAX_N;                        // PD_TR_OPT_MAX_FRAMES
    int long_attn = 0;                                   // PD_TR_OPT_LONG_ATTN
    int pend_long = 0;                                   // the pending forward ran the key-tiled attention: so does its backward
    // frame counts per sequence (pd_trainer_set_frame_counts): d_nf follows the entry point, d_nf_pend is the pending forward's own copy
    int *d_nf = nullptr, *d_nf_pend = nullptr;           // [max_B] each
    int *nf_host = nullptr;                              // [max_B] host copy, for validation
    int nf_B = 0;                                        // 0: no counts set
    int pend_nf = 0;                                     // the pending forward ran with counts (d_nf_pend holds them)
    PdDevAllocs mem{"pd_trainer_create"};
    ~pd_trainer() { delete[] nf_host; }
};

// ---- launch helpers shared with pd_vit_train.hip (pd_train_launch.h) --------------------------
int pd_tr_set_attention_lds() {
    const size_t sf = pd_tr_attn_lds(PD_TR_MAX_N, PD_TR_MAX_HD), sb = pd_tr_attn_bwd_lds(PD_TR_MAX_N, PD_TR_MAX_HD);
    const size_t lf = pd_tr_lattn_lds(PD_TR_LA_MAX_N, PD_TR_MAX_HD), la = pd_tr_lattn_bwd_rows_lds(PD_TR_LA_MAX_N, PD_TR_MAX_HD),
                 lb = pd_tr_lattn_bwd_keys_lds(PD_TR_LA_MAX_N, PD_TR_MAX_HD);
    const struct { const void *kernel; size_t bytes; } bounds[] = {
        {(const void *)pd_tr_attn_kernel<false>, sf}, {(const void *)pd_tr_attn_kernel<true>, sf},
        {(const void *)pd_tr_attn_bwd_kernel<false>, sb}, {(const void *)pd_tr_attn_bwd_kernel<true>, sb},
        {(const void *)pd_tr_lattn_kernel<false>, lf}, {(const void *)pd_tr_lattn_kernel<true>, lf},
        {(const void *)pd_tr_lattn_bwd_rows_kernel<false>, la}, {(const void *)pd_tr_lattn_bwd_rows_kernel<true>, la},
        {(const void *)pd_tr_lattn_bwd_keys_kernel<false>, lb}, {(const void *)pd_tr_lattn_bwd_keys_kernel<true>, lb}};
    for (const auto &b : bounds) PD_HIP_CHECK(hipFuncSetAttribute(b.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b.bytes));
    return PD_OK;
}

void pd_tr_gemm_launch(const PdTrGemm &g, int nz, hipStream_t s, const PdTrDrop *dr) {
    const dim3 grid((g.J + 63) / 64, (g.I + 63) / 64, nz);
    if (dr) hipLaunchKernelGGL(pd_tr_gemm_kernel<true>, grid, dim3(256), 0, s, g, *dr);
    else hipLaunchKernelGGL(pd_tr_gemm_kernel<false>, grid, dim3(256), 0, s, g, PdTrDrop{});
}

// the dropout of the pending / running call at `site` (0 .. 3) of `layer`, or null when that site is off
static const PdTrDrop *tr_site(const PdTrDrop &base, unsigned sites, int layer, int site, PdTrDrop *out) {
    if (!(sites & (1u << site))) return nullptr;
    *out = base;
    out->ctr2 = 4u * (unsigned)layer + (unsigned)site;
    out->philox = 1;
    return out;
}

// Y[M, Nout] = X[M, K] W[Nout, K]^T + b (+ ReLU) (+ dropout `dr`) (+ resid)
void pd_tr_linear(const float *X, const float *W, const float *b, float *Y, int M, int Nout, int K, int relu, const float *resid, hipStream_t s,
                  const PdTrDrop *dr) {
    PdTrGemm g;
    memset(&g, 0, sizeof(g));
    g.A = X; g.a_rs = K; g.a_cs = 1; g.a_rfast = 1;
    g.B = W; g.b_rs = 1; g.b_cs = K; g.b_rfast = 1;
    g.C = Y; g.ldc = Nout; g.bias = b; g.relu = relu; g.resid = resid; g.ldr = Nout;
    g.I = M; g.J = Nout; g.R = K; g.r_chunk = K;
    pd_tr_gemm_launch(g, 1, s, dr);
}

// dX[M, Kw] = dY[M, Nout] W[:, koff : koff + Kw] (W [Nout, ldw]), masked by aux (mode 1 / 2), written or accumulated into dX
static void tr_dgrad(const float *dY, const float *W, int ldw, int koff, float *dX, int M, int Nout, int Kw, const float *aux, int mask_mode,
                     bool accumulate, hipStream_t s, const PdTrDrop *dr = nullptr) {
    PdTrGemm g;
    memset(&g, 0, sizeof(g));
    g.A = dY; g.a_rs = Nout; g.a_cs = 1; g.a_rfast = 1;
    g.B = W + koff; g.b_rs = ldw; g.b_cs = 1; g.b_rfast = 0;
    g.C = dX; g.ldc = Kw; g.aux = aux; g.ldaux = Kw; g.mask_mode = aux ? mask_mode : 0;
    if (accumulate) {
        g.resid = dX;
        g.ldr = Kw;
    }
    g.I = M; g.J = Kw; g.R = Nout; g.r_chunk = Nout;
    pd_tr_gemm_launch(g, 1, s, dr);
}

// out[e] (+)= ws[0][e] + ... + ws[nz - 1][e]
template <typename T>
static void tr_reduce(const T *ws, long long total, int nz, float *out, bool acc, hipStream_t s) {
    const dim3 grid((unsigned)std::min<long long>((total + 255) / 256, 2048));      // (a column sum's total, at most 8192, never meets the cap)
    if (acc) hipLaunchKernelGGL((pd_tr_reduce_kernel<T, true>), grid, dim3(256), 0, s, ws, total, nz, out);
    else hipLaunchKernelGGL((pd_tr_reduce_kernel<T, false>), grid, dim3(256), 0, s, ws, total, nz, out);
}

void pd_tr_reduce_launch(const float *ws, long long total, int nz, float *out, hipStream_t s) { tr_reduce(ws, total, nz, out, false, s); }

// dW[Nout, K] (+)= sum_m dY[m, :]^T X[m, :] over the chunks of M, partials added in chunk order; db[Nout] (+)= sum_m dY[m, :] likewise
void pd_tr_wgrad(const PdTrWork &wk, const float *dY, const float *X, float *dW, float *db, int M, int Nout, int K, bool acc, hipStream_t s) {
    int nch, rows;
    pd_tr_chunks(M, &nch, &rows);
    if (dW) {
        PdTrGemm g;
        memset(&g, 0, sizeof(g));
        g.A = dY; g.a_rs = 1; g.a_cs = Nout; g.a_rfast = 0;
        g.B = X; g.b_rs = K; g.b_cs = 1; g.b_rfast = 0;
        g.C = nch > 1 ? wk.ws : dW; g.ldc = K;
        if (nch == 1 && acc) {
            g.resid = dW;
            g.ldr = K;
        }
        g.I = Nout; g.J = K; g.R = M; g.r_chunk = rows;
        pd_tr_gemm_launch(g, nch, s);
        if (nch > 1) tr_reduce(wk.ws, (long long)Nout * K, nch, dW, acc, s);
    }
    if (db) {
        hipLaunchKernelGGL(pd_tr_colsum_kernel<false>, dim3((Nout + 63) / 64, nch), dim3(256), 0, s, dY, (long long)Nout, nullptr, 0LL, nullptr, M, Nout, rows,
                           nullptr, wk.ws_col);
        tr_reduce(wk.ws_col, (long long)Nout, nch, db, acc, s);
    }
}

// LayerNorm's dgamma (+)= sum_m dy xhat, dbeta (+)= sum_m dy
void pd_tr_ln_param_grads(const PdTrWork &wk, const float *dy, const float *x, const float *stats, float *dgamma, float *dbeta, int M, int D, bool acc,
                          hipStream_t s) {
    if (!dgamma && !dbeta) return;
    int nch, rows;
    pd_tr_chunks(M, &nch, &rows);
    double *pa = wk.ws_col, *pb = wk.ws_col + (size_t)PD_TR_MAX_CHUNKS * D;       // [chunks][D] each
    hipLaunchKernelGGL(pd_tr_colsum_kernel<true>, dim3((D + 63) / 64, nch), dim3(256), 0, s, dy, (long long)D, x, (long long)D, stats, M, D, rows, pa, pb);
    if (dgamma) tr_reduce(pa, (long long)D, nch, dgamma, acc, s);
    if (dbeta) tr_reduce(pb, (long long)D, nch, dbeta, acc, s);
}

void pd_tr_ln_launch(const float *in, float *out, const float *gamma, const float *beta, int M, int D, float eps, float *stats, hipStream_t s) {
    hipLaunchKernelGGL(pd_tr_ln_kernel, dim3((M + 3) / 4), dim3(256), 0, s, in, out, gamma, beta, M, D, eps, stats);
}

void pd_tr_ln_bwd_launch(const float *dy, const float *x, const float *stats, const float *gamma, int M, int D, float *dres, hipStream_t s) {
    hipLaunchKernelGGL(pd_tr_ln_bwd_kernel, dim3((M + 3) / 4), dim3(256), 0, s, dy, x, stats, gamma, M, D, dres);
}

// attention forward of one layer: the short kernel (a sequence whole in LDS) or the key-tiled one
void pd_tr_attn_launch(bool tiled, const float *qkv, float *ctx, int B, int N, int nh, int hd, int d, float scale, const PdTrDrop *dr, hipStream_t s,
                       const int *nf) {
    if (tiled) {
        const dim3 grid(B * nh, (N + PD_TR_LA_ROWS - 1) / PD_TR_LA_ROWS);
        if (dr) hipLaunchKernelGGL(pd_tr_lattn_kernel<true>, grid, dim3(256), pd_tr_lattn_lds(N, hd), s, qkv, ctx, nf, N, nh, hd, d, scale, *dr);
        else hipLaunchKernelGGL(pd_tr_lattn_kernel<false>, grid, dim3(256), pd_tr_lattn_lds(N, hd), s, qkv, ctx, nf, N, nh, hd, d, scale, PdTrDrop{});
    } else if (dr) {
        hipLaunchKernelGGL(pd_tr_attn_kernel<true>, dim3(B * nh), dim3(256), pd_tr_attn_lds(N, hd), s, qkv, ctx, N, nh, hd, d, scale, *dr);
    } else {
        hipLaunchKernelGGL(pd_tr_attn_kernel<false>, dim3(B * nh), dim3(256), pd_tr_attn_lds(N, hd), s, qkv, ctx, N, nh, hd, d, scale, PdTrDrop{});
    }
}

// attention backward of one layer: dqkv from qkv and dctx; tiled = phase A (dQ, row statistics) then phase B (dK, dV)
void pd_tr_attn_bwd_launch(bool tiled, const float *qkv, const float *dctx, float *dqkv, float *la_stats, int B, int N, int nh, int hd, int d,
                           float scale, const PdTrDrop *dr, hipStream_t s, const int *nf) {
    if (tiled) {
        const dim3 rows(B * nh, (N + PD_TR_LA_ROWS - 1) / PD_TR_LA_ROWS), keys(B * nh, pd_tr_la_tiles(N));
        const size_t la = pd_tr_lattn_bwd_rows_lds(N, hd), lb = pd_tr_lattn_bwd_keys_lds(N, hd);
        if (dr) {
            hipLaunchKernelGGL(pd_tr_lattn_bwd_rows_kernel<true>, rows, dim3(256), la, s, qkv, dctx, dqkv, la_stats, nf, N, nh, hd, d, scale, *dr);
            hipLaunchKernelGGL(pd_tr_lattn_bwd_keys_kernel<true>, keys, dim3(256), lb, s, qkv, dctx, dqkv, la_stats, nf, N, nh, hd, d, scale, *dr);
        } else {
            hipLaunchKernelGGL(pd_tr_lattn_bwd_rows_kernel<false>, rows, dim3(256), la, s, qkv, dctx, dqkv, la_stats, nf, N, nh, hd, d, scale, PdTrDrop{});
            hipLaunchKernelGGL(pd_tr_lattn_bwd_keys_kernel<false>, keys, dim3(256), lb, s, qkv, dctx, dqkv, la_stats, nf, N, nh, hd, d, scale, PdTrDrop{});
        }
    } else if (dr) {
        hipLaunchKernelGGL(pd_tr_attn_bwd_kernel<true>, dim3(B * nh), dim3(256), pd_tr_attn_bwd_lds(N, hd), s, qkv, dctx, dqkv, N, nh, hd, d, scale, *dr);
    } else {
        hipLaunchKernelGGL(pd_tr_attn_bwd_kernel<false>, dim3(B * nh), dim3(256), pd_tr_attn_bwd_lds(N, hd), s, qkv, dctx, dqkv, N, nh, hd, d, scale, PdTrDrop{});
    }
}

// ---- shape checks ----------------------------------------------------------------------------
static int tr_shape_check(const pd_weights *w, const char *who) {
    const int d = w->d_model, nh = w->nhead;
    const char *msg = nullptr;
    if (d < 32 || d > 2048 || d % 32) msg = "d_model must be a multiple of 32 in [32, 2048]";
    else if (nh < 1 || d % nh) msg = "nhead must divide d_model";
    else if ((d / nh) % 4 || d / nh < 8) msg = "the head dim d_model / nhead must be a multiple of 4, at least 8";
    else if (d / nh > PD_TR_MAX_HD) msg = "the trainer's attention backward takes a head dim of at most 128";
    else if (w->reserved & PD_WEIGHTS_POST_NORM) msg = "the trainer is pre-norm only (norm_first=True); post-norm has no backward";
    else if (w->dim_ff < 1 || w->dim_ff > 8192) msg = "dim_feedforward must be in [1, 8192]";
    else if (w->num_layers < 1 || w->num_layers > PD_MAX_LAYERS) msg = "num_encoder_layers must be in [1, PD_MAX_LAYERS = 16]";
    else if (w->z_dim < 1 || w->z_dim > 4096) msg = "z_dim must be in [1, 4096]";
    else if (w->mlp_hidden < 1 || w->mlp_hidden > 1024) msg = "mlp_hidden_dim must be in [1, 1024]";
    else if (w->n_harmonic != 10 || w->t_emb_dim != 256) msg = "the pose / time embeddings must be the reference's (10 harmonics, t_emb 256)";
    else if (w->timesteps < 1) msg = "timesteps must be positive";
    if (msg) {
        pd_set_error("%s: unsupported configuration: %s (d_model=%d nhead=%d ff=%d layers=%d z=%d hidden=%d flags=%d)", who, msg, d, nh, w->dim_ff,
                     w->num_layers, w->z_dim, w->mlp_hidden, w->reserved);
        return PD_ERR_UNSUPPORTED;
    }
    return PD_OK;
}

extern "C" int pd_trainer_create(const pd_weights *shape, const float *sqrt_alphas_cumprod, const float *sqrt_one_minus_alphas_cumprod,
                                 int max_B, int max_N, pd_trainer **out) {
    if (!shape || !out || !sqrt_alphas_cumprod || !sqrt_one_minus_alphas_cumprod || max_B < 1 || max_N < 1) {
        pd_set_error("pd_trainer_create: invalid arguments (NULL shape / tables / out, or max_B=%d max_N=%d not positive)", max_B, max_N);
        return PD_ERR_INVALID_ARG;
    }
    *out = nullptr;
    PD_TRY(tr_shape_check(shape, "pd_trainer_create"));
    pd_trainer *tr = new pd_trainer();
    tr->d = shape->d_model; tr->nhead = shape->nhead; tr->hd = tr->d / tr->nhead; tr->ff = shape->dim_ff; tr->z = shape->z_dim;
    tr->hid = shape->mlp_hidden; tr->layers = shape->num_layers; tr->timesteps = shape->timesteps;
    tr->pivot = (shape->reserved & PD_WEIGHTS_NO_PIVOT) ? 0 : 1;
    tr->pred_x0 = (shape->reserved & PD_WEIGHTS_PRED_X0) ? 1 : 0;
    tr->Kf = PD_TR_FIRST_FIXED + tr->z + tr->pivot;
    tr->max_B = max_B; tr->max_N = max_N; tr->m_cap = max_B * max_N;
    const size_t rows = (size_t)tr->m_cap, d = tr->d, T = tr->timesteps;
    int rc = PD_OK;
#define TR_A(p, n) if (rc == PD_OK) rc = tr->mem.alloc(&(p), (size_t)(n), true)
    TR_A(tr->qa, T); TR_A(tr->qb, T);
    if (shape->sqrt_recip_alphas_cumprod && shape->sqrt_recipm1_alphas_cumprod) {
        TR_A(tr->c_recip, T); TR_A(tr->c_recipm1, T);
    }
    TR_A(tr->xt, rows * 9); TR_A(tr->emb, rows * tr->Kf);
    for (int i = 0; i <= 2 * tr->layers; ++i) TR_A(tr->hres[i], rows * d);
    for (int l = 0; l < tr->layers; ++l) {
        TR_A(tr->L[l].stats1, rows * 2); TR_A(tr->L[l].stats2, rows * 2);
        TR_A(tr->L[l].qkv, rows * 3 * d); TR_A(tr->L[l].ctx, rows * d); TR_A(tr->L[l].ffa, rows * tr->ff);
    }
    TR_A(tr->hid_pre, rows * tr->hid); TR_A(tr->hid_post, rows * tr->hid); TR_A(tr->hid_stats, rows * 2); TR_A(tr->dl, rows * 9);
    TR_A(tr->t_emb256, (size_t)max_B * 256); TR_A(tr->t_a0, (size_t)max_B * 128); TR_A(tr->t_sact, (size_t)max_B * 128); TR_A(tr->t_emb, (size_t)max_B * 128);
    TR_A(tr->t_b, (size_t)max_B);
    TR_A(tr->hn, rows * d); TR_A(tr->dres, rows * d); TR_A(tr->dres_m, rows * d); TR_A(tr->dhn, rows * d); TR_A(tr->dff, rows * tr->ff); TR_A(tr->dqkv, rows * 3 * d);
    TR_A(tr->dy_hid, rows * tr->hid); TR_A(tr->dhid, rows * tr->hid); TR_A(tr->gout, rows * 9); TR_A(tr->demb_t, rows * 128);
    TR_A(tr->dtemb, (size_t)max_B * 128); TR_A(tr->dts, (size_t)max_B * 128);
    TR_A(tr->wk.la_stats, rows * tr->nhead * PD_TR_LA_STATS);
    const size_t widest_w = std::max({(size_t)d * tr->Kf, (size_t)3 * d * d, (size_t)tr->ff * d, (size_t)tr->hid * d, (size_t)9 * tr->hid, (size_t)128 * 256});
    tr->ws_floats = widest_w * PD_TR_MAX_CHUNKS;
    const size_t widest_c = std::max({(size_t)3 * d, (size_t)tr->ff, (size_t)tr->hid, (size_t)256});
    tr->ws_col_floats = 2 * widest_c * PD_TR_MAX_CHUNKS;
    TR_A(tr->wk.ws, tr->ws_floats); TR_A(tr->wk.ws_col, tr->ws_col_floats);
    TR_A(tr->d_err, 4);
    TR_A(tr->d_nf, (size_t)max_B); TR_A(tr->d_nf_pend, (size_t)max_B);
#undef TR_A
    tr->nf_host = new int[max_B]();
    if (rc == PD_OK && hipMemcpy(tr->qa, sqrt_alphas_cumprod, T * sizeof(float), hipMemcpyDeviceToDevice) != hipSuccess) rc = PD_ERR_HIP;
    if (rc == PD_OK && hipMemcpy(tr->qb, sqrt_one_minus_alphas_cumprod, T * sizeof(float), hipMemcpyDeviceToDevice) != hipSuccess) rc = PD_ERR_HIP;
    if (rc == PD_OK && tr->c_recip) {
        if (hipMemcpy(tr->c_recip, shape->sqrt_recip_alphas_cumprod, T * sizeof(float), hipMemcpyDeviceToDevice) != hipSuccess ||
            hipMemcpy(tr->c_recipm1, shape->sqrt_recipm1_alphas_cumprod, T * sizeof(float), hipMemcpyDeviceToDevice) != hipSuccess)
            rc = PD_ERR_HIP;
    }
    if (rc == PD_OK) rc = pd_tr_set_attention_lds();
    if (rc == PD_OK && hipDeviceSynchronize() != hipSuccess) rc = PD_ERR_HIP;
    if (rc != PD_OK) {
        if (rc == PD_ERR_HIP) pd_set_error("pd_trainer_create: a HIP call failed: %s", hipGetErrorString(hipGetLastError()));
        delete tr;
        return rc;
    }
    *out = tr;
    return PD_OK;
}

extern "C" void pd_trainer_destroy(pd_trainer *tr) { delete tr; }

extern "C" int pd_trainer_set_option(pd_trainer *tr, int option, int value) {
    if (!tr) {
        pd_set_error("pd_trainer_set_option: NULL trainer");
        return PD_ERR_INVALID_ARG;
    }
    if (option == PD_TR_OPT_MAX_FRAMES) {
        if (value < PD_TR_MAX_N || value > PD_TR_LA_MAX_N) {
            pd_set_error("pd_trainer_set_option: PD_TR_OPT_MAX_FRAMES=%d is outside [%d, %d]", value, PD_TR_MAX_N, PD_TR_LA_MAX_N);
            return PD_ERR_INVALID_ARG;
        }
        tr->max_frames = value;
    } else if (option == PD_TR_OPT_LONG_ATTN) {
        if (value != 0 && value != 1) {
            pd_set_error("pd_trainer_set_option: PD_TR_OPT_LONG_ATTN=%d must be 0 or 1", value);
            return PD_ERR_INVALID_ARG;
        }
        tr->long_attn = value;
    } else {
        pd_set_error("pd_trainer_set_option: unknown option %d (value %d)", option, value);
        return PD_ERR_INVALID_ARG;
    }
    return PD_OK;
}

extern "C" int pd_trainer_get_option(pd_trainer *tr, int option, int *value) {
    if (!tr || !value) {
        pd_set_error("pd_trainer_get_option: NULL trainer or value");
        return PD_ERR_INVALID_ARG;
    }
    if (option == PD_TR_OPT_MAX_FRAMES) *value = tr->max_frames;
    else if (option == PD_TR_OPT_LONG_ATTN) *value = tr->long_attn;
    else {
        pd_set_error("pd_trainer_get_option: unknown option %d", option);
        return PD_ERR_INVALID_ARG;
    }
    return PD_OK;
}

extern "C" int pd_trainer_set_frame_counts(pd_trainer *tr, int B, const int32_t *n_frames, void *stream) {
    if (!tr) {
        pd_set_error("pd_trainer_set_frame_counts: NULL trainer");
        return PD_ERR_INVALID_ARG;
    }
    if (!n_frames || B == 0) {
        tr->nf_B = 0;                // cleared: every later forward is a uniform one (a pending stash keeps its own counts)
        return PD_OK;
    }
    if (B < 0 || B > tr->max_B) {
        pd_set_error("pd_trainer_set_frame_counts: B=%d must lie in [0, max_B=%d]", B, tr->max_B);
        return PD_ERR_INVALID_ARG;
    }
    const int cap = std::min(tr->max_N, PD_TR_LA_MAX_N);
    for (int b = 0; b < B; ++b)
        if (n_frames[b] < 1 || n_frames[b] > cap) {
            pd_set_error("pd_trainer_set_frame_counts: n_frames[%d]=%d: every count must lie in [1, N] (N <= %d)", b, (int)n_frames[b], cap);
            return PD_ERR_INVALID_ARG;
        }
    hipStream_t s = (hipStream_t)stream;
    for (int first = 0; first < B; first += PD_TR_NF_CHUNK) {
        const int n = std::min(PD_TR_NF_CHUNK, B - first);
        PdTrCountsChunk c;
        memset(&c, 0, sizeof(c));
        for (int i = 0; i < n; ++i) c.w[i >> 2] |= (unsigned)(n_frames[first + i] - 1) << (8 * (i & 3));
        hipLaunchKernelGGL(pd_tr_set_counts_kernel, dim3((n + 255) / 256), dim3(256), 0, s, c, first, n, tr->d_nf);
    }
    PD_HIP_CHECK(hipGetLastError());
    for (int b = 0; b < B; ++b) tr->nf_host[b] = n_frames[b];
    tr->nf_B = B;
    return PD_OK;
}

static int tr_weights_match(const pd_trainer *tr, const pd_weights *w, const char *who) {
    if (!w) {
        pd_set_error("%s: NULL weights", who);
        return PD_ERR_INVALID_ARG;
    }
    const int pivot = (w->reserved & PD_WEIGHTS_NO_PIVOT) ? 0 : 1, px0 = (w->reserved & PD_WEIGHTS_PRED_X0) ? 1 : 0;
    if (w->d_model != tr->d || w->nhead != tr->nhead || w->dim_ff != tr->ff || w->num_layers != tr->layers || w->z_dim != tr->z ||
        w->mlp_hidden != tr->hid || w->timesteps != tr->timesteps || pivot != tr->pivot || px0 != tr->pred_x0 || (w->reserved & PD_WEIGHTS_POST_NORM)) {
        pd_set_error("%s: the weights' shape fields / flags differ from the shape this trainer was created for", who);
        return PD_ERR_INVALID_ARG;
    }
    bool ok = w->time_w0 && w->time_b0 && w->time_w2 && w->time_b2 && w->first_w && w->first_b && w->last0_w && w->last0_b && w->last_ln_w &&
              w->last_ln_b && w->last3_w && w->last3_b;
    for (int l = 0; l < tr->layers && ok; ++l) {
        const pd_layer_weights &L = w->layers[l];
        ok = L.norm1_w && L.norm1_b && L.in_proj_w && L.in_proj_b && L.out_proj_w && L.out_proj_b && L.norm2_w && L.norm2_b && L.linear1_w &&
             L.linear1_b && L.linear2_w && L.linear2_b;
    }
    if (!ok) {
        pd_set_error("%s: a weight pointer is NULL", who);
        return PD_ERR_INVALID_ARG;
    }
    return PD_OK;
}

// pd_train_forward (sites = 0) and pd_train_forward_dropout: `drop` holds thr / key / step / scale of the call
static int tr_forward(pd_trainer *tr, const pd_weights *w, const float *x_start, const float *z, const int64_t *t_seq, const float *noise, int B,
                      int N, int loss_type, const PdTrDrop &drop, unsigned sites, const char *who, float *loss_out, float *x0_pred_out, float *xt_out,
                      float *model_out, void *stream) {
    if (!x_start || !z || !t_seq || !noise || !loss_out || B < 1 || N < 1 || B > tr->max_B || N > tr->max_N || (loss_type != 1 && loss_type != 2)) {
        pd_set_error("%s: invalid arguments (B=%d N=%d loss_type=%d; max_B=%d max_N=%d; x_start, z, t_seq, noise and loss_out must not be NULL)",
                     who, B, N, loss_type, tr->max_B, tr->max_N);
        return PD_ERR_INVALID_ARG;
    }
    if (N > tr->max_frames) {
        if (tr->max_frames == PD_TR_MAX_N)
            pd_set_error("%s: N=%d exceeds the trainer's limit of %d frames per sequence (the attention backward holds a sequence in LDS)", who, N, PD_TR_MAX_N);
        else
            pd_set_error("%s: N=%d exceeds the trainer's limit of %d frames per sequence (PD_TR_OPT_MAX_FRAMES)", who, N, tr->max_frames);
        return PD_ERR_UNSUPPORTED;
    }
    if (tr->nf_B) {
        if (B != tr->nf_B) {
            pd_set_error("%s: frame counts per sequence are set for B=%d (pd_trainer_set_frame_counts), called with B=%d: a call must use the B "
                         "of the counts, or clear them", who, tr->nf_B, B);
            return PD_ERR_INVALID_ARG;
        }
        for (int b = 0; b < B; ++b)
            if (tr->nf_host[b] > N) {
                pd_set_error("%s: n_frames[%d]=%d (pd_trainer_set_frame_counts) exceeds N=%d: every count must lie in [1, N]", who, b, tr->nf_host[b], N);
                return PD_ERR_INVALID_ARG;
            }
    }
    PD_TRY(tr_weights_match(tr, w, who));
    if (x0_pred_out && !tr->pred_x0 && !tr->c_recip) {
        pd_set_error("%s: x0_pred_out under pred_noise needs sqrt_recip / sqrt_recipm1_alphas_cumprod at pd_trainer_create", who);
        return PD_ERR_STATE;
    }
    hipStream_t s = (hipStream_t)stream;
    const int M = B * N, d = tr->d, rb = (M + 3) / 4;
    tr->pend_B = tr->pend_N = 0;
    tr->pend_sites = 0;
    // with counts the key-tiled family serves every N; the counts of this forward become its stash's own
    const int *nf = nullptr;
    if (tr->nf_B) {
        hipLaunchKernelGGL(pd_tr_copy_counts_kernel, dim3((B + 255) / 256), dim3(256), 0, s, tr->d_nf, B, tr->d_nf_pend);
        nf = tr->d_nf_pend;
    }
    const bool tiled = tr->long_attn || N > PD_TR_MAX_N || nf;
    PdTrDrop site;
    float *xt = tr->xt;
    hipLaunchKernelGGL(pd_tr_q_sample_kernel, dim3((M * 9 + 255) / 256), dim3(256), 0, s, x_start, noise, t_seq, tr->qa, tr->qb, nf, M, N, tr->timesteps,
                       xt, tr->t_b, tr->d_err);
    hipLaunchKernelGGL(pd_tr_time_kernel, dim3(B), dim3(128), 0, s, tr->t_b, w->time_w0, w->time_b0, w->time_w2, w->time_b2, tr->t_emb256, tr->t_a0,
                       tr->t_sact, tr->t_emb);
    {
        const size_t total = (size_t)M * tr->Kf;
        hipLaunchKernelGGL(pd_tr_embed_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, s, xt, z, tr->t_emb, nf, M, N,
                           tr->z, tr->pivot, tr->Kf, tr->emb);
    }
    pd_tr_linear(tr->emb, w->first_w, w->first_b, tr->hres[0], M, d, tr->Kf, 0, nullptr, s);
    const float scale = 1.0f / sqrtf((float)tr->hd);
    for (int l = 0; l < tr->layers; ++l) {
        const pd_layer_weights &W = w->layers[l];
        const PdTrLayerStash &S = tr->L[l];
        float *h0 = tr->hres[2 * l], *h1 = tr->hres[2 * l + 1], *h2 = tr->hres[2 * l + 2];
        pd_tr_ln_launch(h0, tr->hn, W.norm1_w, W.norm1_b, M, d, 1e-5f, S.stats1, s);
        pd_tr_linear(tr->hn, W.in_proj_w, W.in_proj_b, S.qkv, M, 3 * d, d, 0, nullptr, s);
        pd_tr_attn_launch(tiled, S.qkv, S.ctx, B, N, tr->nhead, tr->hd, d, scale, tr_site(drop, sites, l, 0, &site), s, nf);
        pd_tr_linear(S.ctx, W.out_proj_w, W.out_proj_b, h1, M, d, d, 0, h0, s, tr_site(drop, sites, l, 1, &site));
        pd_tr_ln_launch(h1, tr->hn, W.norm2_w, W.norm2_b, M, d, 1e-5f, S.stats2, s);
        pd_tr_linear(tr->hn, W.linear1_w, W.linear1_b, S.ffa, M, tr->ff, d, 1, nullptr, s, tr_site(drop, sites, l, 2, &site));
        pd_tr_linear(S.ffa, W.linear2_w, W.linear2_b, h2, M, d, tr->ff, 0, h1, s, tr_site(drop, sites, l, 3, &site));
    }
    pd_tr_linear(tr->hres[2 * tr->layers], w->last0_w, w->last0_b, tr->hid_pre, M, tr->hid, d, 0, nullptr, s);
    PdTrTail ta;
    memset(&ta, 0, sizeof(ta));
    ta.hid = tr->hid_pre; ta.lnw = w->last_ln_w; ta.lnb = w->last_ln_b; ta.w3 = w->last3_w; ta.b3 = w->last3_b;
    ta.xt = xt; ta.target = tr->pred_x0 ? x_start : noise; ta.t_b = tr->t_b; ta.nf = nf; ta.c_recip = tr->c_recip; ta.c_recipm1 = tr->c_recipm1;
    ta.loss_out = loss_out; ta.x0_out = x0_pred_out; ta.model_out = model_out;
    ta.stats = tr->hid_stats; ta.hid_post = tr->hid_post; ta.dl = tr->dl;
    ta.M = M; ta.H = tr->hid; ta.n_frames = N; ta.pred_x0 = tr->pred_x0; ta.loss_type = loss_type;
    hipLaunchKernelGGL(pd_tr_tail_kernel, dim3(rb), dim3(256), 0, s, ta);
    if (xt_out) PD_HIP_CHECK(hipMemcpyAsync(xt_out, xt, (size_t)M * 9 * sizeof(float), hipMemcpyDeviceToDevice, s));
    PD_HIP_CHECK(hipGetLastError());
    tr->pend_B = tr->last_B = B;
    tr->pend_N = tr->last_N = N;
    tr->pend_drop = drop;
    tr->pend_sites = sites;
    tr->pend_long = tiled ? 1 : 0;
    tr->pend_nf = nf ? 1 : 0;
    return PD_OK;
}

extern "C" int pd_train_forward(pd_trainer *tr, const pd_weights *w, const float *x_start, const float *z, const int64_t *t_seq,
                                const float *noise, int B, int N, int loss_type, float *loss_out, float *x0_pred_out, float *xt_out,
                                float *model_out, void *stream) {
    if (!tr) {
        pd_set_error("pd_train_forward: NULL trainer");
        return PD_ERR_INVALID_ARG;
    }
    return tr_forward(tr, w, x_start, z, t_seq, noise, B, N, loss_type, PdTrDrop{}, 0u, "pd_train_forward", loss_out, x0_pred_out, xt_out, model_out, stream);
}

extern "C" int pd_train_forward_dropout(pd_trainer *tr, const pd_weights *w, const float *x_start, const float *z, const int64_t *t_seq,
                                        const float *noise, int B, int N, int loss_type, float p, unsigned sites, uint64_t seed, uint32_t step,
                                        float *loss_out, float *x0_pred_out, float *xt_out, float *model_out, void *stream) {
    if (!tr) {
        pd_set_error("pd_train_forward_dropout: NULL trainer");
        return PD_ERR_INVALID_ARG;
    }
    if (!(p >= 0.0f && p < 1.0f)) {                      // NaN fails both comparisons
        pd_set_error("pd_train_forward_dropout: invalid argument p=%g: the dropout probability must lie in [0, 1)", (double)p);
        return PD_ERR_INVALID_ARG;
    }
    if (sites & ~PD_DROP_ALL) {
        pd_set_error("pd_train_forward_dropout: invalid argument sites=0x%x: only the bits of PD_DROP_ALL (0x%x) are defined", sites, PD_DROP_ALL);
        return PD_ERR_INVALID_ARG;
    }
    PdTrDrop drop = {};
    if (p == 0.0f) sites = 0;                            // pd_train_forward itself: same launches, same bits
    if (sites) {
        drop.thr = (unsigned int)floor((double)p * 4294967296.0);
        drop.scale = 1.0f / (1.0f - p);
        drop.key0 = (unsigned int)(seed & 0xffffffffu);
        drop.key1 = (unsigned int)(seed >> 32);
        drop.step = step;
    }
    return tr_forward(tr, w, x_start, z, t_seq, noise, B, N, loss_type, drop, sites, "pd_train_forward_dropout", loss_out, x0_pred_out, xt_out, model_out, stream);
}

// pd_train_backward (g_loss alone) and pd_train_backward_ex: `who` names the entry point in every message
static int tr_backward(pd_trainer *tr, const pd_weights *w, const float *g_loss, const float *g_model_out, const float *g_x0_pred,
                       const pd_weight_grads *grads, float *dz_out, void *stream, const char *who) {
    if (tr->pend_B < 1 || tr->pend_N < 1) {
        pd_set_error("%s: no forward is pending (pd_train_forward fills the stash that one backward consumes)", who);
        return PD_ERR_STATE;
    }
    if (g_x0_pred && !tr->pred_x0 && !tr->c_recipm1) {
        pd_set_error("%s: g_x0_pred under pred_noise needs sqrt_recip / sqrt_recipm1_alphas_cumprod at pd_trainer_create", who);
        return PD_ERR_STATE;
    }
    PD_TRY(tr_weights_match(tr, w, who));
    hipStream_t s = (hipStream_t)stream;
    const int B = tr->pend_B, N = tr->pend_N, M = B * N, d = tr->d, ff = tr->ff, hid = tr->hid, rb = (M + 3) / 4, Lc = tr->layers;
    tr->pend_B = tr->pend_N = 0;
    const PdTrDrop &drop = tr->pend_drop;
    const unsigned sites = tr->pend_sites;
    const int *nf = tr->pend_nf ? tr->d_nf_pend : nullptr;   // the forward's counts, whatever pd_trainer_set_frame_counts did since
    PdTrDrop site;
    const unsigned mask_blocks = (unsigned)std::min<long long>(((long long)((M + 3) / 4) * d + 255) / 256, 4096);
    // tail: loss derivative -> _last.3 -> ReLU mask -> LayerNorm(hidden) backward
    PdTrTailBwd tb;
    memset(&tb, 0, sizeof(tb));
    tb.g_loss = g_loss; tb.g_mo = g_model_out; tb.g_x0 = g_x0_pred; tb.c_recipm1 = tr->c_recipm1; tb.t_b = tr->t_b; tb.pred_x0 = tr->pred_x0;
    tb.dl = tr->dl; tb.w3 = w->last3_w; tb.lnw = w->last_ln_w; tb.hid = tr->hid_pre; tb.hid_post = tr->hid_post; tb.stats = tr->hid_stats;
    tb.gout = tr->gout; tb.dy = tr->dy_hid; tb.dhid = tr->dhid; tb.M = M; tb.H = hid; tb.n_frames = N; tb.nf = nf;
    hipLaunchKernelGGL(pd_tr_tail_bwd_kernel, dim3(rb), dim3(256), 0, s, tb);
    pd_tr_wgrad(tr->wk, tr->gout, tr->hid_post, grads->last3_w, grads->last3_b, M, 9, hid, false, s);
    pd_tr_ln_param_grads(tr->wk, tr->dy_hid, tr->hid_pre, tr->hid_stats, grads->last_ln_w, grads->last_ln_b, M, hid, false, s);
    pd_tr_wgrad(tr->wk, tr->dhid, tr->hres[2 * Lc], grads->last0_w, grads->last0_b, M, hid, d, false, s);
    tr_dgrad(tr->dhid, w->last0_w, d, 0, tr->dres, M, hid, d, nullptr, 0, false, s);
    const float scale = 1.0f / sqrtf((float)tr->hd);
    for (int l = Lc - 1; l >= 0; --l) {
        const pd_layer_weights &W = w->layers[l];
        const pd_layer_grads &G = grads->layers[l];
        const PdTrLayerStash &S = tr->L[l];
        const float *h0 = tr->hres[2 * l], *h1 = tr->hres[2 * l + 1];
        // feed-forward sublayer: dres is the gradient of linear2's output
        // (dropout: linear2's dY is dres masked at site 3; the stash is post-dropout, so "aux > 0" is "ReLU passed and kept", times scale)
        const float *dy2 = tr->dres;
        if (const PdTrDrop *dr = tr_site(drop, sites, l, 3, &site)) {
            hipLaunchKernelGGL(pd_tr_dropmask_kernel, dim3(mask_blocks), dim3(256), 0, s, tr->dres, tr->dres_m, M, d, *dr);
            dy2 = tr->dres_m;
        }
        const PdTrDrop *ffs = tr_site(drop, sites, l, 2, &site);
        if (ffs) site.philox = 0;
        pd_tr_wgrad(tr->wk, dy2, S.ffa, G.linear2_w, G.linear2_b, M, d, ff, false, s);
        tr_dgrad(dy2, W.linear2_w, ff, 0, tr->dff, M, d, ff, S.ffa, 1, false, s, ffs);
        if (G.linear1_w) pd_tr_ln_launch(h1, tr->hn, W.norm2_w, W.norm2_b, M, d, 1e-5f, S.stats2, s);
        pd_tr_wgrad(tr->wk, tr->dff, tr->hn, G.linear1_w, G.linear1_b, M, ff, d, false, s);
        tr_dgrad(tr->dff, W.linear1_w, d, 0, tr->dhn, M, ff, d, nullptr, 0, false, s);
        pd_tr_ln_param_grads(tr->wk, tr->dhn, h1, S.stats2, G.norm2_w, G.norm2_b, M, d, false, s);
        pd_tr_ln_bwd_launch(tr->dhn, h1, S.stats2, W.norm2_w, M, d, tr->dres, s);
        // attention sublayer: dres is the gradient of out_proj's output
        const float *dy1 = tr->dres;
        if (const PdTrDrop *dr = tr_site(drop, sites, l, 1, &site)) {
            hipLaunchKernelGGL(pd_tr_dropmask_kernel, dim3(mask_blocks), dim3(256), 0, s, tr->dres, tr->dres_m, M, d, *dr);
            dy1 = tr->dres_m;
        }
        pd_tr_wgrad(tr->wk, dy1, S.ctx, G.out_proj_w, G.out_proj_b, M, d, d, false, s);
        tr_dgrad(dy1, W.out_proj_w, d, 0, tr->dhn, M, d, d, nullptr, 0, false, s);
        pd_tr_attn_bwd_launch(tr->pend_long != 0, S.qkv, tr->dhn, tr->dqkv, tr->wk.la_stats, B, N, tr->nhead, tr->hd, d, scale, tr_site(drop, sites, l, 0, &site), s, nf);
        if (G.in_proj_w) pd_tr_ln_launch(h0, tr->hn, W.norm1_w, W.norm1_b, M, d, 1e-5f, S.stats1, s);
        pd_tr_wgrad(tr->wk, tr->dqkv, tr->hn, G.in_proj_w, G.in_proj_b, M, 3 * d, d, false, s);
        tr_dgrad(tr->dqkv, W.in_proj_w, d, 0, tr->dhn, M, 3 * d, d, nullptr, 0, false, s);
        pd_tr_ln_param_grads(tr->wk, tr->dhn, h0, S.stats1, G.norm1_w, G.norm1_b, M, d, false, s);
        pd_tr_ln_bwd_launch(tr->dhn, h0, S.stats1, W.norm1_w, M, d, tr->dres, s);
    }
    // head of the network: dres is the gradient of _first's output
    pd_tr_wgrad(tr->wk, tr->dres, tr->emb, grads->first_w, grads->first_b, M, d, tr->Kf, false, s);
    if (dz_out) tr_dgrad(tr->dres, w->first_w, tr->Kf, PD_TR_FIRST_FIXED, dz_out, M, d, tr->z, nullptr, 0, false, s);
    if (grads->time_w0 || grads->time_b0 || grads->time_w2 || grads->time_b2) {
        tr_dgrad(tr->dres, w->first_w, tr->Kf, 189, tr->demb_t, M, d, 128, nullptr, 0, false, s);
        hipLaunchKernelGGL(pd_tr_tsum_kernel, dim3(B), dim3(128), 0, s, tr->demb_t, N, tr->dtemb);
        pd_tr_wgrad(tr->wk, tr->dtemb, tr->t_sact, grads->time_w2, grads->time_b2, B, 128, 128, false, s);
        if (grads->time_w0 || grads->time_b0) {
            tr_dgrad(tr->dtemb, w->time_w2, 128, 0, tr->dts, B, 128, 128, tr->t_a0, 2, false, s);
            pd_tr_wgrad(tr->wk, tr->dts, tr->t_emb256, grads->time_w0, grads->time_b0, B, 128, 256, false, s);
        }
    }
    PD_HIP_CHECK(hipGetLastError());
    return PD_OK;
}

extern "C" int pd_train_backward(pd_trainer *tr, const pd_weights *w, const float *g_loss, const pd_weight_grads *grads, float *dz_out,
                                 void *stream) {
    if (!tr || !g_loss || !grads) {
        pd_set_error("pd_train_backward: NULL trainer, g_loss or grads");
        return PD_ERR_INVALID_ARG;
    }
    return tr_backward(tr, w, g_loss, nullptr, nullptr, grads, dz_out, stream, "pd_train_backward");
}

extern "C" int pd_train_backward_ex(pd_trainer *tr, const pd_weights *w, const float *g_loss, const float *g_model_out, const float *g_x0_pred,
                                    const pd_weight_grads *grads, float *dz_out, void *stream) {
    if (!tr || !grads) {
        pd_set_error("pd_train_backward_ex: NULL trainer or grads");
        return PD_ERR_INVALID_ARG;
    }
    if (!g_loss && !g_model_out && !g_x0_pred) {
        pd_set_error("pd_train_backward_ex: g_loss, g_model_out and g_x0_pred are all NULL: at least one upstream gradient is needed");
        return PD_ERR_INVALID_ARG;
    }
    return tr_backward(tr, w, g_loss, g_model_out, g_x0_pred, grads, dz_out, stream, "pd_train_backward_ex");
}

extern "C" int pd_train_debug_relu(pd_trainer *tr, int layer, float *dst, long long n_floats, void *stream) {
    if (!tr || !dst || layer < 0 || layer > tr->layers) {
        pd_set_error("pd_train_debug_relu: NULL trainer / dst, or layer outside [0, num_layers]");
        return PD_ERR_INVALID_ARG;
    }
    if (tr->last_B < 1) {
        pd_set_error("pd_train_debug_relu: no forward has run on this trainer");
        return PD_ERR_STATE;
    }
    const long long M = (long long)tr->last_B * tr->last_N;
    const long long want = M * (layer < tr->layers ? tr->ff : tr->hid);
    if (n_floats != want) {
        pd_set_error("pd_train_debug_relu: n_floats=%lld, the last forward stashed %lld values there", n_floats, want);
        return PD_ERR_INVALID_ARG;
    }
    const float *src = layer < tr->layers ? tr->L[layer].ffa : tr->hid_post;
    PD_HIP_CHECK(hipMemcpyAsync(dst, src, (size_t)want * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return PD_OK;
}

extern "C" int pd_trainer_check_async(pd_trainer *tr) {
    if (!tr) {
        pd_set_error("pd_trainer_check_async: NULL trainer");
        return PD_ERR_INVALID_ARG;
    }
    unsigned int word = 0;
    PD_HIP_CHECK(hipDeviceSynchronize());
    PD_HIP_CHECK(hipMemcpy(&word, tr->d_err, sizeof(word), hipMemcpyDeviceToHost));
    if (!word) return PD_OK;
    PD_HIP_CHECK(hipMemset(tr->d_err, 0, sizeof(word)));
    pd_set_error("pd_trainer_check_async: a timestep outside [0, %d) was clamped by pd_train_forward (error word %u)", tr->timesteps, word);
    return PD_ERR_STATE;
}
