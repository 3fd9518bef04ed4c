// pd_denoiser_first_t.hip -- the streamed denoiser path's `_first` GEMM when every sequence has a timestep of its own
// (pd_denoise_step_t, pd_p_losses; models/gaussian_diffuser.py:331 draws one t per sequence).
//
// h = zproj + ttab[t_row[m]] + D W_d^T: the launch of den_first_streamed (pd_denoiser.hip) with the time piece looked up per ROW in the
// epilogue (pd_gemm_dma EPI 5) instead of passed as the bias vector of one t -- the same K = 192 MFMA chain and the same two fp32
// additions in the same order, so a t_seq whose entries are all equal gives bitwise the result of the single-t launch.
//
// A translation unit of its own: pd_denoiser.hip holds exactly the GEMM instantiations the single-t sampling path launches, and its
// register budget is checked kernel by kernel (tests/test_kernel_resources.py); this one is checked by tests/test_kernel_resources_tseq.py.
#include "pd_denoiser_dev.h"
#include "pd_gemm_stream.h"

void pd_den_first_gemm_t(const PdDenoiserDev *d, const int *t_row, int M, hipStream_t s) {
    pd_gemm_dma<5>(d->emb, KFIRST_D, d->first_df, KFIRST_D, d->ttab, d->h, M, DM, s, nullptr, d->zproj, t_row);
}
