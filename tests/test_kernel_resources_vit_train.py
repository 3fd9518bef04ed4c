"""Register / scratch budget of the backbone trainer's kernels (posediffusion_amd/csrc/pd_vit_train.hip, include/pd_engine_vit_train.h),
read from hipcc's own resource remarks like tests/test_kernel_resources_train.py does (cross-compiled for gfx950, no GPU needed): nothing
in the new translation unit may spill or touch scratch, every kernel the launch list of DESIGN 3.10 names is there, and every kernel is
either the denoiser trainer's (pd_tr_*) or the unit's own (pd_vt_*)."""
import shutil

import pytest

from test_kernel_resources_train import _kernel_resources

SHARED = ("pd_tr_gemm_kernel", "pd_tr_reduce_kernel", "pd_tr_colsum_kernel", "pd_tr_ln_bwd_kernel", "pd_tr_lattn_kernel",
          "pd_tr_lattn_bwd_rows_kernel", "pd_tr_lattn_bwd_keys_kernel")
OWN = ("pd_vt_im2col_kernel", "pd_vt_assemble_kernel", "pd_vt_assemble_bwd_kernel", "pd_vt_ln_kernel", "pd_vt_gelu_kernel",
       "pd_vt_gelu_bwd_kernel", "pd_vt_final_kernel", "pd_vt_final_bwd_kernel", "pd_vt_final_param_kernel", "pd_vt_reduce_acc_kernel",
       "pd_vt_posgrid_kernel")


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_backbone_training_kernels_do_not_spill_or_touch_scratch(tmp_path):
    kernels = _kernel_resources("pd_vit_train.hip", tmp_path)
    for stem in SHARED + OWN:
        assert [k for k in kernels if stem in k], (stem, sorted(kernels))
    assert all("pd_tr_" in k or "pd_vt_" in k for k in kernels), sorted(kernels)                # nothing instantiated from other headers
    assert len([k for k in kernels if "pd_vt_reduce_acc_kernel" in k]) == 2, sorted(kernels)     # weight-gradient and column-sum partials
    for name, r in kernels.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (name, r)
    for stem in OWN:                                                                             # memory-bound row / element kernels: full occupancy
        assert all(r["Occupancy"] == 8 for k, r in kernels.items() if stem in k), stem
    pos = next(v for k, v in kernels.items() if "pd_vt_posgrid_kernel" in k)
    assert pos["LDS Size"] == 4 * 4 * 256 * 4, pos                                               # the tap tables of both axes
