"""Register / scratch budget of the backbone trainer's kernels (posediffusion_amd/csrc/pd_vit_train.hip, include/pd_engine_vit_train.h),
read from hipcc's own resource remarks like tests/test_kernel_resources_train.py does (cross-compiled for gfx950, no GPU needed): nothing
in the translation unit may spill or touch scratch, every kernel the launch list of DESIGN 3.10 names is there -- the unit's own
(pd_vt_*) in pd_vit_train.hip, which holds no second copy of a pd_tr_* kernel, and the shared ones (pd_tr_*) in pd_train.hip alone."""
import shutil

import pytest

from test_kernel_resources_train import _kernel_resources

SHARED = ("pd_tr_gemm_kernel", "pd_tr_reduce_kernel", "pd_tr_colsum_kernel", "pd_tr_ln_kernel", "pd_tr_ln_bwd_kernel", "pd_tr_lattn_kernel",
          "pd_tr_lattn_bwd_rows_kernel", "pd_tr_lattn_bwd_keys_kernel")
OWN = ("pd_vt_im2col_kernel", "pd_vt_assemble_kernel", "pd_vt_assemble_bwd_kernel", "pd_vt_gelu_kernel", "pd_vt_gelu_bwd_kernel",
       "pd_vt_final_kernel", "pd_vt_final_bwd_kernel", "pd_vt_final_param_kernel", "pd_vt_posgrid_kernel")


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_backbone_training_kernels_do_not_spill_or_touch_scratch(tmp_path):
    kernels = _kernel_resources("pd_vit_train.hip", tmp_path)
    for stem in OWN:
        assert [k for k in kernels if stem in k], (stem, sorted(kernels))
    assert all("pd_vt_" in k for k in kernels), sorted(kernels)                                  # nothing instantiated from other headers
    assert not [k for k in kernels if "pd_tr_" in k], sorted(kernels)                            # no second copy of a shared kernel
    for name, r in kernels.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (name, r)
    for stem in OWN:                                                                             # memory-bound row / element kernels: full occupancy
        assert all(r["Occupancy"] == 8 for k, r in kernels.items() if stem in k), stem
    pos = next(v for k, v in kernels.items() if "pd_vt_posgrid_kernel" in k)
    assert pos["LDS Size"] == 4 * 4 * 256 * 4, pos                                               # the tap tables of both axes


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_shared_kernels_of_the_backbone_trainer_live_in_the_denoiser_trainers_unit(tmp_path):
    kernels = _kernel_resources("pd_train.hip", tmp_path)
    for stem in SHARED:
        mine = {k: r for k, r in kernels.items() if stem in k}
        assert mine, (stem, sorted(kernels))
        for name, r in mine.items():
            assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (name, r)
    # float (weight-gradient partials) and double (column-sum partials), each writing (the denoiser, a call's first scale) and adding (later scales)
    assert len([k for k in kernels if "pd_tr_reduce_kernel" in k]) == 4, sorted(kernels)
    assert all(r["Occupancy"] == 8 for k, r in kernels.items() if "pd_tr_ln_kernel" in k)        # the forward LayerNorm of both trainers
