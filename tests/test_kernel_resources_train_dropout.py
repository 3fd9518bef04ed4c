"""Register / scratch budget of the dropout variants of the training branch's kernels (posediffusion_amd/csrc/pd_train_kernels.h), read
from hipcc's resource remarks like tests/test_kernel_resources_train.py (cross-compiled for gfx950, no GPU needed): the DROP = true
instantiations of the GEMM and of both attention kernels and the masked-copy kernel exist, carry the pd_tr_ prefix, neither spill nor
touch scratch (the Philox words are selected, never indexed at run time), and the GEMM variant keeps 4 workgroups' worth of waves per SIMD."""
import shutil

import pytest

from test_kernel_resources_train import _kernel_resources

# (substring of the mangled name): template <bool DROP> mangles as ILb1E / ILb0E
VARIANTS = ("pd_tr_gemm_kernelILb1E", "pd_tr_attn_kernelILb1E", "pd_tr_attn_bwd_kernelILb1E", "pd_tr_dropmask_kernel")
PLAIN = ("pd_tr_gemm_kernelILb0E", "pd_tr_attn_kernelILb0E", "pd_tr_attn_bwd_kernelILb0E")


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_dropout_variants_exist_and_do_not_spill_or_touch_scratch(tmp_path):
    kernels = _kernel_resources("pd_train.hip", tmp_path)
    for stem in VARIANTS + PLAIN:
        match = [k for k in kernels if stem in k]
        assert len(match) == 1, (stem, sorted(kernels))
        r = kernels[match[0]]
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (match[0], r)
    assert all("pd_tr_" in k for k in kernels), sorted(kernels)
    for stem in ("pd_tr_gemm_kernelILb1E", "pd_tr_gemm_kernelILb0E"):
        gemm = next(v for k, v in kernels.items() if stem in k)
        assert gemm["Occupancy"] >= 4 and gemm["LDS Size"] <= 20 * 1024, (stem, gemm)
    assert len([k for k in kernels if "pd_tr_colsum_kernel" in k]) == 2, sorted(kernels)
