"""Register / scratch budget of the training branch's kernels (posediffusion_amd/csrc/pd_train.hip, include/pd_engine_train.h), read from
hipcc's own resource remarks like tests/test_kernel_resources_tseq.py does (cross-compiled for gfx950, no GPU needed): nothing in the new
translation unit may spill or touch scratch, and every kernel the launch list of DESIGN 3.9 names is there."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "posediffusion_amd", "csrc")
KERNELS = ("pd_tr_gemm_kernel", "pd_tr_reduce_kernel", "pd_tr_colsum_kernel", "pd_tr_q_sample_kernel", "pd_tr_time_kernel",
           "pd_tr_embed_kernel", "pd_tr_ln_kernel", "pd_tr_ln_bwd_kernel", "pd_tr_attn_kernel", "pd_tr_attn_bwd_kernel",
           "pd_tr_tail_kernel", "pd_tr_tail_bwd_kernel", "pd_tr_tsum_kernel")


def _kernel_resources(src, tmp_path):
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-Rpass-analysis=kernel-resource-usage",
                          "-c", os.path.join(CSRC, src), "-o", str(tmp_path / (src + ".o"))], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+?): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split("[")[0].strip()] = int(m.group(2))
    return kernels


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_training_kernels_do_not_spill_or_touch_scratch(tmp_path):
    kernels = _kernel_resources("pd_train.hip", tmp_path)
    for stem in KERNELS:
        assert [k for k in kernels if stem in k], (stem, sorted(kernels))
    assert len([k for k in kernels if "pd_tr_colsum_kernel" in k]) == 2, sorted(kernels)       # bias sums and LayerNorm's dgamma / dbeta
    assert all("pd_tr_" in k for k in kernels), sorted(kernels)                                 # nothing instantiated from other headers
    for name, r in kernels.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (name, r)
    gemm = next(v for k, v in kernels.items() if "pd_tr_gemm_kernel" in k)
    assert gemm["Occupancy"] >= 4 and gemm["LDS Size"] <= 20 * 1024, gemm                       # several workgroups per CU hide the staging
