"""Register / scratch budget of the kernels that serve one timestep per sequence (pd_denoise_step_t, pd_p_losses), read from hipcc's own
resource remarks like tests/test_kernel_resources.py does for the single-t kernels (cross-compiled for gfx950, no GPU needed).

The new instantiations are the per-row-bias `_first` GEMM of the streamed path (pd_gemm_dma_kernel EPI 5, pd_denoiser_first_t.hip), the
small-batch `_first` GEMM whose A staging picks the time-table row of its token row (pd_gemm_kernel AMODE 3, both tile widths), the tail
with per-row schedule coefficients (pd_tail_t_kernel) and the generic path's two TSEQ variants.  None of them may touch scratch, and
the new GEMMs must keep the occupancy of the single-t kernels they stand in for (EPI 4: >= 5 waves per SIMD)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "posediffusion_amd", "csrc")


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


def _no_spill(name, r):
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (name, r)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_streamed_first_gemm_with_per_row_bias_keeps_its_budget(tmp_path):
    kernels = _kernel_resources("pd_denoiser_first_t.hip", tmp_path)
    dma = {k: v for k, v in kernels.items() if "pd_gemm_dma_kernel" in k}
    assert len(dma) == 1 and "ILi5E" in next(iter(dma)), sorted(kernels)        # this file instantiates EPI 5 and nothing else
    for name, r in dma.items():
        _no_spill(name, r)
        assert r["Occupancy"] >= 5, (name, r)                                   # the bound of EPI 4, the single-t launch it replaces


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_default_path_tseq_kernels_do_not_spill(tmp_path):
    kernels = _kernel_resources("pd_denoiser.hip", tmp_path)
    first = {k: v for k, v in kernels.items() if "pd_gemm_kernel" in k and "ILi704ELi3ELi0E" in k}
    assert len(first) == 2, sorted(kernels)                                     # 32- and 16-wide tiles
    single = {k: v for k, v in kernels.items() if "pd_gemm_kernel" in k and "ILi704ELi2ELi0E" in k}
    assert len(single) == 2, sorted(kernels)
    for name, r in first.items():
        _no_spill(name, r)
        twin = single[name.replace("ILi704ELi3ELi0E", "ILi704ELi2ELi0E")]
        assert r["Occupancy"] >= twin["Occupancy"], (name, r, twin)             # no fewer waves per SIMD than the single-t staging
    tail = {k: v for k, v in kernels.items() if "pd_tail_t_kernel" in k}
    assert len(tail) == 1, sorted(kernels)
    pre = {k: v for k, v in kernels.items() if "pd_q_sample_kernel" in k or "pd_t_rows_kernel" in k}
    assert len(pre) == 2, sorted(kernels)
    for name, r in {**tail, **pre}.items():
        _no_spill(name, r)
    # the single-t streamed path keeps exactly its five LDS-DMA GEMMs in this file: EPI 5 lives in pd_denoiser_first_t.hip
    assert not [k for k in kernels if "pd_gemm_dma_kernel" in k and "ILi5E" in k], sorted(kernels)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_generic_path_tseq_kernels_do_not_spill(tmp_path):
    kernels = _kernel_resources("pd_denoiser_generic.hip", tmp_path)
    for stem in ("pd_gen_embed_kernel", "pd_gen_tail_kernel"):
        both = {k: v for k, v in kernels.items() if stem in k}
        assert len(both) == 2, (stem, sorted(kernels))                          # <false> (single t) and <true> (per sequence)
        for name, r in both.items():
            _no_spill(name, r)
