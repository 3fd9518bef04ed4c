"""Register / scratch budget of the image feature extractor's strip GEMM instances, read from hipcc's own resource remarks (cross-compiled for
gfx950, no GPU needed), as tests/test_kernel_resources.py does for the denoiser: pd_vit.hip instantiates pd_gemm_strip_kernel with its own
epilogues (GELU among them), and nothing of them may spill or touch scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_vit_strip_kernels_do_not_spill(tmp_path):
    src = os.path.join(ROOT, "posediffusion_amd", "csrc", "pd_vit.hip")
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-Rpass-analysis=kernel-resource-usage",
                          "-c", src, "-o", str(tmp_path / "pd_vit.o")], capture_output=True, text=True, timeout=900)
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
    strip = {k: v for k, v in kernels.items() if "pd_gemm_strip_kernel" in k}
    assert len(strip) == 3, sorted(kernels)                     # qkv (EPI 0), proj / fc2 (EPI 2), fc1 (EPI 3: GELU), 64-row tiles, fp16 planes, 64-k form
    pairs = {name: re.search(r"pd_gemm_strip_kernelILi(\d+)ELi(\d+)EEv", name) for name in strip}       # <EPI, RT> and nothing else
    assert all(pairs.values()), sorted(strip)
    assert {(int(m.group(1)), int(m.group(2))) for m in pairs.values()} == {(0, 2), (2, 2), (3, 2)}, sorted(strip)
    for name, r in strip.items():
        assert r["VGPRs Spill"] == 0 and r.get("SGPRs Spill", 0) == 0 and r["ScratchSize"] == 0, (name, r)
        # one wave per SIMD less for the instance that holds the residual tile, as in the denoiser
        assert r["Occupancy"] >= (3 if "kernelILi2E" in name else 4), (name, r)
