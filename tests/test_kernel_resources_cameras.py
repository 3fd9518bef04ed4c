"""Register / scratch budget of the camera-normalisation kernel (posediffusion_amd/csrc/pd_cameras.hip, include/pd_engine_cameras.h), read
from hipcc's own resource remarks like tests/test_kernel_resources_train.py does (cross-compiled for gfx950, no GPU needed): the one
kernel of the translation unit, all fp64, neither spills nor touches scratch, and its LDS is the few hundred bytes of one sequence's
partial sums and broadcast values."""
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


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_camera_kernel_does_not_spill_or_touch_scratch(tmp_path):
    kernels = _kernel_resources("pd_cameras.hip", tmp_path)
    assert len(kernels) == 1 and "pd_normalize_cameras_kernel" in next(iter(kernels)), sorted(kernels)
    r = next(iter(kernels.values()))
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, r
    assert r["LDS Size"] <= 1024, r
    with open(os.path.join(CSRC, "Makefile")) as fh:
        mk = fh.read()
    assert "build/pd_cameras.o" in mk and "pd_engine_cameras.h" in mk
