"""Register / scratch / LDS budget of the key-tiled attention kernels for sequences of more than 64 frames (pd_attn_long.h), read from
hipcc's own resource remarks like tests/test_kernel_resources_tseq.py does (cross-compiled for gfx950, no GPU needed).

The new instantiations are pd_attn_long_kernel<0 / 1 / 2> in pd_denoiser.hip (fp32, bf16 split words, fp16 split words) and
pd_gen_attn_long_kernel<0> in pd_denoiser_generic.hip.  None may touch scratch or spill; the default-shape kernel must leave room for two
workgroups per CU in registers (>= 2 waves per SIMD) and in LDS (<= 80 KB); no shape of the family may ask for more LDS than a CU has."""
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
def test_default_shape_long_attention_kernels_keep_their_budget(tmp_path):
    kernels = _kernel_resources("pd_denoiser.hip", tmp_path)
    long_k = {k: v for k, v in kernels.items() if "pd_attn_long_kernel" in k}
    assert sorted(re.search(r"ILi(\d)E", k).group(1) for k in long_k) == ["0", "1", "2"], sorted(kernels)      # SPLIT_OUT 0, 1, 2
    for name, r in long_k.items():
        _no_spill(name, r)
        assert r["Occupancy"] >= 2, (name, r)               # two workgroups of 4 waves per CU
    assert not [k for k in kernels if "pd_gen_attn_long_kernel" in k], sorted(kernels)      # the generic twin lives in its own file


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_generic_long_attention_kernel_does_not_spill(tmp_path):
    kernels = _kernel_resources("pd_denoiser_generic.hip", tmp_path)
    gen = {k: v for k, v in kernels.items() if "pd_gen_attn_long_kernel" in k}
    assert len(gen) == 1, sorted(kernels)
    for name, r in gen.items():
        _no_spill(name, r)
    assert not [k for k in kernels if "pd_attn_long_kernel" in k], sorted(kernels)


_LDS_PROGRAM = r"""
#define PD_ATTN_LONG_HOST_ONLY
#include "pd_attn_long.h"
#include <stdio.h>
int main() {
    size_t worst = 0, worst_default = 0;
    for (int N = 1; N <= 256; ++N)
        for (int hd = 8; hd <= 256; hd += 4) {
            const size_t b = pd_attn_long_lds(N, hd);
            if (b > worst) worst = b;
            if (hd == 128 && b > worst_default) worst_default = b;
            if (N > 1 && b < pd_attn_long_lds(N - 1, hd)) return 2;      /* monotonic in N: the size registered at creation (N = 256) covers every launch */
        }
    printf("%zu %zu %d %d\n", worst, worst_default, PD_ATTN_LONG_TILE * PD_ATTN_LONG_MAX_TILES, PD_ATTN_LONG_ROWS);
    return 0;
}
"""


@pytest.mark.skipif(shutil.which("g++") is None and shutil.which("hipcc") is None, reason="no host C++ compiler")
def test_long_attention_lds_size_fits_a_cu_for_the_whole_family(tmp_path):
    """pd_attn_long_lds(N, hd) on the host, for every N <= 256 and every head dim of the family (a multiple of 4 in [8, 256])."""
    src, exe = tmp_path / "lds.cpp", tmp_path / "lds"
    src.write_text(_LDS_PROGRAM)
    cxx = "g++" if shutil.which("g++") else "hipcc"
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    worst, worst_default, max_frames, rows = (int(v) for v in run.stdout.split())
    assert worst <= 160 * 1024, worst                       # LDS of a CU
    assert worst_default <= 80 * 1024, worst_default        # the default head: two workgroups per CU
    assert max_frames == 256 and rows == 20
