"""Register / scratch / LDS budget of pd_ggs_longm_kernel (PD_OPT_GGS_LONG_PAIR_ITEMS: GGS above 64 frames with frame pairs of several
work items, csrc/pd_ggs_kernels.h), read from hipcc's own resource remarks like tests/test_kernel_resources_ggs_long.py does
(cross-compiled for gfx950, no GPU needed).

The new kernel is held to what pd_ggs_long_kernel is held to: <= 256 VGPRs, no AGPRs, no vector spill, no scratch, two waves per SIMD, no
static LDS.  The kernels beside it must not move: pd_ggs_long_kernel's figures below are the PARENT commit's (e93b9f2 "Device-side match
ingestion per sequence frame count, up to 256 frames"), read from hipcc's remarks on that tree with the flags of
posediffusion_amd/csrc/Makefile -- 256 VGPRs, 106 SGPRs, occupancy 2, static LDS 0 --; the others are the PARENT table of
tests/test_kernel_resources_ggs_long.py, which that commit's tree also gives.
"""
import os
import re
import shutil
import subprocess

import pytest

from test_kernel_resources_ggs_long import CSRC, FLAGS_GGS, PARENT

NEW = "pd_ggs_longm_kernel"
LONG_PARENT = (256, 106, 2, 0)              # pd_ggs_long_kernel on the parent commit: (VGPRs, TotalSGPRs, Occupancy, LDS Size)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_pair_items_kernel_meets_the_budget_and_the_kernels_beside_it_keep_the_parents_resources(tmp_path):
    assert "pd_ggs_long_kernel" not in NEW and not any(k in NEW or NEW in k for k in PARENT)      # the names the other file selects by
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", *FLAGS_GGS, "-Rpass-analysis=kernel-resource-usage",
                          "-c", os.path.join(CSRC, "pd_ggs.hip"), "-o", str(tmp_path / "pd_ggs.o")], capture_output=True, text=True, timeout=1500)
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
    new_k = {k: v for k, v in kernels.items() if NEW in k}
    assert len(new_k) == 1, sorted(kernels)
    for name, r in new_k.items():
        print(name, r)
        assert r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0, (name, r)
        assert r["VGPRs"] <= 256 and r["AGPRs"] == 0 and r["Occupancy"] >= 2, (name, r)
        assert r["LDS Size"] == 0, (name, r)
    long_k = {k: v for k, v in kernels.items() if "pd_ggs_long_kernel" in k}
    assert len(long_k) == 1, sorted(kernels)
    seen = set()
    for name, r in kernels.items():
        key = next((k for k in PARENT if k in name), None)
        want = PARENT[key] if key else LONG_PARENT if name in long_k else None
        if want is None:
            continue
        seen.add(key or "pd_ggs_long_kernel")
        assert (r["VGPRs"], r["TotalSGPRs"], r["Occupancy"], r["LDS Size"]) == want, (name, r, want)
        assert r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0 and r["AGPRs"] == 0, (name, r)
    assert seen == set(PARENT) | {"pd_ggs_long_kernel"}, seen
