"""Register / scratch budget of every kernel that frame counts per sequence (pd_engine_set_frame_counts) touch, read from hipcc's own
resource remarks like tests/test_kernel_resources_long_attn.py does (cross-compiled for gfx950, no GPU needed).

Touched: the three GGS kernels (they take a sequence's frame count from its descriptor and only the row stride of x from PdGgsParams::N),
the key-tiled attention kernels (a length per sequence), the two tails and pd_finish_kernel (padding rows get +0); new: pd_set_counts_kernel
and pd_zero_padding_kernel.  None may use scratch or spill a vector register.  The uniform path must not get dearer: the values below are
the PARENT commit's (8765e58 "Denoiser and unguided sampling up to 256 frames: key-tiled attention"), read from hipcc's remarks on that tree
with the flags of posediffusion_amd/csrc/Makefile:

    kernel                              VGPRs  occupancy  scratch  SGPR spills (into VGPR lanes, no scratch)
    pd_ggs_lane_kernel<14>               256       2         0       154
    pd_ggs_kernel<0, true, 8>            197       2         0       101
    pd_ggs_kernel<0 / 3 / 5 / 6, false, 8>  166 / 148 / 158 / 164   3   0   122 / 123 / 123 / 123
    pd_ggs_kernel<3 / 5 / 6, false, 12>  150 / 154 / 158   3   0   111 each
    pd_ggs2_kernel                       245       2         0        96
    pd_attn_long_kernel<0 / 1 / 2>       110       4         0         0
    pd_gen_attn_long_kernel<0>           116       4         0         0

The GGS kernels' SGPR spills predate this change (the scalar file is 106 registers wide and the kernels hold a descriptor, the parameter
block and the launch geometry): they land in lanes of a VGPR, never in memory, which is why "no spill" is asserted here as no VECTOR spill
and no scratch.  The lane kernel sits AT the 256-VGPR limit: one more live value would spill, so its VGPRs, scratch and occupancy are pinned
to the parent's."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "posediffusion_amd", "csrc")
FLAGS_DEFAULT = ["-ffp-contract=fast"]
FLAGS_GGS = ["-ffp-contract=on", "-fno-slp-vectorize"]            # the Makefile's flags of pd_ggs.o

# parent commit 8765e58 (see the table above)
PARENT_LANE = {"VGPRs": 256, "Occupancy": 2, "ScratchSize": 0}
PARENT_GGS_OCCUPANCY = {"pd_ggs2_kernel": 2, "ILi0ELb1ELi8E": 2, "ILi0ELb0ELi8E": 3, "ILi3ELb0ELi8E": 3, "ILi5ELb0ELi8E": 3, "ILi6ELb0ELi8E": 3,
                        "ILi3ELb0ELi12E": 3, "ILi5ELb0ELi12E": 3, "ILi6ELb0ELi12E": 3}
PARENT_LONG_ATTN_OCCUPANCY = 4          # pd_attn_long_kernel<0 / 1 / 2> and pd_gen_attn_long_kernel<0>

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")


def _kernel_resources(src, flags, tmp_path):
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", *flags, "-Rpass-analysis=kernel-resource-usage",
                          "-c", os.path.join(CSRC, src), "-o", str(tmp_path / (src + ".o"))], capture_output=True, text=True, timeout=1500)
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


def _no_vector_spill_no_scratch(name, r):
    assert r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0, (name, r)


def _no_spill(name, r):
    _no_vector_spill_no_scratch(name, r)
    assert r["SGPRs Spill"] == 0, (name, r)


def test_ggs_kernels_keep_the_parents_registers_and_occupancy(tmp_path):
    kernels = _kernel_resources("pd_ggs.hip", FLAGS_GGS, tmp_path)
    lane = {k: v for k, v in kernels.items() if "pd_ggs_lane_kernel" in k}
    assert len(lane) == 1, sorted(kernels)
    for name, r in lane.items():
        _no_vector_spill_no_scratch(name, r)
        assert {k: r[k] for k in PARENT_LANE} == PARENT_LANE, (name, r)
    seen = set()
    for name, r in kernels.items():
        if "pd_ggs_kernel" not in name and "pd_ggs2_kernel" not in name:
            continue
        _no_vector_spill_no_scratch(name, r)
        key = next(k for k in PARENT_GGS_OCCUPANCY if k in name)
        seen.add(key)
        assert r["Occupancy"] == PARENT_GGS_OCCUPANCY[key], (name, r)
        assert r["VGPRs"] <= 256 and r["AGPRs"] == 0, (name, r)
        print(name, {k: r[k] for k in ("VGPRs", "Occupancy", "SGPRs Spill")})
    assert seen == set(PARENT_GGS_OCCUPANCY), seen ^ set(PARENT_GGS_OCCUPANCY)      # every variant of the one variant table was looked at


def test_default_shape_attention_tail_keep_their_budget(tmp_path):
    kernels = _kernel_resources("pd_denoiser.hip", FLAGS_DEFAULT, tmp_path)
    long_k = {k: v for k, v in kernels.items() if "pd_attn_long_kernel" in k}
    assert sorted(re.search(r"ILi(\d)E", k).group(1) for k in long_k) == ["0", "1", "2"], sorted(kernels)
    for name, r in long_k.items():
        _no_spill(name, r)
        assert r["Occupancy"] >= 2 and r["Occupancy"] == PARENT_LONG_ATTN_OCCUPANCY, (name, r)
    tails = {k: v for k, v in kernels.items() if "pd_tail_kernel" in k or "pd_tail_t_kernel" in k}
    assert len(tails) == 2, sorted(kernels)
    for name, r in tails.items():
        _no_spill(name, r)
        assert r["Occupancy"] == 8, (name, r)


def test_generic_attention_and_tail_keep_their_budget(tmp_path):
    kernels = _kernel_resources("pd_denoiser_generic.hip", FLAGS_DEFAULT, tmp_path)
    gen = {k: v for k, v in kernels.items() if "pd_gen_attn_long_kernel" in k}
    assert len(gen) == 1, sorted(kernels)
    for name, r in gen.items():
        _no_spill(name, r)
        assert r["Occupancy"] >= 2 and r["Occupancy"] == PARENT_LONG_ATTN_OCCUPANCY, (name, r)
    tails = {k: v for k, v in kernels.items() if "pd_gen_tail_kernel" in k}
    assert len(tails) == 2, sorted(kernels)
    for name, r in tails.items():
        _no_spill(name, r)


def test_engine_side_kernels_do_not_spill(tmp_path):
    kernels = _kernel_resources("pd_engine.hip", FLAGS_DEFAULT, tmp_path)
    for want in ("pd_finish_kernel", "pd_set_counts_kernel", "pd_zero_padding_kernel"):
        found = {k: v for k, v in kernels.items() if want in k}
        assert len(found) == 1, (want, sorted(kernels))
        for name, r in found.items():
            _no_spill(name, r)
            assert r["Occupancy"] == 8 and r["LDS Size"] == 0, (name, r)
