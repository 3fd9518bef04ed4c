"""Register / scratch / LDS budget of pd_ggs_long_kernel (GGS for sequences of 65 .. 256 frames, csrc/pd_ggs_kernels.h) and of the kernels
beside it in pd_ggs.hip, read from hipcc's own resource remarks like tests/test_kernel_resources_long_attn.py does (cross-compiled for
gfx950, no GPU needed), and its LDS image (carve_long, csrc/pd_ggs_lds.h) run on the host.

The new kernel may not touch scratch or spill a vector register ("no spill" as tests/test_kernel_resources_ragged.py defines it for the GGS
kernels: their scalar spills land in lanes of a VGPR, never in memory).  The kernels that were there before must not move: the values below
are the PARENT commit's (b863ad7 "Sample sequences of different frame counts in one padded batch"), read from hipcc's remarks on that
tree with the flags of posediffusion_amd/csrc/Makefile:

    kernel                                   VGPRs  SGPRs  occupancy  scratch  LDS (static)
    pd_ggs2_kernel                            245    106       2         0        0
    pd_ggs_kernel<0, true, 8>                 197    106       2         0        0
    pd_ggs_kernel<0 / 3 / 5 / 6, false, 8>    166 / 148 / 158 / 164   106   3   0   0
    pd_ggs_kernel<3 / 5 / 6, false, 12>       150 / 154 / 158         106   3   0   0
    pd_ggs_lane_kernel<14>                    256    106       2         0        0
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "posediffusion_amd", "csrc")
FLAGS_GGS = ["-ffp-contract=on", "-fno-slp-vectorize"]            # the Makefile's flags of pd_ggs.o

# parent commit b863ad7: mangled-name fragment -> (VGPRs, TotalSGPRs, Occupancy, LDS Size)
PARENT = {
    "pd_ggs2_kernel": (245, 106, 2, 0),
    "pd_ggs_kernelILi0ELb1ELi8E": (197, 106, 2, 0),
    "pd_ggs_kernelILi0ELb0ELi8E": (166, 106, 3, 0),
    "pd_ggs_kernelILi3ELb0ELi8E": (148, 106, 3, 0),
    "pd_ggs_kernelILi5ELb0ELi8E": (158, 106, 3, 0),
    "pd_ggs_kernelILi6ELb0ELi8E": (164, 106, 3, 0),
    "pd_ggs_kernelILi3ELb0ELi12E": (150, 106, 3, 0),
    "pd_ggs_kernelILi5ELb0ELi12E": (154, 106, 3, 0),
    "pd_ggs_kernelILi6ELb0ELi12E": (158, 106, 3, 0),
    "pd_ggs_lane_kernelILi14E": (256, 106, 2, 0),
}


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_long_kernel_does_not_spill_and_the_other_ggs_kernels_keep_the_parents_resources(tmp_path):
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
    long_k = {k: v for k, v in kernels.items() if "pd_ggs_long_kernel" in k}
    assert len(long_k) == 1, sorted(kernels)
    for name, r in long_k.items():
        print(name, r)
        assert r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0, (name, r)
        assert r["VGPRs"] <= 256 and r["AGPRs"] == 0 and r["Occupancy"] >= 2, (name, r)      # 8 waves per workgroup: two per SIMD
        assert r["LDS Size"] == 0, (name, r)                                                    # all of its LDS is the dynamic image
    seen = set()
    for name, r in kernels.items():
        key = next((k for k in PARENT if k in name), None)
        if key is None:
            continue
        seen.add(key)
        assert (r["VGPRs"], r["TotalSGPRs"], r["Occupancy"], r["LDS Size"]) == PARENT[key], (name, r, PARENT[key])
        assert r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0, (name, r)
    assert seen == set(PARENT), seen ^ set(PARENT)


_LDS_PROGRAM = r"""
#include "pd_ggs_lds.h"
#include <stdio.h>
/* every table of the image, in carve order, with the extent (floats) the kernel indexes: each must end where the next begins or before */
static int tables_inside(int n_slots, int n_batch) {
    const LdsLong L = carve_long(pd_ggs_lds_origin(), n_slots, n_batch);
    struct T { const void *p; size_t floats; };
    const T t[] = {
        {L.Rc, (size_t)PD_GGS_LONG_FRAMES * PD_FR_STRIDE}, {L.fl, (size_t)PD_GGS_LONG_FRAMES * 4}, {L.cam, 8},
        {L.gT, (size_t)PD_GGS_LONG_FRAMES * 3}, {L.gR, (size_t)PD_GGS_LONG_FRAMES * 9}, {L.gA, (size_t)PD_GGS_LONG_FRAMES * 4}, {L.ctl, 8},
        {L.red, 32}, {L.xst, (size_t)PD_GGS_LONG_FRAMES * PD_XS_STRIDE}, {L.mst, (size_t)PD_GGS_LONG_FRAMES * PD_XS_STRIDE},
        {L.psum, (size_t)PD_GGS_LONG_FRAMES * 16},            /* the gathered frame sums of 256 frames */
        {L.incoff, 260},                                       /* N + 1 = 257 CSR offsets */
        {L.tot_rows, 256 * 4},                                 /* totals of k = 256 workgroups */
        {L.frame_rows, (size_t)2 * (PD_GGS_LONG_FRAMES - 1) * 16},   /* 510 incidence rows of a frame, both orders of every pair */
        {L.own_rows, (size_t)2 * n_batch * 16}, {L.F, (size_t)n_batch * PD_F_STRIDE}, {L.item, (size_t)n_batch * PD_ITEM_VALS},
        {L.itab, (size_t)n_slots * 4}, {L.grow, (size_t)n_slots * 2}, {L.end, 0}};
    const int n = (int)(sizeof(t) / sizeof(t[0]));
    for (int i = 0; i + 1 < n; ++i)
        if ((const char *)t[i].p + 4 * t[i].floats > (const char *)t[i + 1].p) return i + 1;
    if (L.pinc != L.own_rows || pd_ggs_lds_offset(L.Rc) != 0) return 100;
    if (pd_ggs_lds_offset(L.itab) % 16 || pd_ggs_lds_offset(L.own_rows) % 16 || pd_ggs_lds_offset(L.F) % 16 || pd_ggs_lds_offset(L.xst) % 16 ||
        pd_ggs_lds_offset(L.fl) % 16 || pd_ggs_lds_offset(L.mst) % 16) return 101;       /* the float4 / int4 accesses */
    return 0;
}
int main() {
    size_t worst = 0, prev = 0;
    int max_single = 0, max_slots = 0;
    for (int s = 8; s <= 4096; s += 8) {
        const int nb = ggs_long_batch(s);
        if (nb <= 0) break;                                   /* what pd_ggs_plan refuses */
        max_slots = s;
        if (nb == s) max_single = s;
        if (nb > s || nb > PD_GGS_THREADS || (nb < s && nb % 64)) return 3;
        const size_t b = ggs_long_lds_bytes(s, nb);
        if (b > worst) worst = b;
        const int rc = tables_inside(s, nb);
        if (rc) return 10 + rc;
        /* monotonic in the slot count at a fixed batch, and in the batch at a fixed slot count */
        if (s > 8 && nb == s && b <= prev) return 4;
        if (nb == s) prev = b;
        if (ggs_long_lds_bytes(s + 8, nb) <= b) return 5;
        if (nb >= 8 && ggs_long_lds_bytes(s, nb - 8) >= b) return 6;
    }
    /* capacity the plan must accept on a 256-CU chip: B = 1, 32 640 pairs on 256 workgroups (128 slots); B = 2 at 129 frames (72 slots);
       and 2 080 pairs on 3 workgroups (696 slots, in batches) */
    printf("%zu %d %d %d %d %d\n", worst, max_single, max_slots, ggs_long_batch(128), ggs_long_batch(72), ggs_long_batch(696));
    return 0;
}
"""


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_long_kernel_lds_image_fits_a_cu_and_holds_every_window(tmp_path):
    src, exe = tmp_path / "lds.cpp", tmp_path / "lds"
    src.write_text(_LDS_PROGRAM)
    out = subprocess.run(["hipcc", "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    worst, max_single, max_slots, b128, b72, b696 = (int(v) for v in run.stdout.split())
    print(run.stdout)
    assert worst <= 160 * 1024, worst                       # LDS of a CU, at the largest slot count the plan admits
    assert max_single >= 128 and b128 == 128 and b72 == 72  # the two capacity cases run as one batch
    assert b696 >= 64 and b696 % 64 == 0                    # 65 frames on 3 workgroups: several batches
    assert max_slots >= 696
