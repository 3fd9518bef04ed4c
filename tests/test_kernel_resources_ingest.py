"""Register / scratch / LDS budget of the match ingestion kernels (csrc/pd_ggs_ingest.hip), read from hipcc's own resource remarks like
tests/test_kernel_resources_ggs_long.py does (cross-compiled for gfx950, no GPU needed).

The kernels of sequences above 64 frames (ingest_nf_*, pd_ggs_set_matches_csr_async_nf) may not touch scratch or spill a vector register,
and keep their tables out of LDS: static LDS only, far below 64 KiB (no table of N^2 entries).  The kernels pd_ggs_set_matches_csr_async
launches must not move: the values below are the PARENT commit's (6ba4b2c "Test GGS on non-square images and outside the clipped-step
regime"), read from hipcc's remarks on that tree with the flags of posediffusion_amd/csrc/Makefile:

    kernel                      VGPRs  SGPRs  occupancy  scratch  LDS (static)
    ingest_hist_kernel            50     58       8         0        0
    ingest_tables_kernel          67    106       7         0        0
    ingest_scatter_kernel         64     52       8         0        0
    ingest_lane_stream_kernel     18     22       8         0        0
    ingest_interleave_kernel      37     18       8         0        0
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "posediffusion_amd", "csrc")

# parent commit 6ba4b2c: kernel -> (VGPRs, TotalSGPRs, Occupancy, LDS Size)
PARENT = {
    "ingest_hist_kernel": (50, 58, 8, 0),
    "ingest_tables_kernel": (67, 106, 7, 0),
    "ingest_scatter_kernel": (64, 52, 8, 0),
    "ingest_lane_stream_kernel": (18, 22, 8, 0),
    "ingest_interleave_kernel": (37, 18, 8, 0),
}
NEW = ("ingest_nf_zero_kernel", "ingest_nf_keys_kernel", "ingest_nf_hist2_kernel", "ingest_nf_prefix_kernel", "ingest_nf_scatter_kernelILi0E",
       "ingest_nf_scatter_kernelILi1E", "ingest_nf_tables_kernel")


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_new_ingest_kernels_do_not_spill_and_the_old_ones_keep_the_parents_resources(tmp_path):
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-Rpass-analysis=kernel-resource-usage",
                          "-c", os.path.join(CSRC, "pd_ggs_ingest.hip"), "-o", str(tmp_path / "pd_ggs_ingest.o")],
                         capture_output=True, text=True, timeout=900)
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

    def named(fragment):                                     # (mangled: the length prefix keeps `ingest_tables_kernel` apart from `ingest_nf_...`)
        hit = [k for k in kernels if re.search(r"\d" + fragment + r"(\d|E|$)", k)]
        assert len(hit) == 1, (fragment, sorted(kernels))
        return hit[0]

    for frag in NEW:
        name = named(frag)
        r = kernels[name]
        print(name, r)
        assert r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0, (name, r)
        assert r["LDS Size"] <= 64 * 1024, (name, r)
        assert r["LDS Size"] <= 8 * 1024, (name, r)              # digit counters and per-frame tables only: nothing of N^2 entries
    for frag, want in PARENT.items():
        name = named(frag)
        r = kernels[name]
        assert (r["VGPRs"], r["TotalSGPRs"], r["Occupancy"], r["LDS Size"]) == want, (name, r, want)
        assert r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0, (name, r)
    assert len(kernels) == len(NEW) + len(PARENT), sorted(kernels)
