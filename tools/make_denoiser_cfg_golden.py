"""Generate tests/golden/denoiser_cfgs.npz by executing the UNMODIFIED reference models/denoiser.py on CPU (build container only).

    python tools/make_denoiser_cfg_golden.py            # needs the reference checkout

The recipe is tests/denoiser_cfgs.py make_golden(): the test-side code that may load the reference (the product and tools/ never do,
tests/test_host_cpu.py).  For every configuration of GOLDEN_CFGS there (post-norm, no pivot, odd sizes) the reference's own Denoiser
is built with the drop-in's seed protocol and its forward recorded at two timesteps; weights are not stored, only a checksum:
tests/test_gpu_denoiser_cfgs.py rebuilds them from the seed through the drop-in Denoiser.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from denoiser_cfgs import make_golden  # noqa: E402

if __name__ == "__main__":
    make_golden(os.path.join(ROOT, "tests", "golden", "denoiser_cfgs.npz"))
