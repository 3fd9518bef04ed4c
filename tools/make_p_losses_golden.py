"""Generate tests/golden/p_losses.npz by executing the UNMODIFIED reference models/gaussian_diffuser.py + models/denoiser.py on CPU
(build container only).

    python tools/make_p_losses_golden.py            # needs the reference checkout

The recipe is tests/p_losses_cases.py make_golden(): the test-side code that may load the reference (the product and tools/ never do,
tests/test_host_cpu.py).  The reference's GaussianDiffusion.p_losses is run in .eval() with one timestep per sequence on the conftest's
seeded weights, under both objectives and both loss types; inputs are stored as seeds, weights as a checksum.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from p_losses_cases import make_golden  # noqa: E402

if __name__ == "__main__":
    make_golden(os.path.join(ROOT, "tests", "golden", "p_losses.npz"))
