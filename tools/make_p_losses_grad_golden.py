"""Generate tests/golden/p_losses_grad.npz by executing the UNMODIFIED reference models/gaussian_diffuser.py + models/denoiser.py on CPU
(build container only).

    python tools/make_p_losses_grad_golden.py       # needs the reference checkout

The recipe is tests/train_checks.py make_grad_golden(): the test-side code that may load the reference (the product and tools/ never do,
tests/test_host_cpu.py).  The reference's GaussianDiffusion.p_losses is run in .eval() on case b3n5 of tests/p_losses_cases.py under
pred_noise / l1 and pred_x0 / l2, and ``loss.mean().backward()`` gives the parameter gradients; per tensor the fixture keeps max|g|,
sum(g) and 64 entries at seeded indices.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from train_checks import make_grad_golden  # noqa: E402

if __name__ == "__main__":
    make_grad_golden(os.path.join(ROOT, "tests", "golden", "p_losses_grad.npz"))
