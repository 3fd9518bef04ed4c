"""GPU (-m gpu): the sampling denoiser's attention kernels at N <= 64 under a PEAKED softmax (trained-like weights: W_q and W_k x 3 or x 4,
median largest probability 0.5 .. 0.95 where every other test has 0.03 .. 0.11) -- pd_attn_kernel, pd_attn_seq_kernel<0 / 2>,
pd_attn_mma_kernel<2>, pd_qkv_attn_kernel (what bench.py runs), pd_attn_long_kernel<0 / 2> forced at N <= 64 and pd_gen_attn_kernel.
The cases, their networks and the fp64 / fp32 oracles are tests/denoiser_attn_cases.py; tests/test_denoiser_attn_cases_cpu.py asserts
their preconditions.

Rule for every case, against fp64, per pose column group over ALL sequences (the fused kernel groups sequences: none is sampled):
    err <= max(2e-5, 4 x e32)   and   err < 1e-4,       e32 = the fp32 CPU oracle's own distance from fp64
(2e-5: the suite's teacher-forced tolerance; 4 x: the margin of test_long_denoiser_with_peaked_attention and vit_checks; no figure of the
engine enters the bound).  Bitwise: every case replayed; the fused kernel against its two launches; the forced key-tiled kernel against the
kernel it replaces wherever include/pd_engine.h says so (not against pd_attn_mma_kernel).  Mode 1 (bf16 planes) is a separately reported
mode: bitwise long-attn equality and finiteness, its distance printed.

Measured (profiles/denoiser_peaked_attention.txt): every path within 0.7 .. 1.7 x e32.  What the rule sees of a wrong build: Q K^T on single
fp16 operands misses it by 50 x; 16-bit q and k in the MFMA / fused kernels misses it in 5 of 19 cases; 16-bit K in pd_attn_seq_kernel stays
inside the 4 x margin (2 .. 3 x e32) and fails only the bitwise relations; __expf in the softmax is below fp32's own noise."""
import time

import pytest
import torch

import denoiser_attn_cases as A
import engine_history_cases as H
from conftest import pose_err, pose_group_errs
from posediffusion_amd import _lib
from posediffusion_amd.engine import PoseEngine
from posediffusion_amd.schedule import diffusion_buffers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def engines():
    """One engine per (network, capacity, generic): created at the first case that needs it, closed with the module."""
    made = {}

    def get(case: A.Case) -> PoseEngine:
        key = (case.net, case.cap, case.generic)
        if key not in made:
            sd, _, kw, _ = A.network(case.net)
            made[key] = PoseEngine(sd, diffusion_buffers(), device=torch.device(DEV), max_B=case.cap[0], max_N=case.cap[1],
                                   generic=case.generic and not case.net.startswith("gen_"), **kw)
        return made[key]

    try:
        yield get
    finally:
        for eng in made.values():
            eng.close()


def _run(eng: PoseEngine, case: A.Case, x, z):
    """One Denoiser.forward under the case's three options (an engine below 1 024 rows of capacity has no split modes)."""
    if case.cap[0] * case.cap[1] >= H.PD_STREAM_MIN_ROWS and not case.generic:
        eng.set_split_precision(case.split)
        assert eng.get_option(_lib.PD_OPT_DENOISER_SPLIT) == case.split
    eng.set_option(_lib.PD_OPT_DENOISER_FUSED_ATTN, case.fused)
    eng.set_option(_lib.PD_OPT_DENOISER_LONG_ATTN, case.long)
    return eng.denoise(x, z, case.t)


def _differing(a, b):
    bad = (a != b).reshape(a.shape[0], -1).any(dim=1).nonzero().flatten().tolist()
    return f"sequences {bad[:12]} (of {len(bad)}) differ, by {pose_group_errs(a, b)}"


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.id)
def test_peaked_attention_vs_fp64(engines, case):
    t0 = time.perf_counter()
    ref = A.reference_of(case)
    t1 = time.perf_counter()
    eng = engines(case)
    x, z = (v.to(DEV) for v in A.inputs(case))
    out = _run(eng, case, x, z)
    again = _run(eng, case, x, z)
    twin = A.bitwise_twin(case)
    other = _run(eng, twin, x, z) if twin is not None else None
    eng.check_async()
    finite = bool(torch.isfinite(out).all())
    groups = pose_group_errs(out, ref["out64"]) if finite else {}
    err = pose_err(out, ref["out64"], tag=f"attn_peaked/{case.id}") if finite else float("inf")
    b, n, _ = A.worst_row(out, ref["out64"]) if finite else (-1, -1, 0.0)
    print(f"{case.id}: engine {err:.3e} {({g: f'{v:.2e}' for g, v in groups.items()})}, fp32 CPU oracle {ref['e32']:.3e}, bound {ref['bound']:.3e}, "
          f"worst row (sequence {b}, frame {n}); median largest probability {[f'{p:.2f}' for p in ref['pmax']]}; "
          f"bitwise twin {twin.id if twin else None}; wall {time.perf_counter() - t0:.2f} s (oracles {t1 - t0:.2f} s)")
    assert finite
    assert torch.equal(out, again), "replayed: " + _differing(out, again)
    if twin is not None:
        assert torch.equal(out, other), f"against {twin.id}: " + _differing(out, other)
    assert err <= ref["bound"] and err < A.CEIL, (err, ref["bound"], groups, (b, n))


@pytest.mark.parametrize("case", A.MODE1_CASES, ids=lambda c: c.id)
def test_bf16_plane_mode_is_finite_and_long_attn_is_bitwise(engines, case):
    ref = A.reference_of(case)
    eng = engines(case)
    x, z = (v.to(DEV) for v in A.inputs(case))
    try:
        out = _run(eng, case, x, z)
        forced = _run(eng, case._replace(kernel=A.LONG1, long=1), x, z)
        eng.check_async()
    finally:
        eng.set_split_precision(2)
    assert torch.isfinite(out).all()
    print(f"{case.id}: bf16 planes {pose_group_errs(out, ref['out64'])} from fp64 (fp32 CPU oracle {ref['e32']:.3e}); reported, not bounded")
    assert torch.equal(out, forced), _differing(out, forced)
