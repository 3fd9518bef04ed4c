"""CPU: the preconditions of tests/test_gpu_denoiser_attn_peaked.py, on the case table of tests/denoiser_attn_cases.py -- each case runs the
kernel it names, its softmax is peaked in float64 (and is not under the weights every other test uses), the bound that the fp32 CPU oracle's
own distance from fp64 gives stays under 1e-4, and the row maxima reach the keys at which the kernels' tiles and lane groups end.
Every fp64 / fp32 oracle is computed once per (network, shape, t)."""
import pytest
import torch

import denoiser_attn_cases as A
import engine_history_cases as H

ALL = A.CASES + A.MODE1_CASES
REFS = sorted({(c.net, c.B, c.N, c.t) for c in ALL})
LARGE_KERNELS = (A.SEQ0, A.SEQ1, A.SEQ2, A.MMA, A.QKV)


def test_the_table_holds_every_kernel_and_its_edges():
    ids = [c.id for c in ALL]
    assert len(set(ids)) == len(ids)
    two = [c for c in A.CASES if c.net == "two_f4" and c.t == 31]
    shapes = lambda k, **kw: [(c.B, c.N) for c in two if c.kernel == k and all(getattr(c, a) == v for a, v in kw.items())]   # noqa: E731
    assert shapes(A.SMALL) == A.SMALL_SHAPES and shapes(A.SEQ0) == A.SEQ0_SHAPES and shapes(A.MMA) == A.MMA_SHAPES
    assert shapes(A.QKV) == A.QKV_SHAPES and shapes(A.SEQ2) == A.SEQ2_SHAPES
    assert shapes(A.LONG0, cap=A.LARGE_CAP) == A.LONG_SHAPES and shapes(A.LONG2) == A.LONG_SHAPES and shapes(A.LONG0, cap=A.SMALL_CAP) == [(7, 20)]
    assert shapes(A.GEN) == [(5, 13), (2, 64)]
    for k in (A.SMALL, A.SEQ0, A.MMA, A.QKV, A.SEQ2, A.LONG2, A.GEN):          # the other timesteps and the 8-layer network, once per kernel
        assert {c.t for c in A.CASES if c.kernel == k} == {31, 99, 0}, k
        if k != A.GEN:
            assert any(c.net == "eight_f3" for c in A.CASES if c.kernel == k), k
    assert {c.net for c in A.CASES if c.kernel == A.GEN} == {"two_f4", "gen_hd8_f4", "gen_hd68_f4"}
    # the fused kernel's group edges (pd_qkv_attn.h): G N = 95 at 19 frames; 53 = 13 x 4 + 1 sequences of 20 frames
    assert (H.PD_QA_ROWS - 1) // 19 * 19 == H.PD_QA_ROWS - 1 and 53 % ((H.PD_QA_ROWS - 1) // 20) == 1
    assert not A.DROPPED


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.id)
def test_a_case_runs_the_kernel_it_names(case):
    """(a), and the capacity rules: one engine per (network, cap); large-batch cases just over 1 024 token rows on an engine that has the
    streamed path, small-path and generic cases below."""
    assert A.kernel_of(case) == case.kernel
    assert case.B <= case.cap[0] and case.N <= case.cap[1] and 1 <= case.N <= 64
    rows, cap_rows = case.B * case.N, case.cap[0] * case.cap[1]
    if case.kernel in LARGE_KERNELS or (case.long and case.cap != A.SMALL_CAP):
        assert cap_rows >= H.PD_STREAM_MIN_ROWS and H.PD_STREAM_MIN_ROWS <= rows < H.PD_STREAM_MIN_ROWS + 64, (rows, cap_rows)
    else:
        assert rows < H.PD_STREAM_MIN_ROWS and (case.generic or cap_rows < H.PD_STREAM_MIN_ROWS), (rows, cap_rows)
    twin = A.bitwise_twin(case)
    if case.kernel == A.QKV:                       # the two-launch twin of a fused case, under the same weights: the MFMA attention
        assert twin == case._replace(kernel=A.MMA, fused=0) and A.kernel_of(twin) == A.MMA
    elif case.long:                                # bitwise wherever include/pd_engine.h says so: everywhere but against the MFMA attention
        assert (twin is None) == (case.split == 2 and case.N <= 32 and case.cap != A.SMALL_CAP)
        assert twin is None or (A.kernel_of(twin) == twin.kernel and twin.kernel in (A.SMALL, A.SEQ0, A.SEQ1, A.SEQ2))
    else:
        assert twin is None


@pytest.mark.parametrize("net,B,N,t", REFS, ids=lambda v: str(v))
def test_preconditions_on_fp64(net, B, N, t):
    case = A.Case("", net, B, N, t)
    ref = A.reference_of(case)
    sd, nt, _, _ = A.network(net)
    x, z = A.inputs(case)
    keys = A.argmax_keys(sd, nt, x, t, z)
    _, pb = A.oracle(A.network(net, benign=True)[0], nt, x, t, z, torch.float64)
    benign = A.median_pmax(pb)
    print(f"{net} ({B}, {N}) t = {t}: fp64 median largest probability per layer {[f'{p:.3f}' for p in ref['pmax']]} "
          f"(f = 1: {[f'{p:.3f}' for p in benign]}); fp32 CPU oracle vs fp64 {ref['e32']:.2e}, bound {ref['bound']:.2e}; "
          f"{len(keys)} of {N} keys hold a row maximum")
    # (b) peaked, (e) and not so under the weights of every other test
    if N >= A.PMAX_MIN_N:
        assert min(ref["pmax"]) >= A.PMAX_THRESHOLD[net], ref["pmax"]
        assert max(benign) < A.BENIGN_PMAX, benign
    # (c) the bound is one: 4 x the fp32 oracle's own distance stays under the 1e-4 the output must meet anyway
    assert ref["bound"] == max(A.TOL, A.MARGIN * ref["e32"]) and A.MARGIN * ref["e32"] < A.CEIL, ref["e32"]
    assert torch.isfinite(ref["out64"]).all()
    # (d) the row maxima reach the first and the last key, and every group of 8 keys (the MFMA softmax reduces over 8 lanes of 4 keys;
    #     with it both 16-key tiles)
    if N >= 16:
        assert 0 in keys and N - 1 in keys, keys
        for g0 in range(0, N, 8):
            assert any(g0 <= k < g0 + 8 for k in keys), (g0, keys)
