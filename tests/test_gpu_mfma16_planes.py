"""GPU (-m gpu): the large-batch fp16-plane products on v_mfma_f32_16x16x32_f16 (pd_gemm_strip_kernel's 64-k form, pd_qkv_attn_kernel) --
fp16 subnormals on the new instruction, partly filled and skipped 16-row tiles of the fused kernel, independence of a row's sums from
the tile and lane it sits in, and the strip GEMM's row edges.  Engines of 33 - 129 sequences: just over the 1 024 token rows at which the
plane path runs.  Everything goes through the C-ABI; the fp64 references are computed once per (shape, t) and shared.
"""
import ctypes as C

import pytest
import torch

from conftest import rel_err
from oracle import pd_oracle as O
from posediffusion_amd import _lib, synth
from posediffusion_amd.engine import PoseEngine
from posediffusion_amd.host import denoiser_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_REF = {}


def _engine(diff, B, N):
    dev = torch.device(DEV)
    diff = diff.to(dev)
    eng = PoseEngine(denoiser_state(diff.model), {k: v for k, v in diff.named_buffers(recurse=False)}, device=dev, max_B=B, max_N=N)
    eng.set_split_precision(2)
    assert eng.get_option(_lib.PD_OPT_DENOISER_SPLIT) == 2
    return eng


def _inputs(B, N):
    g = torch.Generator().manual_seed(1000 * B + N)
    return torch.randn(B, N, 9, generator=g), synth.make_z(B, N, seed=3 * B + N)


def _ref(oracle_weights, B, N, t, sub):
    """fp64 oracle on the sequences `sub` of _inputs(B, N), computed once per key"""
    key = (B, N, t, tuple(sub))
    if key not in _REF:
        x, z = _inputs(B, N)
        sd64 = {k: v.double() for k, v in oracle_weights.items()}
        with torch.no_grad():
            _REF[key] = O.denoiser_forward(sd64, x[sub].double(), torch.full((len(sub),), t, dtype=torch.long), z[sub].double())
    return _REF[key]


def test_fp16_matrix_pipe_16x16x32_keeps_subnormal_operands():
    """test_gpu_parity_r4's subnormal check on v_mfma_f32_16x16x32_f16: the `lo` halves of small elements are fp16 subnormals, a flushed
    operand would leave those elements 11 bits of 22.  pd_debug_mfma_f16_subnormal with its shape selector set; constant matrices, 32 k per instruction: 32 x 2^-20 x 2^10 = 2^-5 when kept (0 when
    flushed, either operand), a subnormal x normal product far below fp16's range (fp32 accumulation), 32 for the control."""
    lib = _lib.load()
    out = (C.c_float * 4)(32.0, 0.0, 0.0, 0.0)          # out[0] = 32 on entry: the 16x16x32 shape (include/pd_engine.h)
    with torch.cuda.device(DEV):
        _lib.check(lib.pd_debug_mfma_f16_subnormal(out, torch.cuda.current_stream().cuda_stream), "pd_debug_mfma_f16_subnormal")
    got = list(out)
    print("v_mfma_f32_16x16x32_f16 with fp16-subnormal operands (A sub, B sub, sub x 2^-4, control):", got)
    assert got[3] == 32.0
    assert got[0] == 2.0 ** -5 and got[1] == 2.0 ** -5, "the 16x16x32 form flushes fp16-subnormal operands: the lo plane would need its own scale"
    assert got[2] == 32.0 * 2.0 ** -24


# (B, N): rows of a workgroup of the fused kernel = (95 // N) N, of its last group (B mod (95 // N)) N
@pytest.mark.parametrize("B,N", [(52, 20),       # 80 rows: five full 16-row tiles, one skipped
                                 (53, 20),       # last group of one sequence: 20 rows = one full tile + 4 rows, four tiles skipped
                                 (54, 19),       # G = 5, 95 rows: a last tile with 15 rows
                                 (33, 32),       # G = 2, 64 rows: two tiles skipped; last group of one sequence: 32 rows
                                 (129, 8)])      # G = 11, 88 rows
def test_fused_kernel_partly_filled_and_skipped_tiles(seeded_diffuser, oracle_weights, B, N):
    """pd_qkv_attn_kernel runs ceil(rows / 16) of its six 16-row tiles and stages only their rows: forced on (PD_OPT_DENOISER_FUSED_ATTN = 2) it
    must equal the two-launch path bit for bit on every sequence, and the fp64 oracle within test_fused_qkv_attention_is_bitwise_the_two_launch_path's
    bound (3e-6) on the first, the last and a middle sequence, at t = 99 and 0."""
    eng = _engine(seeded_diffuser, B, N)
    x, z = _inputs(B, N)
    sub = [0, B // 2, B - 1]
    for t in (99, 0):
        eng.set_option(_lib.PD_OPT_DENOISER_FUSED_ATTN, 2)
        fused = eng.denoise(x.to(DEV), z.to(DEV), t)
        eng.set_option(_lib.PD_OPT_DENOISER_FUSED_ATTN, 0)
        plain = eng.denoise(x.to(DEV), z.to(DEV), t)
        assert torch.isfinite(fused).all()
        bad = (fused != plain).reshape(B, -1).any(dim=1).nonzero().flatten().tolist()
        assert not bad, f"t={t}: sequences {bad[:12]} (of {len(bad)}) differ between the fused and the two-launch attention"
        ref = _ref(oracle_weights, B, N, t, sub)
        worst = max(rel_err(fused[s], ref[i]) for i, s in enumerate(sub))
        print(f"(B, N) = ({B}, {N}), t = {t}: fused = two-launch bit for bit; worst of sequences {sub} vs fp64: {worst:.2e}")
        assert worst < 3e-6, (t, worst)
    eng.close()


def test_a_rows_sums_do_not_depend_on_its_tile_or_lane(seeded_diffuser):
    """(53, 20): sequences 0, 3 and 52 get the same x and z.  Sequence 0 opens its group (rows 0 - 19), sequence 3 sits in rows 60 - 79 across a
    16-row tile boundary, sequence 52 is alone in the last group (four tiles skipped): nothing in a row's sums depends on where it sits, so
    the three outputs are equal bit for bit -- on the fused kernel and on the two-launch path (strip GEMM rows 0, 60 and 1 040 on).
    (Holds on the 32x32x16 build too: run once against the parent commit's library, profiles/mfma16_planes.txt.)"""
    B, N = 53, 20
    eng = _engine(seeded_diffuser, B, N)
    x, z = _inputs(B, N)
    for s in (3, 52):
        x[s], z[s] = x[0], z[0]
    for fused in (2, 0):
        eng.set_option(_lib.PD_OPT_DENOISER_FUSED_ATTN, fused)
        for t in (99, 0):
            out = eng.denoise(x.to(DEV), z.to(DEV), t)
            assert torch.isfinite(out).all()
            assert torch.equal(out[0], out[3]) and torch.equal(out[0], out[52]), (fused, t, rel_err(out[3], out[0]), rel_err(out[52], out[0]))
            assert not torch.equal(out[0], out[1])
    eng.close()


@pytest.mark.parametrize("B,N", [(52, 20),       # 1 040 rows: ten 96-row blocks + 80 rows (64-row blocks: sixteen + 16 rows)
                                 (103, 20)])     # 2 060 rows: a last block of 44 rows at either block height: two full 16-row tiles + 12 rows
def test_strip_gemm_row_edges(seeded_diffuser, oracle_weights, B, N):
    """One denoiser step on the two-launch path (fused option 0), whose four GEMMs per layer are pd_gemm_strip_kernel launches with a ragged last row
    block, against fp64 with test_denoiser_at_the_bench_launch_shapes' bound: within 2 x the exact-fp32 mode's error (floor 2e-6), itself under
    2e-5; the compared sequences include the ones whose rows lie in the last row block.  (That rows >= M of the engine's buffers stay untouched is NOT
    checked here: no debug accessor reaches those buffers; the kernel's stores are guarded by row < M as before.)"""
    eng = _engine(seeded_diffuser, B, N)
    eng.set_option(_lib.PD_OPT_DENOISER_FUSED_ATTN, 0)
    x, z = _inputs(B, N)
    sub = sorted({0, B // 2, B - 3, B - 2, B - 1})
    for t in (99, 0):
        ref = _ref(oracle_weights, B, N, t, sub)
        err = {}
        for mode in (0, 2):
            eng.set_split_precision(mode)
            out = eng.denoise(x.to(DEV), z.to(DEV), t)
            assert torch.isfinite(out).all()
            err[mode] = max(rel_err(out[s], ref[i]) for i, s in enumerate(sub))
        print(f"(B, N) = ({B}, {N}), t = {t}: worst of sequences {sub} vs fp64: exact fp32 {err[0]:.2e}, fp16 planes {err[2]:.2e}")
        assert err[0] < 2e-5 and err[2] <= max(2.0 * err[0], 2e-6), (t, err)
    eng.close()
