"""GPU: EVERY token row of the image feature extractor (csrc/pd_vit.hip and the strip / stream GEMMs it shares with the denoiser) against
the fp64 network, at the shapes where the kernels change behaviour and under trained-like weight statistics.

The earlier ViT tests compare the CLS feature only; tests/vit_checks.py and tests/test_vit_checks_cpu.py show why that misses a fault
confined to an edge row.  Here `VitEngine.tokens` (pd_debug_vit_tokens: the residual stream after the last block) is compared row by
row with `vit_oracle.token_rows` of the fp64 network, and the CLS feature with it.  Bound rule (vit_checks): the engine's error
<= max(4 x e32, floor) and < 1e-4, e32 being the CPU fp32 oracle's own distance from fp64 on the same inputs and weights, floor 2e-6 for
the CLS feature and TOKEN_FLOOR for token rows; a case is only used when 4 x e32 < 1e-4, asserted before the engine's result is looked at.
Every case prints its figures (`pytest -s`: profiles/vit_token_parity.txt).

Modes (PD_VIT_OPT_EXACT_FP32) matter from 1 024 token rows on: 1 = exact-fp32 streamed GEMMs, 0 = fp16 hi + lo planes (the default);
below, the small path is exact fp32 whatever the option says (mode `-`)."""
import ctypes as C
import math

import pytest
import torch

import vit_checks as V
from conftest import rel_err
from oracle import vit_oracle as VO
from posediffusion_amd import _lib
from posediffusion_amd.vit import VitEngine, vit_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STREAM_MIN_ROWS = 1024


def _engine(net32):
    return VitEngine(vit_state(net32), torch.device(DEV))


@pytest.fixture(scope="module")
def benign2():
    """make_vit(seed 0) truncated to 2 blocks: (fp32 network, fp64 network, engine)"""
    net32, net64 = V.oracle_pair(V.benign, 0, 2)
    eng = _engine(net32)
    yield net32, net64, eng
    eng.close()


def _modes_for(rows):
    return (1, 0) if rows >= STREAM_MIN_ROWS else (None,)


def _check(tag, eng, net32, net64, x, sf=1, skip=(), modes=None):
    """Token rows and CLS feature of `eng` on x against fp64 in every mode that applies; prints one line per mode, then asserts the bound
    rule for all of them.  Returns {mode: token rows (CPU)}."""
    ref64, e32, c32 = V.oracle_errs(net32, net64, x, sf, skip)
    assert torch.isfinite(ref64).all(), tag
    assert V.usable(e32["worst"]) and V.usable(c32), (tag, "the fp32 oracle itself leaves the bound rule no room", e32["worst"], c32)
    cls64 = V.cls_feature(net64, ref64)
    n, T, _ = ref64.shape
    modes = _modes_for(n * T) if modes is None else modes
    b_tok, b_cls = V.bound(e32["worst"], V.TOKEN_FLOOR), V.bound(c32, V.CLS_FLOOR)
    res, out = [], {}
    try:
        for mode in modes:
            if mode is not None:
                eng.set_exact_fp32(mode)
            got = eng.tokens(x.to(DEV), sf).cpu()
            z = eng.multiscale(x.to(DEV), (sf,)).cpu()
            assert got.shape == ref64.shape, (tag, got.shape, ref64.shape)
            e, c = V.token_row_errs(got, ref64, skip), rel_err(z, cls64)
            print(f"{tag} | {n} x {T} = {n * T} rows | mode {'-' if mode is None else mode} | token rows: e32 {e32['worst']:.2e}, engine {V.describe(e)}, "
                  f"bound {b_tok:.2e} | CLS: e32 {c32:.2e}, engine {c:.2e}, bound {b_cls:.2e}")
            res.append((mode, bool(torch.isfinite(got).all() and torch.isfinite(z).all()), e, c))
            out[mode] = got
    finally:
        eng.set_exact_fp32(0)
    for mode, finite, e, c in res:
        assert finite, (tag, mode, "non-finite output")
        assert e["worst"] <= b_tok and e["worst"] < V.CONTRACT, (tag, mode, "token rows vs fp64", V.describe(e), b_tok,
                                                                 "worst per query-block position", e["per_token_pos"].tolist())
        assert c <= b_cls and c < V.CONTRACT, (tag, mode, "CLS feature vs fp64", c, b_cls)
    return out


# ---- C.1: the token-count sweep ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,T", V.SWEEP, ids=[f"{h}x{w}_T{T}" for (h, w), T in V.SWEEP])
def test_token_count_sweep(benign2, hw, T):
    """one image, depth 2: T on and around the 32-key tile, the 8-key chunk, the 256 keys where the PV loop changes shape, VT_MAX = 1 056;
    the two shapes of >= 1 024 rows run the streamed GEMMs in modes 1 and 0"""
    net32, net64, eng = benign2
    assert V.tokens_of(*hw) == T
    _check(f"sweep {hw[0]} x {hw[1]}", eng, net32, net64, V.images(1, *hw, 100 + T))


def test_more_than_1056_tokens_stay_refused(benign2):
    """a return code, nothing is launched"""
    _, _, eng = benign2
    for hw in ((528, 528), (80, 3392)):                           # 1 090 tokens; 1 061, the first grid past the limit in the 80-pixel family
        assert V.tokens_of(*hw) > 1056
        with pytest.raises(RuntimeError, match="tokens per image"):
            eng.multiscale(torch.rand(1, 3, *hw).to(DEV), (1,))
        with pytest.raises(RuntimeError, match="tokens per image"):
            eng.tokens(torch.rand(1, 3, *hw).to(DEV))


# ---- C.2: both sides of 1 024 rows --------------------------------------------------------------------------------------------------------
THRESHOLD = [((112, 112), 20), ((112, 112), 21), ((64, 64), 60), ((64, 64), 61), ((16, 16), 511), ((16, 16), 512), ((224, 224), 5), ((224, 224), 6),
             ((224, 224), 7)]


@pytest.mark.parametrize("hw,n", THRESHOLD, ids=[f"{n}x{h}x{w}_{n * V.tokens_of(h, w)}rows" for (h, w), n in THRESHOLD])
def test_both_sides_of_the_streamed_threshold(benign2, hw, n):
    """1 000 / 1 050 rows (the headline workload's second scale: 20 images at 112 x 112), 1 020 / 1 037, 1 022 / 1 024, 985 / 1 182, and
    1 379 rows: ragged against 96-, 64- and 4-row tiles alike (35 over a multiple of 96 and of 64, 3 over a multiple of 4)"""
    net32, net64, eng = benign2
    rows = n * V.tokens_of(*hw)
    if n == 7:
        assert rows % 96 == 35 and rows % 64 == 35 and rows % 4 == 3
    _check(f"threshold {n} x {hw[0]} x {hw[1]}", eng, net32, net64, V.images(n, *hw, 200 + n))


# ---- C.3: batch independence ----------------------------------------------------------------------------------------------------------------
def test_token_rows_do_not_depend_on_the_rest_of_the_batch(benign2):
    """Within one path and mode, every kernel's tile shape is fixed (pd_gemm_strip / pd_gemm_stream: 96- / 64-row tiles whatever M;
    vit_gemm_kernel 32 x 32; the attention works per image): the rows of image i are bit for bit the same in a larger batch."""
    _, _, eng = benign2
    x = V.images(7, 224, 224, 33).to(DEV)
    try:
        for mode in (1, 0):
            eng.set_exact_fp32(mode)
            six, seven = eng.tokens(x[:6]), eng.tokens(x[:7])          # 1 182 and 1 379 rows: both streamed
            assert torch.equal(six, seven[:6]), (mode, (six - seven[:6]).abs().max().item())
    finally:
        eng.set_exact_fp32(0)
    two, three = eng.tokens(x[:2]), eng.tokens(x[:3])                  # 394 and 591 rows: the small path
    assert torch.equal(two, three[:2])


# ---- C.4: depth and grid limits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 12, 16])
def test_depth_1_12_16(depth):
    """VDEPTH_MAX = 16; 6 images of 224 x 224 (streamed, modes 1 and 0) and 2 images (small path)"""
    net32, net64 = V.oracle_pair(V.deep, 0, depth)
    assert len(net32.blocks) == depth
    eng = _engine(net32)
    try:
        x = V.images(6, 224, 224, 300 + depth)
        _check(f"depth {depth}, 6 images", eng, net32, net64, x)
        _check(f"depth {depth}, 2 images", eng, net32, net64, x[:2])
    finally:
        eng.close()


def test_depth_17_and_position_grid_16_are_refused():
    torch.manual_seed(0)
    with pytest.raises(RuntimeError, match="unsupported ViT shape"):
        _engine(VO.DinoViT(depth=17).eval())
    with pytest.raises(RuntimeError, match="unsupported ViT shape"):
        _engine(VO.DinoViT(img_size=256, depth=1).eval())              # 16 x 16 position grid (limit 15)


def test_network_trained_on_a_15x15_grid():
    """DinoViT(img_size=240): native size (no resampling, 226 tokens; 2 images small path, 5 images streamed) and resampled to 224"""
    net32, net64 = V.oracle_pair(V.grid15, 0, 2)
    eng = _engine(net32)
    try:
        assert eng.grid0 == 15 and eng._pos_for(240, 240) is None and eng._pos_for(224, 224) is not None
        _check("grid 15 at 240 x 240", eng, net32, net64, V.images(2, 240, 240, 41))
        _check("grid 15 at 240 x 240", eng, net32, net64, V.images(5, 240, 240, 42))
        _check("grid 15 resampled to 224 x 224", eng, net32, net64, V.images(2, 224, 224, 43))
    finally:
        eng.close()


# ---- C.5: workspace growth and reuse --------------------------------------------------------------------------------------------------------
def test_workspace_growth_and_reuse(benign2):
    """one engine: 2 images -> 7 images (the workspaces grow) -> 2 images again -> another image size; each result bitwise a fresh engine's"""
    net32, _, _ = benign2
    eng = _engine(net32)
    xs = [V.images(2, 224, 224, 51), V.images(7, 224, 224, 52), V.images(2, 224, 224, 51), V.images(3, 128, 192, 53)]
    try:
        for i, x in enumerate(xs):
            got = eng.tokens(x.to(DEV))
            fresh = _engine(net32)
            try:
                assert torch.equal(got, fresh.tokens(x.to(DEV))), i
            finally:
                fresh.close()
        # pd_debug_vit_tokens hands out what the last forward wrote, no more: 3 x 97 rows now
        buf = torch.empty(3 * 97 * 384 + 1, device=DEV)
        stream = torch.cuda.current_stream().cuda_stream
        assert eng.lib.pd_debug_vit_tokens(eng._h, buf.data_ptr(), buf.numel(), stream) != 0
        assert eng.lib.pd_debug_vit_tokens(eng._h, buf.data_ptr(), buf.numel() - 1, stream) == 0
    finally:
        eng.close()


def test_multiscale_is_unchanged_by_token_calls_in_between(benign2):
    """the three accumulating pd_vit_forward_scale calls of `multiscale`, with a `tokens` call of a LARGER batch (the workspaces grow)
    between every two of them: the same features bit for bit"""
    net32, _, _ = benign2
    eng = _engine(net32)
    try:
        x, other = V.images(2, 224, 224, 61).to(DEV), V.images(7, 224, 224, 62).to(DEV)
        sfs = (1, 1 / 2, 1 / 3)
        ref = eng.multiscale(x, sfs)
        z = torch.empty_like(ref)
        stream = torch.cuda.current_stream().cuda_stream
        for i, sf in enumerate(sfs):
            hs, ws = (224, 224) if sf == 1 else (int(math.floor(224 * sf)),) * 2
            pos = eng._pos_for(hs, ws)
            _lib.check(eng.lib.pd_vit_forward_scale(eng._h, x.data_ptr(), 2, 224, 224, C.c_double(float(sf)), None if pos is None else pos.data_ptr(),
                                                    C.c_float(1.0 / 3), int(i > 0), z.data_ptr(), stream), "pd_vit_forward_scale")
            eng.tokens(other[:3 + 2 * i])
        assert torch.equal(z, ref)
        assert torch.equal(eng.multiscale(x, sfs), ref)
    finally:
        eng.close()


# ---- D: the fp16-plane mode under trained-like weight statistics ----------------------------------------------------------------------------
FAMILY_CASES = [(n, d) for n, (_, ds, _) in sorted(V.FAMILIES.items()) for d in ds]


@pytest.mark.parametrize("name,depth", FAMILY_CASES, ids=[f"{n}_depth{d}" for n, d in FAMILY_CASES])
def test_fp16_plane_mode_under_trained_like_weights(name, depth):
    """The ViT counterpart of the denoiser's test_fp16_plane_mode_under_adversarial_operands: the static power-of-two scales of the fp16
    planes come from loose bounds (pd_plane_exponents); here the bounds are loose, the values sit far below them, the attention is peaked
    or the LayerNorm gains are spread.  6 images of 224 x 224 (1 182 rows: streamed), modes 1 and 0, every token row and the CLS feature
    against fp64; the default mode really ran on planes (its rows differ from the exact mode's)."""
    fam, _, skip = V.FAMILIES[name]
    net32, net64 = V.oracle_pair(fam, 0, depth)
    x = V.images(6, 224, 224, 31)
    if name in V.PEAKEDNESS:
        pmax, span = V.attention_stats(net64, x[:2])
        print(f"{name} depth {depth}: fp64 mean largest attention probability {pmax:.3f}, largest logit range {span:.0f}")
        assert pmax >= V.PEAKEDNESS[name], (name, pmax)
    eng = _engine(net32)
    try:
        got = _check(f"{name} depth {depth}", eng, net32, net64, x, skip=skip)
        if skip:                                                   # with the massive channel in the row norms too
            _check(f"{name} depth {depth}, all channels", eng, net32, net64, x)
        d = rel_err(got[0], got[1])
        print(f"{name} depth {depth}: fp16 planes vs exact fp32, whole tensor {d:.2e}")
        assert 0 < d, "the default mode did not run on fp16 planes"
    finally:
        eng.close()
