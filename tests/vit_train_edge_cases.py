"""The cases of the backbone trainer's edge tests (include/pd_engine_vit_train.h, posediffusion_amd/csrc/pd_vit_train.hip): a plain module
shared by tests/test_vit_train_edges_cpu.py (which pins every figure below from the reference alone, so no case can drift below the
threshold it is there for) and tests/test_gpu_vit_train_edges.py.  Cases and pure-Python figures only; images and g_z are
vit_train_checks.inputs(case), nets are vit_train_checks.make_net or a builder of tests/vit_checks.py at seed 0.

ROW COUNTS -- where the host code changes regime above the 394 rows of tests/test_gpu_vit_train.py (M = token rows of one scale):
  * pd_vt_final_kernel takes 4 images per workgroup: a second workgroup from 5 images on                              (IMAGES_PER_FINAL_WG)
  * pd_vt_gelu_kernel / _bwd (float4) and pd_vt_assemble_kernel are capped at 4 096 workgroups of 256 threads: the grid-stride loop takes
    a second pass when M x 1536 / 4 > 1 048 576 and M x 384 > 1 048 576, both M >= 2 731                               (WRAP_GELU_ASSEMBLE)
  * pd_vt_im2col_kernel is capped at 8 192 workgroups: n P x 768 > 2 097 152, patch rows >= 2 731                      (WRAP_IM2COL)
  * the reduce after a split vt_dgrad is capped at 2 048 workgroups: M x 384 > 524 288, M >= 1 366                      (WRAP_DGRAD_REDUCE)
  * vt_chunks gives ceil(M / 256) chunks up to 16; above M = 4 096 the chunk length grows instead                      (CHUNK_CAP_ROWS)
  rows_2758    14 x 224 x 224 at (1, 1/2, 1/3): 2 758 / 700 / 238 rows, 2 744 patch rows at scale 1.  Every wrap above; 11-, 3- and 1-chunk
               reductions with the accumulate path on the 11- and 3-chunk ones (the scales run in reverse: 1/3 writes); 4 final-LayerNorm
               workgroups, the last half full.  Image 13 holds rows 2 561 .. 2 757: every row of the second grid-stride pass (from row 2 731).
  chunk_cap    17 x 240 x 272: 4 352 rows = 16 chunks of 288, the last of 32; 4 335 patch rows = 16 chunks of 288, the last of 15.
  five_images  5 x 48 x 32: the smallest second workgroup of the final kernels.
GEOMETRY -- every size of tests/test_gpu_vit_train.py has W = 16 x gw and a scale of 1 / k:
  ragged_pixels       2 x 100 x 75 at (1, 1/2, 1/3): 100 x 75, 50 x 37 and 33 x 25 pixels, 25 / 7 / 3 tokens; an im2col with 16 x gw = 64 for
                      the row stride reads other pixels
  up_and_odd_scales   2 x 40 x 56 at (1.5, 0.75): 60 x 84 and 30 x 42 pixels, 16 and 3 tokens
  one_row_grid        2 x 16 x 64: gh = 1, every vertical bicubic tap of the position grid clamps
  trained_grid_wide / _tall   1 x 224 x 232 and 1 x 232 x 224: the trained 14 x 14 grid, which DINO nevertheless RESAMPLES (its copy branch
                      asks for height == width); trained_grid_padded, 1 x 230 x 230, is the copy branch
KEY-TILE EDGES at head dim 64, one image each: 64, 65, 128 (1 x 127 and 127 x 1 grids), 129, 192 and 193 tokens.
SHAPE FAMILY: position grid 1 (vit_checks.grid1) and 15 (grid15), each native and resampled; depth 16 (deep).
TRAINED-LIKE WEIGHTS, 3 x 96 x 96, three scales, depth 2: peaked_attention_x6 (softmax backward with underflowing keys), massive_channel
  (LayerNorm backward with one dominant channel), wide_gamma_1p0 (spread gains).  tiny_gelu_outputs is left out on purpose: torch's own
  float32 is 3e-3 from float64 there, so the 4 x own rule says nothing.
"""
import functools
import math
from typing import NamedTuple, Tuple

import torch

import vit_checks as V
import vit_train_checks as VC

PATCH = 16
ONE, THREE = (1,), VC.THREE


class Edge(NamedTuple):
    case: VC.Case
    family: str                       # "make_net" (vit_train_checks.make_net) or the name of a builder of vit_checks
    tokens: Tuple[int, ...]           # tokens per image at each scale of the call: pinned by the CPU test


EDGES = {
    # row counts
    "rows_2758": Edge(VC.Case(14, 224, 224, THREE, 1), "make_net", (197, 50, 17)),
    "chunk_cap": Edge(VC.Case(17, 240, 272, ONE, 1), "make_net", (256,)),
    "five_images": Edge(VC.Case(5, 48, 32, ONE, 1), "make_net", (7,)),
    # geometry
    "ragged_pixels": Edge(VC.Case(2, 100, 75, THREE, 1), "make_net", (25, 7, 3)),
    "up_and_odd_scales": Edge(VC.Case(2, 40, 56, (1.5, 0.75), 1), "make_net", (16, 3)),
    "one_row_grid": Edge(VC.Case(2, 16, 64, ONE, 1), "make_net", (5,)),
    "trained_grid_wide": Edge(VC.Case(1, 224, 232, ONE, 1), "make_net", (197,)),
    "trained_grid_tall": Edge(VC.Case(1, 232, 224, ONE, 1), "make_net", (197,)),
    "trained_grid_padded": Edge(VC.Case(1, 230, 230, ONE, 1), "make_net", (197,)),
    # key-tile edges of the attention kernels at head dim 64
    "tokens_64": Edge(VC.Case(1, 144, 112, ONE, 1), "make_net", (64,)),
    "tokens_65": Edge(VC.Case(1, 128, 128, ONE, 1), "make_net", (65,)),
    "tokens_128_wide": Edge(VC.Case(1, 16, 2032, ONE, 1), "make_net", (128,)),
    "tokens_128_tall": Edge(VC.Case(1, 2032, 16, ONE, 1), "make_net", (128,)),
    "tokens_129": Edge(VC.Case(1, 128, 256, ONE, 1), "make_net", (129,)),
    "tokens_192": Edge(VC.Case(1, 16, 3056, ONE, 1), "make_net", (192,)),
    "tokens_193": Edge(VC.Case(1, 192, 256, ONE, 1), "make_net", (193,)),
    # the shape family's limits
    "grid1_two_scales": Edge(VC.Case(2, 48, 32, (1, 1 / 2), 1), "grid1", (7, 2)),
    "grid1_native": Edge(VC.Case(2, 16, 16, ONE, 1), "grid1", (2,)),
    "grid15_native": Edge(VC.Case(2, 240, 240, ONE, 1), "grid15", (226,)),
    "grid15_three_scales": Edge(VC.Case(2, 240, 240, THREE, 1), "grid15", (226, 50, 26)),
    "depth_16": Edge(VC.Case(2, 96, 96, THREE, 16), "deep", (37, 10, 5)),
    # trained-like weights
    "peaked_attention_x6": Edge(VC.Case(3, 96, 96, THREE, 2), "peaked_attention_x6", (37, 10, 5)),
    "massive_channel": Edge(VC.Case(3, 96, 96, THREE, 2), "massive_channel", (37, 10, 5)),
    "wide_gamma_1p0": Edge(VC.Case(3, 96, 96, THREE, 2), "wide_gamma_1p0", (37, 10, 5)),
}
KEY_TILE_EDGES = tuple(k for k in EDGES if k.startswith("tokens_"))

# thresholds of the docstring, as the smallest count that is past them
IMAGES_PER_FINAL_WG = 4
WRAP_GELU_ASSEMBLE = 2731             # M x 384 > 4 096 x 256 (and M x 1536 / 4 likewise)
WRAP_IM2COL = 2731                    # patch rows x 768 > 8 192 x 256
WRAP_DGRAD_REDUCE = 1366              # M x 384 > 2 048 x 256
CHUNK_CAP_ROWS = 4096                 # 16 chunks x 256 rows
assert (WRAP_GELU_ASSEMBLE - 1) * 384 <= 4096 * 256 < WRAP_GELU_ASSEMBLE * 384
assert (WRAP_IM2COL - 1) * 768 <= 8192 * 256 < WRAP_IM2COL * 768
assert (WRAP_DGRAD_REDUCE - 1) * 384 <= 2048 * 256 < WRAP_DGRAD_REDUCE * 384

# (pixels per scale) and (chunks, rows per chunk, rows of the last chunk) per reduction: pinned by the CPU test from vt_chunks restated
PIXELS = {"ragged_pixels": ((100, 75), (50, 37), (33, 25)), "up_and_odd_scales": ((60, 84), (30, 42))}
ROWS = {"rows_2758": (2758, 700, 238), "chunk_cap": (4352,), "five_images": (35,)}
PATCH_ROWS = {"rows_2758": (2744, 686, 224), "chunk_cap": (4335,), "five_images": (30,)}
ROW_CHUNKS = {"rows_2758": ((11, 256, 198), (3, 256, 188), (1, 256, 238)), "chunk_cap": ((16, 288, 32),), "five_images": ((1, 64, 35),)}
PATCH_ROW_CHUNKS = {"rows_2758": ((11, 256, 184), (3, 256, 174), (1, 224, 224)), "chunk_cap": ((16, 288, 15),), "five_images": ((1, 32, 30),)}
# Blocks whose OWN distance is not held below 1e-4 by the CPU test (every whole tensor and every other block is): under massive_channel the
# LayerNorm rows of block 1 are all close to +- sqrt(384) e_137, so hn is nearly the same for every token, while the key gradients of a
# softmax row sum to zero and the query gradients nearly so: dW_q / dW_k = sum_tokens d{q, k}^T hn cancel to 1e-4 .. 3e-4 of the v rows'
# magnitude, and float32 autograd itself is 0.9e-4 (q) and 5.1e-4 (k) of the block's maximum from float64.  The GPU test holds them to
# max(4 x own, floor) like every block; only the "own < 1e-4" condition is not asked of them.
CANCELLING_BLOCKS = {"massive_channel": ("blocks.1.attn.qkv.weight[q]", "blocks.1.attn.qkv.weight[k]", "blocks.1.attn.qkv.bias[q]")}
LAST_IMAGE_ROWS ={"rows_2758": (2561, 2757), "chunk_cap": (4096, 4351)}      # the scale-1 rows of the last image: past every wrap


def scaled_size(H, W, sf):
    """pixels of one scale: F.interpolate's floor(size x scale_factor) in double; a scale of 1 keeps the image"""
    return (H, W) if sf == 1 else (int(math.floor(H * float(sf))), int(math.floor(W * float(sf))))


def grids(case):
    """[(gh, gw)] of a case's scales"""
    return [(h // PATCH, w // PATCH) for h, w in (scaled_size(case.H, case.W, sf) for sf in case.scales)]


def tokens(case):
    return tuple(1 + gh * gw for gh, gw in grids(case))


def rows(case):
    """token rows of each scale"""
    return tuple(case.n * t for t in tokens(case))


def patch_rows(case):
    return tuple(case.n * (t - 1) for t in tokens(case))


@functools.lru_cache(maxsize=None)
def net_of(family, depth):
    """the float32 CPU network of a case: shared, never modified (the references differentiate copies)"""
    if family == "make_net":
        return VC.make_net(depth)
    return getattr(V, family)(0, depth, torch.float32)
