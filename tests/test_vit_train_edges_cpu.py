"""No GPU: the cases of tests/test_gpu_vit_train_edges.py (tests/vit_train_edge_cases.py) are what they claim, from the reference alone.
  1. FIGURES: token counts, rows, patch rows, chunk counts and last-chunk lengths (vt_chunks restated in vit_train_checks) are pinned, and
     the five regime thresholds are inequalities on the cases' own numbers: a changed case cannot silently fall below one.
  2. SIGHT: conditions on the inputs, not measurements -- the last image of the two large cases alone moves every gradient tensor by more
     than 16 x that tensor's bound (its rows are the ones beyond every grid-stride wrap); the unresampled position table moves z by more
     than 100 x the bound where DINO resamples the trained grid, and by nothing where DINO copies; a row stride of 16 x gw moves z by more
     than 100 x the bound; the trained-like families are peaked / massive on these very inputs.  Where DINO resamples the trained grid
     onto its own size the yardstick's pos_embed gradient is held against a central difference of the oracle's forward (torch's CPU
     bicubic backward copies at equal sizes although its forward does not), and VitTrainer's tap matrices against the oracle's table.
  3. TEETH: every case's own distance (float32 autograd from float64 autograd) is finite and below 1e-4 for z, every tensor and every
     asserted block, so max(4 x own, floor) is a bound a wrong kernel misses.  Worst here: 7.3e-5 (pos_embed[patch]) and 6.7e-5 as a
     whole tensor (blocks.0.mlp.fc2.weight), both peaked_attention_x6; random-weight cases about 1e-6.  Three near-cancelled blocks of
     massive_channel (vit_train_edge_cases.CANCELLING_BLOCKS, up to 5.1e-4) are printed only."""
import copy
import functools
import os
import shutil
import subprocess

import pytest
import torch

from oracle import vit_oracle as VO
from posediffusion_amd import vit_train as VT
import vit_checks as V
import vit_train_checks as VC
import vit_train_edge_cases as EC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "posediffusion_amd", "csrc")


@functools.lru_cache(maxsize=None)
def _refs(name):
    """(images, g_z, (z64, g64), (z32, g32)) of a case: computed once, shared, never modified"""
    edge = EC.EDGES[name]
    net = EC.net_of(edge.family, edge.case.depth)
    images, g_z = VC.inputs(edge.case)
    return (images, g_z, VC.reference(net, images, g_z, edge.case.scales, torch.float64),
            VC.reference(net, images, g_z, edge.case.scales, torch.float32))


def _z_bound(name):
    _, _, (z64, _), (z32, _) = _refs(name)
    return VC.bound(VC.grad_dist(z32, z64))


# ------------------------------------------------------------------------------------------------ 1. figures
def test_vt_chunks_restatement():
    assert VC.vt_chunks(1) == (1, 32, 1) and VC.vt_chunks(256) == (1, 256, 256) and VC.vt_chunks(257) == (2, 160, 97)
    assert VC.vt_chunks(394) == (2, 224, 170)                               # the largest reduction of tests/test_gpu_vit_train.py: 2 chunks
    assert VC.vt_chunks(4096) == (16, 256, 256) and VC.vt_chunks(4097) == (15, 288, 65)
    for M in (1, 31, 255, 1000, 2758, 4096, 4352, 5280, 100000):
        chunks, r, last = VC.vt_chunks(M)
        assert 1 <= chunks <= 16 and r % 32 == 0 and 1 <= last <= r and (chunks - 1) * r + last == M


_CHUNKS_PROGRAM = r"""
#define PD_TR_LAUNCH_HOST_ONLY
#include "pd_train_launch.h"
#include <stdio.h>
int main() {
    for (int M = 1; M <= 20000; ++M) {
        int chunks, rows;
        pd_tr_chunks(M, &chunks, &rows);
        printf("%d %d %d\n", M, chunks, rows);
    }
    return 0;
}
"""


@pytest.mark.skipif(shutil.which("c++") is None and shutil.which("g++") is None, reason="no host C++ compiler")
def test_vt_chunks_is_pd_tr_chunks_of_the_launch_header(tmp_path):
    """the pinned figures above rest on vit_train_checks.vt_chunks: it is the trainers' one C++ rule, compiled from its header on the host"""
    src, exe = tmp_path / "chunks.cpp", tmp_path / "chunks"
    src.write_text(_CHUNKS_PROGRAM)
    cxx = shutil.which("c++") or shutil.which("g++")
    out = subprocess.run([cxx, "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [tuple(int(x) for x in line.split()) for line in subprocess.run([str(exe)], capture_output=True, text=True, timeout=30).stdout.splitlines()]
    assert [M for M, _, _ in rows] == list(range(1, 20001))
    for M, chunks, r in rows:
        assert (chunks, r) == VC.vt_chunks(M)[:2], (M, chunks, r, VC.vt_chunks(M))


@pytest.mark.parametrize("name", list(EC.EDGES))
def test_token_counts_and_the_family_limits(name):
    edge = EC.EDGES[name]
    case = edge.case
    assert EC.tokens(case) == edge.tokens
    assert max(edge.tokens) <= VT.MAX_TOKENS and min(edge.tokens) >= 2
    assert sum(edge.tokens) == VT.token_rows(case.H, case.W, case.scales)            # the engine side's own count
    assert [EC.scaled_size(case.H, case.W, sf) for sf in case.scales] == [VT.scaled_size(case.H, case.W, sf) for sf in case.scales]
    shape = VT.shape_from_module(EC.net_of(edge.family, case.depth))
    assert shape["depth"] == case.depth and shape["pos_grid"] == {"grid1": 1, "grid15": 15}.get(edge.family, 14)
    if name in EC.PIXELS:
        assert tuple(EC.scaled_size(case.H, case.W, sf) for sf in case.scales) == EC.PIXELS[name]


def test_row_counts_chunks_and_thresholds():
    for name in EC.ROWS:
        case = EC.EDGES[name].case
        assert EC.rows(case) == EC.ROWS[name] and EC.patch_rows(case) == EC.PATCH_ROWS[name]
        assert tuple(VC.vt_chunks(m) for m in EC.rows(case)) == EC.ROW_CHUNKS[name]
        assert tuple(VC.vt_chunks(m) for m in EC.patch_rows(case)) == EC.PATCH_ROW_CHUNKS[name]
    big, cap, five = (EC.EDGES[k].case for k in ("rows_2758", "chunk_cap", "five_images"))
    assert EC.rows(big)[0] == 2758 >= EC.WRAP_GELU_ASSEMBLE                  # GELU (float4) and token assembly take a second pass
    assert EC.patch_rows(big)[0] == 2744 >= EC.WRAP_IM2COL                   # so does im2col
    assert EC.rows(big)[0] >= EC.WRAP_DGRAD_REDUCE                           # and the reduce after a split data gradient
    assert EC.rows(cap)[0] == 4352 > EC.CHUNK_CAP_ROWS and EC.patch_rows(cap)[0] > EC.CHUNK_CAP_ROWS
    assert big.n == 14 > EC.IMAGES_PER_FINAL_WG and five.n == EC.IMAGES_PER_FINAL_WG + 1 and big.n % 4 == 2          # 4 workgroups, the last half full
    # chunk regimes: 11-, 3- and 1-chunk reductions in one call, the 1-chunk scale (1 / 3) runs first in the backward and writes
    assert [c for c, _, _ in EC.ROW_CHUNKS["rows_2758"]] == [11, 3, 1]
    assert EC.ROW_CHUNKS["chunk_cap"][0][:2] == (16, 288) and EC.PATCH_ROW_CHUNKS["chunk_cap"][0] == (16, 288, 15)
    for name, (first, last) in EC.LAST_IMAGE_ROWS.items():
        case = EC.EDGES[name].case
        assert (first, last) == ((case.n - 1) * EC.tokens(case)[0], EC.rows(case)[0] - 1)
    # the last image of rows_2758 holds EVERY row of the second grid-stride pass; chunk_cap's holds the whole last chunk
    assert EC.LAST_IMAGE_ROWS["rows_2758"][0] < EC.WRAP_GELU_ASSEMBLE - 1 and EC.LAST_IMAGE_ROWS["chunk_cap"][0] <= 4352 - 32


def test_key_tile_edges_and_geometry_cases_are_on_their_edges():
    assert sorted(EC.EDGES[k].tokens[0] for k in EC.KEY_TILE_EDGES) == [64, 65, 128, 128, 129, 192, 193]
    assert EC.grids(EC.EDGES["tokens_128_wide"].case) == [(1, 127)] and EC.grids(EC.EDGES["tokens_128_tall"].case) == [(127, 1)]
    ragged = EC.EDGES["ragged_pixels"].case
    assert all(h % 16 and w % 16 for h, w in EC.PIXELS["ragged_pixels"]) and 16 * EC.grids(ragged)[0][1] == 64 != ragged.W
    assert any(sf > 1 for sf in EC.EDGES["up_and_odd_scales"].case.scales)
    assert all(abs(1 / sf - round(1 / sf)) > 0.1 for sf in EC.EDGES["up_and_odd_scales"].case.scales)
    assert EC.grids(EC.EDGES["one_row_grid"].case) == [(1, 4)]
    for k in ("trained_grid_wide", "trained_grid_tall", "trained_grid_padded"):
        assert EC.grids(EC.EDGES[k].case) == [(14, 14)]
    assert EC.grids(EC.EDGES["grid15_native"].case) == [(15, 15)] and EC.grids(EC.EDGES["grid1_native"].case) == [(1, 1)]


# ------------------------------------------------------------------------------------------------ 2. the checks see what a case is there for
@pytest.mark.parametrize("name", list(EC.LAST_IMAGE_ROWS))
def test_the_last_image_alone_moves_every_gradient_tensor(name):
    edge = EC.EDGES[name]
    case = edge.case
    images, g_z, (_, g64), (_, g32) = _refs(name)
    part = VC.image_contribution(EC.net_of(edge.family, case.depth), images, g_z, case.scales, case.n - 1)
    worst = None
    for k in g64:
        rows = [(k, part[k], g32[k], g64[k])]
        b, b32, b64 = (VC.grad_blocks(k, t[k]) for t in (part, g32, g64))
        rows += [(f"{k}[{blk}]", b[blk], b32[blk], b64[blk]) for blk in b64 if not VC.is_k_bias(k, blk)]
        for lab, p, own, ref in rows:
            moved, bnd = p.abs().max().item() / ref.abs().max().item(), VC.bound(VC.grad_dist(own, ref))
            worst = min(worst or (moved / bnd, lab), (moved / bnd, lab))
            assert moved > 16 * bnd, (lab, moved, bnd)
    print(f"{name}: image {case.n - 1} alone moves every tensor by at least {worst[0]:.0f} x its bound ({worst[1]})")


@pytest.mark.parametrize("name,resampled", [("trained_grid_wide", True), ("trained_grid_tall", True), ("trained_grid_padded", False)])
def test_the_unresampled_table_is_wrong_exactly_where_dino_resamples(name, resampled):
    edge = EC.EDGES[name]
    images, _, (z64, _), _ = _refs(name)
    z_table = VC.z_on_unresampled_table(EC.net_of(edge.family, edge.case.depth), images, edge.case.scales)
    e, bnd = VC.grad_dist(z_table, z64), _z_bound(name)
    print(f"{name}: float64 z on the unresampled table is {e:.3e} from the oracle's (bound {bnd:.3e})")
    assert e > 100 * bnd if resampled else e == 0.0


@pytest.mark.parametrize("name", ["trained_grid_wide", "trained_grid_tall"])
def test_the_yardsticks_pos_embed_gradient_is_the_derivative_of_its_forward(name):
    """Where DINO resamples the trained grid onto its own size, torch's CPU bicubic FORWARD evaluates the scale factor and its BACKWARD
    copies: plain autograd is not the derivative there.  vit_train_checks.reference takes the adjoint of the forward itself; a central
    difference of the oracle's float64 forward along a random direction of the patch rows decides between the two."""
    edge = EC.EDGES[name]
    case = edge.case
    net = EC.net_of(edge.family, case.depth)
    images, g_z, (z64, g64), _ = _refs(name)
    assert torch.equal(z64, VO.multiscale_features(copy.deepcopy(net).double(), images.double(), case.scales))      # the forward is the oracle's
    d = torch.zeros(1, 197, 384, dtype=torch.float64)
    d[:, 1:] = torch.randn(1, 196, 384, dtype=torch.float64, generator=torch.Generator().manual_seed(5))

    def S(eps):
        m = copy.deepcopy(net).double()
        with torch.no_grad():
            m.pos_embed += eps * d
        return (VO.multiscale_features(m, images.double(), case.scales) * g_z.double()).sum().item()
    fd = (S(1e-4) - S(-1e-4)) / 2e-4
    ours = (g64["pos_embed"] * d).sum().item()
    m = copy.deepcopy(net).double()
    names = [k for k, _ in m.named_parameters()]
    plain = dict(zip(names, torch.autograd.grad((VC.multiscale(m, images.double(), case.scales) * g_z.double()).sum(), list(m.parameters()))))
    print(f"{name}: dS along a random direction of the patch rows: central difference {fd:+.8e}, reference {ours:+.8e}, "
          f"plain torch autograd {(plain['pos_embed'] * d).sum().item():+.8e}")
    assert abs(ours - fd) < 1e-6 * abs(fd)
    assert [k for k in g64 if k != "pos_embed" and not torch.equal(g64[k], plain[k])] == []        # every other tensor is plain autograd's
    assert torch.equal(g64["pos_embed"][:, :1], plain["pos_embed"][:, :1])                          # and so is the CLS row


@pytest.mark.parametrize("family,g", [("make_net", 14), ("grid15", 15), ("grid1", 1)])
def test_the_tap_matrices_are_dinos_resampling_of_the_trained_grid_onto_itself(family, g):
    """VitTrainer's table for the trained grid under unequal pixel sizes (torch's GPU bicubic kernel copies at equal sizes, so the trainer
    writes the resampling out) against the oracle's own float64 call"""
    net = copy.deepcopy(EC.net_of(family, 1)).double()
    with torch.no_grad():
        want = net.interpolate_pos_encoding(torch.zeros(1, 1 + g * g, 384, dtype=torch.float64), 16 * g, 16 * g + 8)[0]
        m = VT._bicubic_matrix(g, g)
        assert m.dtype == torch.float32 and m.shape == (g, g) and torch.allclose(m.sum(1), torch.ones(g), atol=1e-6)
        grid = net.pos_embed[0, 1:].reshape(g, g, 384)
        got = torch.einsum("yi,xj,ijc->yxc", m.double(), m.double(), grid).reshape(g * g, 384)
    e, moved = VC.grad_dist(got, want[1:]), VC.grad_dist(grid.reshape(g * g, 384), want[1:])
    print(f"grid {g}: tap matrices {e:.3e} from the oracle's resampled table; pos_embed itself is {moved:.3e} from it")
    assert e < 1e-6 and torch.equal(want[0], net.pos_embed[0, 0])
    assert moved > 1e-2 if g > 1 else moved < 1e-12                           # one cell resampled onto one cell: every tap clamps to it (weights sum to 1)


def test_a_row_stride_of_16_gw_is_seen_at_ragged_pixels():
    edge = EC.EDGES["ragged_pixels"]
    case = edge.case
    images, _, (z64, _), _ = _refs("ragged_pixels")
    wrong = VC.with_row_stride(images, 16 * (case.W // 16))
    assert wrong.shape == (case.n, 3, case.H, 64) and torch.equal(wrong[0, 0, 0], images[0, 0, 0, :64])
    assert torch.equal(wrong[0, 0, 1, :11], images[0, 0, 0, 64:]) and torch.equal(wrong[0, 0, 1, 11:], images[0, 0, 1, :53])
    assert EC.grids(VC.Case(case.n, case.H, 64, case.scales, 1)) == EC.grids(case)                  # the same token grids at every scale
    with torch.no_grad():
        z_wrong = VC.multiscale(copy.deepcopy(EC.net_of(edge.family, case.depth)).double(), wrong.double(), case.scales)
    e, bnd = VC.grad_dist(z_wrong, z64), _z_bound("ragged_pixels")
    print(f"ragged_pixels: float64 z of the buffer read with row stride 64 is {e:.3e} from the oracle's (bound {bnd:.3e})")
    assert e > 100 * bnd


def test_trained_like_families_are_what_they_claim_on_these_inputs():
    for name in ("peaked_attention_x6", "massive_channel"):
        edge = EC.EDGES[name]
        net64 = getattr(V, edge.family)(0, edge.case.depth, torch.float64)
        images, _ = VC.inputs(edge.case)
        if name in V.PEAKEDNESS:
            pmax, span = V.attention_stats(net64, images)
            print(f"{name}: mean largest attention probability {pmax:.3f}, largest logit range {span:.0f}")
            assert pmax >= V.PEAKEDNESS[name]
        else:
            rows = VO.token_rows(net64, images.double())
            print(f"{name}: least |channel {V.MASSIVE}| over the token rows {rows[..., V.MASSIVE].abs().min().item():.0f}")
            assert rows[..., V.MASSIVE].abs().min() > 250


# ------------------------------------------------------------------------------------------------ 3. the rule has teeth
@pytest.mark.parametrize("name", list(EC.EDGES))
def test_own_distance_is_finite_and_small(name):
    _, _, (z64, g64), (z32, g32) = _refs(name)
    owns = [("z", VC.grad_dist(z32, z64))]
    for k in g64:
        assert torch.isfinite(g64[k]).all() and torch.isfinite(g32[k]).all(), k
        owns.append((k, VC.grad_dist(g32[k], g64[k])))
        owns += [(f"{k}[{blk}]", own) for blk, _, own, _ in VC.block_dists(k, g32[k], g32[k], g64[k]) if not VC.is_k_bias(k, blk)]
    cancelling = EC.CANCELLING_BLOCKS.get(name, ())
    for lab in cancelling:                                                   # what the exception rests on: the block is a near-cancelled sum
        k, blk = lab[:-1].split("[")
        b = VC.grad_blocks(k, g64[k])
        ratio = (b[blk].abs().max() / g64[k].abs().max()).item()
        print(f"{name}: {lab} is {ratio:.1e} of its tensor's maximum in float64; own {dict(owns)[lab]:.3e} -- printed only")
        assert ratio < 1e-3 and dict(owns)[lab] < float("inf")
    worst = max((o, lab) for lab, o in owns if lab not in cancelling)
    print(f"{name}: z own {owns[0][1]:.3e}; largest own {worst[0]:.3e} ({worst[1]})")
    assert all(o == o and o < 1e-4 for lab, o in owns if lab not in cancelling), worst
