"""CPU: the scenes of tests/ggs_pair_items_cases.py hold what their docstring says -- sizes, work items per big pair, and the oracle-side
figures (valid matches equal in fp64 and fp32, no Sampson value near the threshold, iterations stepped) that make them fit to judge a
kernel by -- and the option's constant is the header's.

The scenes of 40 .. 256 frames (cases.LONG_SCENES) must also let the checks of tests/ggs_checks.py SEE every work item of every big pair:
with one item's matches removed, the fp64 gradient at the start point moves, in at least one column group, by more than 10 x the bound
check_loss_grad applies.  A kernel that dropped, repeated or misplaced one item of one pair would then miss that bound by a wide margin.

Oracle time for scene256 on one CPU thread (68 511 matches): loss and gradient in fp64 and fp32 0.6 s, GGS_optimize(iter_num=3) in both
2.1 s; building the scene 6 s.  The shortened guide costs about as much again per precision, which is why
tests/test_gpu_ggs_pair_items_long.py computes the guide oracle only for scene129 and scene100_both."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import ggs_pair_items_cases as cases
from ggs_checks import (FLOOR_GRAD, K_GRAD, _x, bounds, grad_group_errs, one_thread, oracle_guide, oracle_loss_grad,
                        oracle_optimize)
from oracle import pd_oracle as O
from posediffusion_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _figures(md, pm, x0, big):
    n64, _, _ = oracle_loss_grad(x0, pm)
    n32, _, _ = oracle_loss_grad(x0, pm, torch.float32)
    with one_thread():
        s, _ = O.compute_sampson_distance(_x(x0, torch.float64), pm, sampson_max=float("inf"))
    in_big = tuple(int((s[r] < 10).sum()) for r in cases.big_pair_rows(md, big))
    steps = (oracle_optimize(x0, pm, iter_num=3)[1], oracle_optimize(x0, pm, torch.float32, iter_num=3)[1])
    return n64, n32, in_big, float((s - 10).abs().min()) / 10, steps


def _shape(md, N, big):
    key = md["i12"][:, 0] * N + md["i12"][:, 1]
    cnt = np.bincount(key, minlength=N * N)
    items = [-(-int(cnt[i * N + j]) // 512) for (i, j) in sorted(big)]
    assert [int(cnt[i * N + j]) for (i, j) in sorted(big)] == [c for _, c in sorted(big.items())]
    sorted_upload = bool((np.diff(key) >= 0).all())
    return len(key), int((cnt > 0).sum()), items, int(cnt.max()), sorted_upload


def test_scene_of_65_frames_holds_its_documented_figures():
    md, pm, x0, base = cases.scene65()
    F = cases.SCENE65_FIGURES
    M, pairs, items, _, sorted_upload = _shape(md, 65, cases.BIG65)
    assert (M, pairs, items) == (F["matches"], F["pairs"], [2, 2, 3, 3]) and not sorted_upload
    assert len(base["kp1"]) == 8 * (2080 - 4) and _shape(base, 65, {})[3] == 8       # the base rows alone: every pair one work item
    n64, n32, in_big, nearest, steps = _figures(md, pm, x0, cases.BIG65)
    assert n64 == n32 == F["valid"] and in_big == F["valid_big"], (n64, n32, in_big)
    assert 9.6e-5 < nearest < 9.8e-5, nearest                                        # 9.7e-4 from the threshold of 10
    assert steps == (F["steps"], F["steps"])
    assert oracle_guide(x0, md, cases.GUIDE_CFG)[1] == oracle_guide(x0, md, cases.GUIDE_CFG, torch.float32)[1] == F["guide_steps"]


def test_scene_of_33_frames_was_chosen_from_the_oracle_alone():
    md, pm, x0 = cases.scene33()
    F = cases.SCENE33_FIGURES
    M, pairs, items, _, sorted_upload = _shape(md, 33, cases.BIG33)
    assert (M, pairs, items) == (F["matches"], F["pairs"], [2, 3]) and not sorted_upload
    n64, n32, in_big, nearest, steps = _figures(md, pm, x0, cases.BIG33)
    assert n64 == n32 == F["valid"] and in_big == F["valid_big"], (n64, n32, in_big)
    assert nearest > 1e-4 and abs(nearest - F["nearest_rel"]) < 1e-6, nearest      # no value within the contract band of the threshold
    assert steps == (F["steps"], F["steps"])


# ------------------------------------------------------------------------------------------------ 40 .. 256 frames
@pytest.mark.parametrize("name", list(cases.LONG_SCENES))
def test_long_scene_holds_its_documented_figures(name):
    N, _, ordered, big, _ = cases.LONG_SCENES[name]
    F = cases.LONG_FIGURES[name]
    md, pm, x0 = cases.long_scene(name)
    assert cases.SEEDS[name] == F["seed"] >= cases.SEED_START[name] and int(md["img_shape"][0]) == N
    M, pairs, items, _, sorted_upload = _shape(md, N, big)
    assert (M, pairs, items) == (F["matches"], F["pairs"], F["items"]) and not sorted_upload
    assert pairs == (N * (N - 1) if ordered else N * (N - 1) // 2)
    for pair, c in big.items():
        rows = cases.pair_rows(md, pair)
        assert len(rows) == c and rows[-1] - rows[0] > M // 2, (pair, rows[0], rows[-1])      # scattered over the upload ...
        assert int((np.diff(rows) == 1).sum()) < c // 8, pair                                  # ... and nowhere a run to speak of
        assert [len(r) for r in cases.item_rows(md, pair)] == [c // -(-c // 512) + (k < c % -(-c // 512)) for k in range(-(-c // 512))]
    n64, _, _ = oracle_loss_grad(x0, pm)
    n32, _, _ = oracle_loss_grad(x0, pm, torch.float32)
    with one_thread():
        s, _ = O.compute_sampson_distance(_x(x0, torch.float64), pm, sampson_max=float("inf"))
    in_big = tuple(int((s[cases.pair_rows(md, p)] < 10).sum()) for p in sorted(big))
    nearest = float((s - 10).abs().min()) / 10
    assert n64 == n32 == F["valid"] and in_big == F["valid_big"], (n64, n32, in_big)
    assert nearest > 1e-4 and abs(nearest - F["nearest_rel"]) < 1e-6, nearest
    assert oracle_optimize(x0, pm, iter_num=3)[1] == oracle_optimize(x0, pm, torch.float32, iter_num=3)[1] == F["steps"] == 6
    if name in cases.GUIDED:
        assert oracle_guide(x0, md, cases.GUIDE_CFG)[1] == oracle_guide(x0, md, cases.GUIDE_CFG, torch.float32)[1] == F["guide_steps"]


def test_big_pairs_sit_in_the_documented_rounds_and_workgroups():
    """rank -> (round, workgroup) at 256 workgroups of 8 waves: p = wg*8 + (s&7) + (s>>3)*2048"""
    where = lambda r: (r // 2048, (r % 2048) // 8)
    r129, r256 = sorted(cases.RANKS129), sorted(cases.RANKS256)
    assert [where(r) for r in r129] == [(0, 7), (1, 125), (2, 255), (3, 107), (4, 7)]         # every round; one workgroup twice
    assert [where(r) for r in r256] == [(0, 0), (9, 97), (15, 239)]
    assert cases.pair_of(r129[-1], 129) == (127, 128) and cases.RANKS129[r129[-1]] == 2049 and r129[-1] == 129 * 128 // 2 - 1
    assert cases.pair_of(r256[-1], 256) == (254, 255) and cases.RANKS256[r256[-1]] == 1537 and r256[-1] == 256 * 255 // 2 - 1
    for N, ranks in ((129, r129), (256, r256)):
        assert all(cases.rank_of(*cases.pair_of(r, N), N) == r for r in ranks)
    assert sorted(cases.RANKS129.values()) == [513, 1024, 1025, 1536, 2049] and sorted(cases.RANKS256.values()) == [600, 1100, 1537]
    assert (99, 98) not in cases.BIG100 and cases.BIG100[(7, 50)] != cases.BIG100[(50, 7)]


@functools.lru_cache(maxsize=None)
def _full_gradient(name):
    """(fp64 gradient at the start point, the bound check_loss_grad applies to it per column group)"""
    _, pm, x0 = cases.long_scene(name)
    g64 = oracle_loss_grad(x0, pm)[2]
    g32 = oracle_loss_grad(x0, pm, torch.float32)[2]
    return g64, bounds(grad_group_errs(g32, g64), K_GRAD, FLOOR_GRAD)


def _visible(name, md_changed, what):
    g64, bnd = _full_gradient(name)
    e = grad_group_errs(oracle_loss_grad(cases.long_scene(name)[2], cases._pm(md_changed))[2], g64)
    ratio = max(e[g] / bnd[g] for g in bnd)
    print(f"{name} {what}: gradient moves by {ratio:.0f} x the bound")
    assert ratio > 10, (name, what, e, bnd)


@pytest.mark.parametrize("name", list(cases.LONG_SCENES))
def test_the_checks_can_see_every_item_of_every_big_pair(name):
    md = cases.long_scene(name)[0]
    for pair in sorted(cases.LONG_SCENES[name][3]):
        for k, rows in enumerate(cases.item_rows(md, pair)):
            _visible(name, cases.without_rows(md, rows), f"pair {pair} without item {k} ({len(rows)} matches)")


def test_the_checks_can_see_the_two_orders_of_a_pair_swapped():
    md = cases.long_scene("scene100_both")[0]
    a, b = cases.pair_rows(md, (7, 50)), cases.pair_rows(md, (50, 7))
    swapped = dict(md, i12=md["i12"].copy())
    swapped["i12"][a], swapped["i12"][b] = (50, 7), (7, 50)
    _visible("scene100_both", swapped, "row sets of (7, 50) and (50, 7) swapped")


def test_option_constant_is_the_headers():
    text = open(os.path.join(ROOT, "include", "pd_engine.h")).read()
    m = re.search(r"#define PD_OPT_GGS_LONG_PAIR_ITEMS (\d+)", text)
    assert m and int(m.group(1)) == _lib.PD_OPT_GGS_LONG_PAIR_ITEMS == 8
