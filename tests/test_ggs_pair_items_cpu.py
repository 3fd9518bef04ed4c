"""CPU: the scenes of tests/ggs_pair_items_cases.py hold what their docstring says -- sizes, work items per big pair, and the oracle-side
figures (valid matches equal in fp64 and fp32, no Sampson value near the threshold, iterations stepped) that make them fit to judge a
kernel by -- and the option's constant is the header's."""
import os
import re

import numpy as np
import torch

import ggs_pair_items_cases as cases
from ggs_checks import _x, one_thread, oracle_guide, oracle_loss_grad, oracle_optimize
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


def test_option_constant_is_the_headers():
    text = open(os.path.join(ROOT, "include", "pd_engine.h")).read()
    m = re.search(r"#define PD_OPT_GGS_LONG_PAIR_ITEMS (\d+)", text)
    assert m and int(m.group(1)) == _lib.PD_OPT_GGS_LONG_PAIR_ITEMS == 8
