"""The scenes of the tests of PD_OPT_GGS_LONG_PAIR_ITEMS (frame pairs of more than 512 matches above 64 frames): a plain module shared by
tests/test_ggs_pair_items_cpu.py (which pins the oracle-side figures below, so the scenes cannot drift) and tests/test_gpu_ggs_pair_items.py.

scene65(): 65 frames.  Cameras and base matches are those of test_gpu_ggs_long._scene(65, 8) (make_cameras(65, seed=865), 8 matches for
each of the 2 080 pairs i < j, seed 865).  The rows of four pairs are replaced by larger sets, BIG65 = {(0, 1): 513, (3, 40): 1024,
(10, 64): 1025, (63, 64): 1500}: pair n (sorted order) of c matches gets make_matches(enc[[i, j]], per_pair=c, seed=7000 + n) with i12
rewritten to (i, j).  The four big pairs stand FIRST in kp1 / kp2 / i12, the remaining base rows behind them: the upload is not pair-sorted.
20 670 matches in 2 080 pairs; work items per big pair 2, 2, 3, 3 (1 025 cuts into 342 + 342 + 341: the balanced cut and an interleave
group that is not full).  Start point perturb_pose(enc, seed=875).  Figures of the oracle alone (CPU, fp64 and fp32 alike):
  * 11 702 valid matches at the start point; 125, 696, 699 and 883 of them in the four big pairs;
  * GGS_optimize(iter_num=3) steps 6 of 6 iterations; the shortened guide (iter_num=2) steps [4, 2, 2, 2, 4];
  * the Sampson value nearest the threshold of 10 is 9.7e-4 away (a match of the base scene, which the 65-frame tests of
    test_gpu_ggs_long.py already carry).

scene33(): 33 frames under PD_GGS_CFG_LONG_FRAMES, 528 pairs: the cameras and base matches of make_cameras(33, seed=SEED33) /
make_matches(per_pair=16, seed=SEED33), with BIG33 = {(0, 1): 600, (5, 32): 1100} replaced the same way (seeds 7100 + n) and standing
first.  10 116 matches; 2 and 3 work items.  Start point perturb_pose(enc, seed=SEED33 + 10).  SEED33 is chosen from the oracle alone, as
test_gpu_ggs_long.test_both_orders_of_every_pair_at_100_frames documents: the first seed from 833 upward at which the fp64 and fp32
oracles count the same valid matches and no Sampson value lies within 1e-4 relative of the threshold -- 833 itself: 5 762 valid matches
in both precisions (88 and 988 of them in the two big pairs), the nearest Sampson value 2.07e-4 relative from the threshold, and
GGS_optimize(iter_num=3) steps 6 of 6 in both (SCENE33_FIGURES, asserted by the CPU test).
"""
import functools

import numpy as np

from oracle import pd_oracle as O
from posediffusion_amd import synth

H = W = 224
BIG65 = {(0, 1): 513, (3, 40): 1024, (10, 64): 1025, (63, 64): 1500}
BIG33 = {(0, 1): 600, (5, 32): 1100}
SEED33 = 833
# figures of the oracle, fp64 == fp32: valid matches at the start point (and inside the big pairs), iterations stepped by
# GGS_optimize(iter_num=3) / the shortened guide; scene33: the distance of the nearest Sampson value from the threshold, relative to it
SCENE33_FIGURES = {"valid": 5762, "valid_big": (88, 988), "nearest_rel": 2.07e-4, "steps": 6, "matches": 10116, "pairs": 528}
SCENE65_FIGURES = {"valid": 11702, "valid_big": (125, 696, 699, 883), "steps": 6, "guide_steps": [4, 2, 2, 2, 4], "matches": 20670, "pairs": 2080}
GUIDE_CFG = dict(synth.GGS_CFG, iter_num=2)


def _with_big_pairs(enc, md, big, seed0):
    """(matches_dict with the rows of the pairs of `big` replaced and moved to the front, matches_dict of the remaining base rows)"""
    i12 = md["i12"]
    keep = np.ones(len(i12), dtype=bool)
    kp1, kp2, idx = [], [], []
    for n, ((i, j), c) in enumerate(sorted(big.items())):
        keep &= ~((i12[:, 0] == i) & (i12[:, 1] == j))
        m = synth.make_matches(enc[[i, j]], H, W, per_pair=c, seed=seed0 + n)
        assert len(m["kp1"]) == c
        kp1.append(m["kp1"])
        kp2.append(m["kp2"])
        idx.append(np.tile(np.array([[i, j]], dtype=np.int64), (c, 1)))
    base = {"kp1": md["kp1"][keep], "kp2": md["kp2"][keep], "i12": i12[keep], "img_shape": md["img_shape"]}
    full = {"kp1": np.concatenate(kp1 + [base["kp1"]]), "kp2": np.concatenate(kp2 + [base["kp2"]]),
            "i12": np.concatenate(idx + [base["i12"]]), "img_shape": md["img_shape"]}
    return full, base


def _pm(md):
    return O.prepare_matches(md["kp1"], md["kp2"], md["i12"], md["img_shape"])


@functools.lru_cache(maxsize=None)
def scene65():
    """(matches_dict, prepared matches, start pose [1, 65, 9], matches_dict of the base rows alone: every pair one work item)"""
    enc = synth.make_cameras(65, seed=865)
    md = synth.make_matches(enc, H, W, per_pair=8, seed=865)
    full, base = _with_big_pairs(enc, md, BIG65, 7000)
    return full, _pm(full), synth.perturb_pose(enc, seed=875), base


@functools.lru_cache(maxsize=None)
def scene33(seed=SEED33):
    """(matches_dict, prepared matches, start pose [1, 33, 9])"""
    enc = synth.make_cameras(33, seed=seed)
    md = synth.make_matches(enc, H, W, per_pair=16, seed=seed)
    full, _ = _with_big_pairs(enc, md, BIG33, 7100)
    return full, _pm(full), synth.perturb_pose(enc, seed=seed + 10)


@functools.lru_cache(maxsize=None)
def scene40():
    """the single-item 40-frame scene of test_gpu_ggs_long._scene(40, 16): (matches_dict, prepared matches, start pose)"""
    enc = synth.make_cameras(40, seed=840)
    md = synth.make_matches(enc, H, W, per_pair=16, seed=840)
    return md, _pm(md), synth.perturb_pose(enc, seed=850)


def big_pair_rows(md, big):
    """row slices of the big pairs of a scene built by _with_big_pairs (they stand first, in sorted pair order)"""
    out, at = [], 0
    for (_, c) in sorted(big.items()):
        out.append(slice(at, at + c))
        at += c
    return out
