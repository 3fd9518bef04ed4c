"""The scenes of the tests of PD_OPT_GGS_LONG_PAIR_ITEMS (frame pairs of more than 512 matches above 64 frames): a plain module shared by
tests/test_ggs_pair_items_cpu.py (which pins the oracle-side figures below, so the scenes cannot drift), tests/test_gpu_ggs_pair_items.py and
tests/test_gpu_ggs_pair_items_long.py.

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

long_scene(name): the scenes of tests/test_gpu_ggs_pair_items_long.py, 40 .. 256 frames (LONG_SCENES).  Cameras make_cameras(N, seed),
base matches make_matches(per_pair, seed), the big pairs replaced by _with_big_pairs (pair n in sorted order: seed 7200 / 7300 / 7400 /
7500 / 7600 + n), then ALL rows shuffled with the fixed permutation default_rng(N): the rows of every big pair are scattered over the
whole upload, and a pair's work items are the balanced cut of its rows in upload order (what a stable sort by pair leaves: item_rows).
The shuffled dict is the one every path gets.  Start point perturb_pose(enc, seed + 10).  `seed` is the first from SEED_START[name]
upward at which, from the oracle alone: fp64 and fp32 count the same valid matches at the start point; no Sampson value lies within 1e-4
relative of the threshold 10; GGS_optimize(iter_num=3) steps 6 of 6 in both precisions; and (scene129, scene100_both, scene70) the
shortened guide steps the same stage counts in both.  Figures in SCENE*_FIGURES, asserted by the CPU test.

  scene129       129 frames, per_pair 2, 8 256 pairs i < j, 22 649 matches, seed 1133 (1129 .. 1132 have a Sampson value 3.0e-5 .. 5.5e-5
                 from the threshold); 15 311 valid, nearest 5.2e-4, guide [4, 2, 2, 2, 4].  Big pairs by RANK in sorted pair order; at the
                 default 256 workgroups (nW = 2 048 waves) round = rank // 2048, workgroup = (rank % 2048) // 8:
                     rank   pair        matches  items                       round  workgroup  valid
                       60   (0, 61)        513   2 (257 + 256)                 0        7       217
                     3048   (26, 72)     1 024   2 (512 + 512: both full)      1      125       735
                     6142   (63, 95)     1 025   3 (342 + 342 + 341)           2      255       923
                     7000   (78, 98)     1 536   3 (3 x 512: every item full)  3      107     1 380
                     8255   (127, 128)   2 049   5 (4 x 410 + 409)             4        7     1 404    the LAST pair of the table
                 (ranks 60 and 8 255: the same workgroup, rounds 0 and 4.  Rank 6 143 = (63, 96), the last of round 2, was measured
                 first: 7 of its 1 025 matches are valid at the start point and removing its second item moves the gradient by 7.5 x the
                 bound only, under the factor 10 the CPU test asks, so its neighbour in the same workgroup and round stands in.)
  scene256       256 frames, per_pair 2, 32 640 pairs, 68 511 matches, seed 1256; 43 760 valid, nearest 1.25e-4.  16 rounds:
                     rank 5 = (0, 6): 600, 2 items, round 0, workgroup 0, 483 valid;  rank 19 209 = (91, 191): 1 100, 3 items (367 + 367 +
                     366), round 9, workgroup 97, 947 valid;  rank 32 639 = (254, 255): 1 537, 4 items (385 + 3 x 384), round 15, workgroup
                     239, 1 240 valid: the last pair.
  scene100_both  100 frames, both orders of every pair, per_pair 2, 9 900 pairs (198 incidence rows per frame), 22 307 matches, seed 1100;
                 14 264 valid, nearest 1.42e-4, guide [4, 2, 2, 2, 4].  (7, 50): 700, 2 items, 485 valid; (50, 7): 1 300, 3 items (434 + 433
                 + 433), 877 valid; (98, 99): 513, 2 items, 3 valid (each item still moves the gradient by more than 60 x the bound);
                 (99, 98) stays a single item of 2 matches.
  scene70        70 frames, per_pair 4, 2 415 pairs, 11 277 matches, seed 1071 (1070: a Sampson value 1.6e-5 from the threshold); 8 006
                 valid, nearest 1.52e-4, guide [4, 2, 2, 2, 4].  (0, 69): 1 025, 3 items, 798 valid; (33, 34): 600, 2 items, 513 valid.
  scene40_big    40 frames, per_pair 8, 780 pairs, 6 932 matches, seed 1040; 3 485 valid, nearest 1.35e-4.  (3, 8): 700, 2 items of 350, 296
                 valid.  (Pair (3, 7) was measured first: 3 of its 700 matches are valid at the start point, none of them in its second
                 item, which no check could then see; (3, 8) is the next pair in sorted order.)
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


# ------------------------------------------------------------------------------------------------ 66 .. 256 frames (docstring above)
def rank_of(i, j, N):
    """rank of the pair (i, j), i < j, among all C(N, 2) pairs in sorted order"""
    return i * N - i * (i + 1) // 2 + (j - i - 1)


def pair_of(rank, N):
    """the pair i < j of that rank"""
    i = 0
    while rank >= N - 1 - i:
        rank -= N - 1 - i
        i += 1
    return i, i + 1 + rank


# rank in sorted pair order -> matches; at 256 workgroups round = rank // 2048, workgroup = (rank % 2048) // 8
RANKS129 = {60: 513, 3048: 1024, 6142: 1025, 7000: 1536, 8255: 2049}
RANKS256 = {5: 600, 19209: 1100, 32639: 1537}
BIG129 = {pair_of(r, 129): c for r, c in RANKS129.items()}
BIG256 = {pair_of(r, 256): c for r, c in RANKS256.items()}
BIG100 = {(7, 50): 700, (50, 7): 1300, (98, 99): 513}
BIG70 = {(0, 69): 1025, (33, 34): 600}
BIG40 = {(3, 8): 700}
#        frames, per_pair, both orders, big pairs, seed of the first big pair
LONG_SCENES = {"scene129": (129, 2, False, BIG129, 7200), "scene256": (256, 2, False, BIG256, 7300),
               "scene100_both": (100, 2, True, BIG100, 7400), "scene70": (70, 4, False, BIG70, 7500),
               "scene40_big": (40, 8, False, BIG40, 7600)}
SEED_START = {"scene129": 1129, "scene256": 1256, "scene100_both": 1100, "scene70": 1070, "scene40_big": 1040}
# the first seed from SEED_START upward that meets the conditions of the docstring, and the oracle's figures at it (fp64 == fp32)
SEEDS = {"scene129": 1133, "scene256": 1256, "scene100_both": 1100, "scene70": 1071, "scene40_big": 1040}
SCENE129_FIGURES = {"seed": 1133, "valid": 15311, "valid_big": (217, 735, 923, 1380, 1404), "nearest_rel": 5.196e-4, "steps": 6,
                    "guide_steps": [4, 2, 2, 2, 4], "matches": 22649, "pairs": 8256, "items": [2, 2, 3, 3, 5]}
SCENE256_FIGURES = {"seed": 1256, "valid": 43760, "valid_big": (483, 947, 1240), "nearest_rel": 1.249e-4, "steps": 6,
                    "matches": 68511, "pairs": 32640, "items": [2, 3, 4]}
SCENE100_BOTH_FIGURES = {"seed": 1100, "valid": 14264, "valid_big": (485, 877, 3), "nearest_rel": 1.424e-4, "steps": 6,
                         "guide_steps": [4, 2, 2, 2, 4], "matches": 22307, "pairs": 9900, "items": [2, 3, 2]}
SCENE70_FIGURES = {"seed": 1071, "valid": 8006, "valid_big": (798, 513), "nearest_rel": 1.516e-4, "steps": 6,
                   "guide_steps": [4, 2, 2, 2, 4], "matches": 11277, "pairs": 2415, "items": [3, 2]}
SCENE40_BIG_FIGURES = {"seed": 1040, "valid": 3485, "valid_big": (296,), "nearest_rel": 1.347e-4, "steps": 6,
                       "matches": 6932, "pairs": 780, "items": [2]}
LONG_FIGURES = {"scene129": SCENE129_FIGURES, "scene256": SCENE256_FIGURES, "scene100_both": SCENE100_BOTH_FIGURES,
                "scene70": SCENE70_FIGURES, "scene40_big": SCENE40_BIG_FIGURES}
GUIDED = ("scene129", "scene100_both", "scene70")


def shuffled(md, seed):
    """the rows of a matches_dict under the fixed permutation default_rng(seed)"""
    perm = np.random.default_rng(seed).permutation(len(md["kp1"]))
    return {"kp1": md["kp1"][perm], "kp2": md["kp2"][perm], "i12": md["i12"][perm], "img_shape": md["img_shape"]}


@functools.lru_cache(maxsize=None)
def long_scene(name, seed=None):
    """(matches_dict with its rows shuffled, prepared matches of that dict, start pose [1, N, 9]) of a scene of LONG_SCENES"""
    N, per_pair, ordered, big, seed0 = LONG_SCENES[name]
    seed = SEEDS[name] if seed is None else seed
    enc = synth.make_cameras(N, seed=seed)
    md = synth.make_matches(enc, H, W, per_pair=per_pair, seed=seed, ordered_pairs=ordered)
    full, _ = _with_big_pairs(enc, md, big, seed0)
    full = shuffled(full, N)
    return full, _pm(full), synth.perturb_pose(enc, seed=seed + 10)


def pair_rows(md, pair):
    """the rows of a frame pair in upload order (the order a stable sort by pair keeps)"""
    return np.nonzero((md["i12"][:, 0] == pair[0]) & (md["i12"][:, 1] == pair[1]))[0]


def item_rows(md, pair):
    """the rows of each work item of a pair: ceil(c / 512) items, the balanced cut (the first c % items of them one match longer)"""
    rows = pair_rows(md, pair)
    n = -(-len(rows) // 512)
    q, r = divmod(len(rows), n)
    cuts = np.cumsum([0] + [q + (k < r) for k in range(n)])
    return [rows[cuts[k]:cuts[k + 1]] for k in range(n)]


def without_rows(md, rows):
    keep = np.ones(len(md["kp1"]), dtype=bool)
    keep[rows] = False
    return {"kp1": md["kp1"][keep], "kp2": md["kp2"][keep], "i12": md["i12"][keep], "img_shape": md["img_shape"]}


def big_pair_rows(md, big):
    """row slices of the big pairs of a scene built by _with_big_pairs (they stand first, in sorted pair order)"""
    out, at = [], 0
    for (_, c) in sorted(big.items()):
        out.append(slice(at, at + c))
        at += c
    return out
