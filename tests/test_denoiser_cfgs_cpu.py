"""CPU: the drop-in Denoiser / TransformerEncoderWrapper accept the configuration family of the shape-generic denoiser path
(include/pd_engine.h, pd_weights) with the reference's parameter names, shapes and seeded weights, refuse everything outside it with a
ValueError that names the limit, and the new pd_weights.reserved flags of the header match posediffusion_amd._lib."""
import os
import re

import pytest
import torch
import torch.nn as nn

from denoiser_cfgs import CONFIGS, EDGE_CFGS, GOLDEN_CFGS, Cfg, build_dropin
from posediffusion_amd import _lib, synth
from posediffusion_amd.compat import AttrDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ODD = Cfg(160, 5, 333, 3, 77, 45, True, True)                # head dim 32, odd FF / z / hidden widths
ALL = list(dict.fromkeys(CONFIGS + GOLDEN_CFGS + [ODD] + EDGE_CFGS))


def _reference_layout(cfg: Cfg):
    """nn.TransformerEncoder + Linear / MLP built the reference's way (models/denoiser.py:22-98, :101-163), in its construction order."""
    from posediffusion_amd import synth as S
    models = S._dropin()
    torch.manual_seed(123)
    m = nn.Module()
    m.time_embed = models.denoiser.TimeStepEmbedding()
    m.pose_embed = models.denoiser.PoseEmbedding(target_dim=9)
    m._first = nn.Linear(m.time_embed.out_dim + m.pose_embed.out_dim + cfg.z + int(cfg.pivot), cfg.d)
    layer = nn.TransformerEncoderLayer(d_model=cfg.d, nhead=cfg.heads, dim_feedforward=cfg.ff, dropout=0.1, batch_first=True,
                                       norm_first=cfg.norm_first)
    m._trunk = nn.TransformerEncoder(layer, cfg.layers)
    m._last = nn.Sequential(nn.Linear(cfg.d, cfg.hidden), nn.LayerNorm(cfg.hidden), nn.ReLU(inplace=True), nn.Linear(cfg.hidden, 9))
    return m


@pytest.mark.parametrize("cfg", ALL, ids=[c.name for c in ALL])
def test_dropin_constructs_with_reference_names_and_shapes(cfg):
    den = build_dropin(cfg, seed=3)
    mine = {k: tuple(v.shape) for k, v in den.state_dict().items()}
    ref = {k: tuple(v.shape) for k, v in _reference_layout(cfg).state_dict().items()}
    assert list(mine) == list(ref)
    assert mine == ref
    assert den._trunk.layers[0].norm_first == cfg.norm_first and den.pivot_cam_onehot == cfg.pivot
    assert den._first.in_features == 317 + cfg.z + int(cfg.pivot)


def test_same_seed_same_weights_and_strict_load():
    cfg = ODD
    a, b = build_dropin(cfg, seed=11), build_dropin(cfg, seed=11)
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)
    c = build_dropin(cfg, seed=12)
    c.load_state_dict(a.state_dict(), strict=True)
    assert all(torch.equal(c.state_dict()[k], v) for k, v in a.state_dict().items())


def test_engine_z_dim_counts_the_pivot_only_when_present():
    # PoseEngine derives z_dim from _first's width (engine.py): 317 + z + pivot
    for cfg in (GOLDEN_CFGS[0], GOLDEN_CFGS[1]):
        den = build_dropin(cfg, seed=1)
        assert den._first.weight.shape[1] - (9 * 21 + 128 + int(cfg.pivot)) == cfg.z


BAD_TRUNK = [
    (dict(d_model=100), "multiple of 32"),
    (dict(d_model=2080), "multiple of 32"),
    (dict(d_model=16, nhead=2), "multiple of 32"),
    (dict(d_model=256, nhead=3), "nhead must divide"),
    (dict(d_model=256, nhead=64), r"head dim .* \[8, 256\]"),        # head dim 4
    (dict(d_model=1024, nhead=2), r"head dim .* \[8, 256\]"),        # head dim 512
    (dict(d_model=96, nhead=16), r"head dim .* multiple of 4"),      # head dim 6
    (dict(dim_feedforward=8193), r"dim_feedforward .* \[1, 8192\]"),
    (dict(dim_feedforward=0), r"dim_feedforward .* \[1, 8192\]"),
    (dict(num_encoder_layers=17), r"num_encoder_layers .* \[1, 16\]"),
    (dict(num_encoder_layers=0), r"num_encoder_layers .* \[1, 16\]"),
    (dict(batch_first=False), "batch_first"),
]


@pytest.mark.parametrize("over,msg", BAD_TRUNK, ids=[str(o) for o, _ in BAD_TRUNK])
def test_out_of_family_trunk_raises(over, msg):
    models = synth._dropin()
    kw = dict(d_model=256, nhead=8, num_encoder_layers=2, dim_feedforward=512, dropout=0.1, norm_first=False, batch_first=True)
    kw.update(over)
    with pytest.raises(ValueError, match=msg):
        models.TransformerEncoderWrapper(**kw)


@pytest.mark.parametrize("over,msg", [(dict(target_dim=7), "target_dim=9"), (dict(z_dim=0), r"z_dim .* \[1, 4096\]"),
                                      (dict(z_dim=4097), r"z_dim .* \[1, 4096\]"), (dict(mlp_hidden_dim=1025), r"mlp_hidden_dim .* \[1, 1024\]"),
                                      (dict(mlp_hidden_dim=0), r"mlp_hidden_dim .* \[1, 1024\]")])
def test_out_of_family_denoiser_raises(over, msg):
    models = synth._dropin()
    tr = AttrDict({"_target_": "models.TransformerEncoderWrapper", "d_model": 128, "nhead": 4, "dim_feedforward": 256,
                   "num_encoder_layers": 1, "dropout": 0.1, "batch_first": True, "norm_first": True})
    with pytest.raises(ValueError, match=msg):
        models.Denoiser(TRANSFORMER=tr, **over)


def test_header_flags_match_lib():
    src = open(os.path.join(ROOT, "include", "pd_engine.h")).read()
    for name in ("PD_WEIGHTS_PRED_X0", "PD_WEIGHTS_POST_NORM", "PD_WEIGHTS_NO_PIVOT", "PD_WEIGHTS_GENERIC"):
        m = re.search(rf"#define {name} (\d+)", src)
        assert m, name
        assert int(m.group(1)) == getattr(_lib, name), name
    assert len({_lib.PD_WEIGHTS_PRED_X0, _lib.PD_WEIGHTS_POST_NORM, _lib.PD_WEIGHTS_NO_PIVOT, _lib.PD_WEIGHTS_GENERIC}) == 4
