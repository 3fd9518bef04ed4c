"""No GPU: the C-ABI of the backbone trainer (include/pd_engine_vit_train.h) -- declared in the extension header, exported by the built
library, bound in posediffusion_amd._lib (VIT_TRAIN_SIGNATURES; the other signature tables are pinned by their own tests) -- and the
host-side rules of the drop-in opt-in that need no device."""
import ctypes as C
import os
import re

import torch

from posediffusion_amd import _lib, synth
from posediffusion_amd.vit_train import param_names, scaled_size, shape_from_module, token_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "pd_engine_vit_train.h")) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


def test_header_and_vit_train_signatures_list_the_same_functions():
    hdr = _header()
    assert set(re.findall(r"\b(pd_\w+)\s*\(", hdr)) == set(_lib.VIT_TRAIN_SIGNATURES)
    assert not set(_lib.VIT_TRAIN_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.TRAIN_SIGNATURES))
    for name, (_, args) in _lib.VIT_TRAIN_SIGNATURES.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == len(args), name
    assert int(re.search(r"#define PD_VIT_TRAIN_MAX_TOKENS (\d+)", hdr).group(1)) == _lib.PD_VIT_TRAIN_MAX_TOKENS
    assert int(re.search(r"#define PD_VIT_TRAIN_MAX_SCALES (\d+)", hdr).group(1)) == _lib.PD_VIT_TRAIN_MAX_SCALES


def test_grad_structs_mirror_the_weight_structs():
    assert [n for n, _ in _lib.pd_vit_layer_grads._fields_] == [n for n, _ in _lib.pd_vit_layer_weights._fields_]
    weights = [n for n, _ in _lib.pd_vit_weights._fields_]
    grads = [n for n, _ in _lib.pd_vit_weight_grads._fields_]
    assert grads == weights[weights.index("patch_w"):]
    hdr = _header()
    m = re.search(r"typedef struct pd_vit_layer_grads \{(.*?)\}", hdr, flags=re.S)
    assert re.findall(r"\*(\w+)", m.group(1)) == [n for n, _ in _lib.pd_vit_layer_grads._fields_]
    m = re.search(r"typedef struct pd_vit_weight_grads \{(.*?)pd_vit_layer_grads layers\[(\d+)\]", hdr, flags=re.S)
    assert re.findall(r"\*(\w+)", m.group(1)) == grads[:6] and int(m.group(2)) == 16
    assert C.sizeof(_lib.pd_vit_layer_grads) == C.sizeof(_lib.pd_vit_layer_weights) == 8 * 12
    assert C.sizeof(_lib.pd_vit_weight_grads) == 8 * (6 + 12 * 16)
    assert C.sizeof(_lib.pd_vit_weights) == 8 * 4 + C.sizeof(_lib.pd_vit_weight_grads)


def test_symbols_are_exported_and_refuse_null_handles():
    assert os.path.isfile(_lib.LIB_PATH), "run `python -c 'import __graft_entry__ as g; g.build()'` first"
    lib = _lib.load()
    for name, (_, args) in _lib.VIT_TRAIN_SIGNATURES.items():
        assert getattr(lib, name).argtypes == args
    assert lib.pd_vit_train_forward(None, None, None, 1, 16, 16, None, 1, None, None, None) == -1
    assert "pd_vit_train_forward" in _lib.last_error()
    assert lib.pd_vit_train_backward(None, None, None, None, None) == -1
    assert "pd_vit_train_backward" in _lib.last_error()
    out = C.c_void_p(None)
    assert lib.pd_vit_trainer_create(None, 1, 2, 1, C.byref(out)) == -1 and not out.value
    w = _lib.pd_vit_weights()
    w.dim, w.depth, w.num_heads, w.mlp_hidden, w.patch_size, w.pos_grid = 384, 12, 6, 1536, 16, 14
    assert lib.pd_vit_trainer_create(C.byref(w), 0, 2, 1, C.byref(out)) == -1 and "max_images" in _lib.last_error()
    w.depth = 17                                                        # outside pd_vit_weights' family: refused before anything is allocated
    assert lib.pd_vit_trainer_create(C.byref(w), 1, 2, 1, C.byref(out)) == -2 and "depth" in _lib.last_error() and not out.value
    w.depth, w.dim = 12, 768
    assert lib.pd_vit_trainer_create(C.byref(w), 1, 2, 1, C.byref(out)) == -2 and "dim" in _lib.last_error() and not out.value
    lib.pd_vit_trainer_destroy(None)


def test_param_names_are_the_backbones_parameters_and_rows_follow_the_floor_rule():
    models = synth._dropin()
    ext = models.MultiScaleImageFeatureExtractor()
    assert sorted(param_names(12)) == sorted(n for n, _ in ext._net.named_parameters())          # (pd_vit_weights' order, not the module's)
    assert shape_from_module(ext._net) == {"dim": 384, "depth": 12, "num_heads": 6, "mlp_hidden": 1536, "patch_size": 16, "pos_grid": 14}
    assert scaled_size(96, 96, 1 / 3) == (32, 32) and scaled_size(224, 224, 1 / 3) == (74, 74) and scaled_size(224, 230, 1) == (224, 230)
    assert token_rows(224, 224, (1, 1 / 2, 1 / 3)) == 197 + 50 + 17 and token_rows(96, 96, (1, 1 / 2, 1 / 3)) == 37 + 10 + 5
    assert token_rows(240, 272, (1,)) == 256


def test_engine_grad_defaults_off_and_needs_both_opt_ins():
    models = synth._dropin()
    ext = models.MultiScaleImageFeatureExtractor()
    assert ext.engine_grad is False and not ext._wants_engine_grad()
    ext.engine_grad = True
    assert ext._wants_engine_grad()
    with torch.no_grad():
        assert not ext._wants_engine_grad()
    frozen = models.MultiScaleImageFeatureExtractor(freeze=True)
    frozen.engine_grad = True
    assert not frozen._wants_engine_grad()
    for p in ext.parameters():
        p.requires_grad_(False)
    assert not ext._wants_engine_grad()
    assert "engine_grad" not in ext.state_dict()                        # an attribute, not a buffer: checkpoints are unchanged
