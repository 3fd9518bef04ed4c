"""No GPU: the C-ABI of the training branch with gradients (include/pd_engine_train.h) -- declared in the extension header, exported by the
built library, bound in posediffusion_amd._lib (TRAIN_SIGNATURES; the other two signature tables are pinned by their own tests) -- and
the host-side rules of the drop-in opt-in that need no device."""
import ctypes as C
import os
import re

import pytest
import torch

from posediffusion_amd import _lib, synth
from posediffusion_amd.train import param_names, shape_from_modules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "pd_engine_train.h")) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


def test_header_and_train_signatures_list_the_same_functions():
    hdr = _header()
    assert set(re.findall(r"\b(pd_\w+)\s*\(", hdr)) == set(_lib.TRAIN_SIGNATURES)
    assert not set(_lib.TRAIN_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES))
    for name, (_, args) in _lib.TRAIN_SIGNATURES.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == len(args), name


def test_grad_structs_mirror_the_weight_structs():
    assert [n for n, _ in _lib.pd_layer_grads._fields_] == [n for n, _ in _lib.pd_layer_weights._fields_]
    weights = [n for n, _ in _lib.pd_weights._fields_]
    grads = [n for n, _ in _lib.pd_weight_grads._fields_]
    assert grads == weights[weights.index("time_w0"):weights.index("last3_b") + 1]
    m = re.search(r"typedef struct pd_layer_grads \{(.*?)\}", _header(), flags=re.S)
    assert re.findall(r"\*(\w+)", m.group(1)) == [n for n, _ in _lib.pd_layer_grads._fields_]
    assert C.sizeof(_lib.pd_weight_grads) == 8 * (12 + 12 * _lib.PD_MAX_LAYERS)


def test_symbols_are_exported_and_refuse_null_handles():
    assert os.path.isfile(_lib.LIB_PATH), "run `python -c 'import __graft_entry__ as g; g.build()'` first"
    lib = _lib.load()
    for name, (_, args) in _lib.TRAIN_SIGNATURES.items():
        assert getattr(lib, name).argtypes == args
    assert lib.pd_train_forward(None, None, None, None, None, None, 1, 1, 1, None, None, None, None, None) == -1
    assert "pd_train_forward" in _lib.last_error()
    assert lib.pd_train_backward(None, None, None, None, None, None) == -1
    assert lib.pd_train_debug_relu(None, 0, None, 0, None) == -1
    assert lib.pd_trainer_check_async(None) == -1
    out = C.c_void_p(None)
    assert lib.pd_trainer_create(None, None, None, 1, 1, C.byref(out)) == -1 and not out.value
    lib.pd_trainer_destroy(None)


def test_param_names_are_the_denoisers_parameters_and_shape_is_read_off_the_modules():
    diff = synth.make_diffuser(seed=0, num_layers=2)
    assert sorted(param_names(2)) == sorted(n for n, _ in diff.model.named_parameters())      # (pd_weights' order, not the module's)
    s = shape_from_modules(diff.model, diff)
    assert (s["d_model"], s["nhead"], s["dim_ff"], s["num_layers"], s["z_dim"], s["mlp_hidden"]) == (512, 4, 1024, 2, 384, 128)
    assert s["norm_first"] and s["pivot"] and s["objective"] == "pred_noise"


def test_engine_grad_defaults_off_and_refuses_dropout_in_train_mode():
    diff = synth.make_diffuser(seed=0, num_layers=1)
    assert diff.engine_grad is False
    diff.engine_grad = True
    diff.train()
    x = torch.zeros(1, 2, 9)
    with pytest.raises(RuntimeError, match=r"dropout.*TRANSFORMER\.dropout = 0 or call \.eval\(\)"):
        diff.p_losses(x, torch.tensor([3]), z=torch.zeros(1, 2, 384), noise=x)
    for m in diff.model.modules():                       # dropout 0 under .train() is engine training: the rule lets it through to the device check
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    for layer in diff.model._trunk.layers:
        layer.self_attn.dropout = 0.0
    with pytest.raises(RuntimeError, match="AMD GPU"):
        diff.p_losses(x, torch.tensor([3]), z=torch.zeros(1, 2, 384), noise=x)
