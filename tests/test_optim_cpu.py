"""No GPU: the optimiser step's C-ABI (include/pd_engine_optim.h, posediffusion_amd._lib.OPTIM_SIGNATURES, the built library), the bounds of
tests/optim_checks.py met by the fp32 emulation of the kernel's formula on every input set the GPU tests use, EngineAdamW's host-side rules,
and the register budget of posediffusion_amd/csrc/pd_optim.hip."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import optim_checks as OC
from posediffusion_amd import _lib, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "posediffusion_amd", "csrc")


def _header():
    with open(os.path.join(ROOT, "include", "pd_engine_optim.h")) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


def test_header_and_optim_signatures_list_the_same_functions():
    hdr = _header()
    assert set(re.findall(r"\b(pd_\w+)\s*\(", hdr)) == set(_lib.OPTIM_SIGNATURES)
    others = set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.TRAIN_SIGNATURES) | set(_lib.VIT_TRAIN_SIGNATURES)
    assert not set(_lib.OPTIM_SIGNATURES) & others
    for name, (_, args) in _lib.OPTIM_SIGNATURES.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == len(args), name
    assert int(re.search(r"#define PD_OPTIM_CHUNK (\d+)", hdr).group(1)) == _lib.PD_OPTIM_CHUNK == optim.CHUNK == OC.CHUNK
    assert optim.CHUNK % 4 == 0                                        # a chunk keeps its tensor's alignment
    m = re.search(r"typedef struct pd_optim_tensor \{(.*?)\}", hdr, flags=re.S)
    assert re.findall(r"\b(\w+)\s*[,;]", m.group(1)) == [n for n, _ in _lib.pd_optim_tensor._fields_]
    assert C.sizeof(_lib.pd_optim_tensor) == 48 and C.sizeof(_lib.pd_optim_group) == 40


def test_symbols_are_exported_and_refuse_null_handles():
    assert os.path.isfile(_lib.LIB_PATH), "run `python -c 'import __graft_entry__ as g; g.build()'` first"
    lib = _lib.load()
    for name, (_, args) in _lib.OPTIM_SIGNATURES.items():
        assert getattr(lib, name).argtypes == args
    calls = {"pd_optim_grad_norm": (None, None, 0, None, None),
             "pd_optim_clip_grad_norm": (None, None, 0, 1.0, None, None),
             "pd_optim_adamw_step": (None, None, 0, None, 0, 1.0, None, None),
             "pd_optimizer_create": (1, 1, None)}
    assert set(calls) | {"pd_optimizer_destroy"} == set(_lib.OPTIM_SIGNATURES)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -1, name
        assert name in _lib.last_error(), (name, _lib.last_error())
    out = C.c_void_p(None)
    assert lib.pd_optimizer_create(0, 1, C.byref(out)) == -1 and not out.value and "max_tensors" in _lib.last_error()
    lib.pd_optimizer_destroy(None)


@pytest.mark.parametrize("case", OC.all_cases(), ids=lambda c: c["name"])
def test_the_fp32_emulation_stays_inside_every_bound(case):
    p, m, v, norm = OC.emulate_case(case)
    w = OC.check_case(case, p, m, v, norm)
    assert all(x <= 1.0 for x in w.values()), w


def test_the_bounds_are_not_vacuous():
    """an update computed with a gradient one part in 2^18 off -- far more than any rounding sequence of the formula -- leaves them"""
    case = OC.make_case("base", seed=1)
    off = dict(case, g=[g * np.float32(1.0 + 2.0 ** -18) for g in case["g"]])
    p, m, v, _ = OC.emulate_case(off)
    w = OC.check_case(case, p, m, v)
    assert w["m"] > 1.0 and w["v"] > 1.0, w
    case = OC.make_case("step1000", steps=1000, seed=2)
    p, m, v, _ = OC.emulate_case(case)
    p = [x + 4 * np.spacing(np.abs(x)) for x in p]
    assert OC.check_case(case, p, m, v)["p"] > 1.0


def test_the_emulated_norm_and_coefficient():
    g = OC.norm_values(OC.sizes(), seed=3)
    n64 = OC.norm64(g)
    assert np.isfinite(n64) and abs(float(OC.norm32(g)) - n64) <= OC.norm_bound(n64)
    assert OC.coef32(np.float32(0.5), 1.0) == 1.0 and OC.coef32(np.float32(4.0), 1.0) < 0.25001
    assert np.isnan(OC.coef32(np.float32(np.nan), 1.0)) and OC.coef32(np.float32(np.inf), 1.0) == 0.0


def _params():
    ps = [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(7))]
    for p in ps:
        p.grad = torch.ones_like(p)
    return ps


def test_engine_adamw_keeps_torchs_state_dict_and_group_keys():
    kw = dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.1)
    ours, theirs = optim.EngineAdamW(_params(), max_grad_norm=1.0, **kw), torch.optim.AdamW(_params(), **kw)
    assert list(ours.param_groups[0]) == list(theirs.param_groups[0])
    a, b = ours.state_dict(), theirs.state_dict()
    assert a.keys() == b.keys() and a["state"] == b["state"] == {}
    assert a["param_groups"] == b["param_groups"]
    theirs.step()                                                       # a PyTorch checkpoint loads: same state keys, step stays a CPU tensor
    ours.load_state_dict(theirs.state_dict())
    st = ours.state[ours.param_groups[0]["params"][0]]
    assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and st["step"].device.type == "cpu" and float(st["step"]) == 1.0
    import posediffusion_amd
    assert posediffusion_amd.EngineAdamW is optim.EngineAdamW and posediffusion_amd.clip_grad_norm_ is optim.clip_grad_norm_


@pytest.mark.parametrize("key", ["amsgrad", "maximize", "capturable", "differentiable"])
def test_engine_adamw_refuses_torchs_variants(key):
    with pytest.raises(ValueError, match=f"{key}=True is not supported"):
        optim.EngineAdamW(_params(), **{key: True})
    opt = optim.EngineAdamW(_params())
    opt.param_groups[0][key] = True                                     # set on a live group: refused at the step, before the device check
    with pytest.raises(ValueError, match=f"{key}=True is not supported"):
        opt.step()


@pytest.mark.parametrize("key", ["foreach", "fused"])
def test_engine_adamw_refuses_an_implementation_choice(key):
    for value in (True, False):
        with pytest.raises(ValueError, match=f"{key}={value} selects one of PyTorch's own implementations"):
            optim.EngineAdamW(_params(), **{key: value})


def test_engine_adamw_refuses_bad_hyperparameters_like_torch():
    for kw, msg in ((dict(lr=-1.0), "Invalid learning rate"), (dict(eps=-1.0), "Invalid epsilon"), (dict(betas=(1.0, 0.9)), "beta parameter at index 0"),
                    (dict(betas=(0.9, -0.1)), "beta parameter at index 1"), (dict(weight_decay=-1.0), "Invalid weight_decay"),
                    (dict(max_grad_norm=0.0), "Invalid max_grad_norm")):
        with pytest.raises(ValueError, match=msg):
            optim.EngineAdamW(_params(), **kw)


@pytest.mark.skipif(torch.cuda.is_available(), reason="the rule of a machine without a GPU")
def test_without_a_gpu_the_object_builds_and_the_step_raises():
    opt = optim.EngineAdamW(_params(), max_grad_norm=1.0)                # construction needs no device
    with pytest.raises(RuntimeError, match="AMD GPU"):
        opt.step()
    with pytest.raises(RuntimeError, match="AMD GPU"):
        optim.clip_grad_norm_(_params(), 1.0)
    assert opt.state_dict()["state"] == {}                               # nothing was touched


def test_a_step_under_stream_capture_is_refused_before_the_device_is_touched(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="EngineAdamW.step under stream capture"):
        optim.EngineAdamW(_params()).step()
    with pytest.raises(RuntimeError, match="clip_grad_norm_ under stream capture"):
        optim.clip_grad_norm_(_params(), 1.0)


def _kernel_resources(src, tmp_path, contract):
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", f"-ffp-contract={contract}", "-Rpass-analysis=kernel-resource-usage",
                          "-c", os.path.join(CSRC, src), "-o", str(tmp_path / (src + ".o"))], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+?): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split("[")[0].strip()] = int(m.group(2))
    return kernels


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_optimiser_kernels_do_not_spill_and_the_big_two_run_at_occupancy_8(tmp_path):
    with open(os.path.join(CSRC, "Makefile")) as fh:                     # the unit is built with contraction per source expression
        assert re.search(r"build/pd_optim\.o: CXXFLAGS := .*-ffp-contract=on", fh.read())
    kernels = _kernel_resources("pd_optim.hip", tmp_path, "on")
    stems = ("pd_opt_set_entries_kernel", "pd_opt_set_hypers_kernel", "pd_opt_sqnorm_kernel", "pd_opt_finish_norm_kernel",
             "pd_opt_adamw_kernel", "pd_opt_scale_kernel")
    for stem in stems:
        assert len([k for k in kernels if stem in k]) == 1, (stem, sorted(kernels))
    assert len(kernels) == len(stems), sorted(kernels)
    for name, r in kernels.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (name, r)
    for stem in ("pd_opt_sqnorm_kernel", "pd_opt_adamw_kernel"):
        r = next(v for k, v in kernels.items() if stem in k)
        assert r["Occupancy"] == 8, (stem, r)
