"""No GPU: the C-ABI of frame counts per sequence (pd_engine_set_frame_counts) -- declared in include/pd_engine.h, exported by the built
library, bound in posediffusion_amd._lib with the header's signature, and refusing a NULL engine with PD_ERR_INVALID_ARG."""
import ctypes as C
import os
import re

import pytest

from posediffusion_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "pd_engine_set_frame_counts"


def _header():
    with open(os.path.join(ROOT, "include", "pd_engine.h")) as fh:
        return fh.read()


def test_symbol_is_declared_in_the_header_with_the_documented_signature():
    m = re.search(r"int\s+" + NAME + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, "pd_engine_set_frame_counts is not declared in include/pd_engine.h"
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert args == ["pd_engine *eng", "int B", "const int32_t *n_frames", "void *stream"], args


def test_header_names_the_callers_job_and_the_calls_that_honour_the_counts():
    h = re.sub(r"\s+", " ", _header().replace("\n *", " "))
    assert "GROUPING SEQUENCES INTO LAUNCHES THE PLAN ACCEPTS IS THE CALLER'S JOB" in h
    for call in ("pd_denoise_step", "pd_p_mean", "pd_p_finish", "pd_ggs_guide", "pd_sample_phase", "pd_debug_ggs_plan"):
        assert call in h


def test_symbol_is_bound_in_lib_with_four_arguments():
    res, args = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == 4
    assert args[0] is C.c_void_p and args[1] is C.c_int and args[2] == C.POINTER(C.c_int32) and args[3] is C.c_void_p


@pytest.fixture(scope="module")
def lib():
    assert os.path.isfile(_lib.LIB_PATH), "run `python -c 'import __graft_entry__ as g; g.build()'` first"
    return _lib.load()


def test_symbol_is_exported_by_the_library(lib):
    assert hasattr(lib, NAME)
    assert getattr(lib, NAME).argtypes == _lib.SIGNATURES[NAME][1]


def test_null_engine_is_an_invalid_argument(lib):
    counts = (C.c_int32 * 3)(8, 5, 2)
    assert lib.pd_engine_set_frame_counts(None, 3, counts, None) == -1          # PD_ERR_INVALID_ARG
    assert "NULL engine" in _lib.last_error()
    assert lib.pd_engine_set_frame_counts(None, 0, None, None) == -1            # clearing needs an engine too


def test_python_entry_points_take_n_frames():
    import inspect

    from posediffusion_amd import synth
    from posediffusion_amd.engine import PoseEngine
    from posediffusion_amd.pipeline import SamplingPipeline
    GaussianDiffusion = synth._dropin().GaussianDiffusion           # (the drop-in tree is importable through its own registry)
    assert "n_frames" in inspect.signature(PoseEngine.set_frame_counts).parameters
    for fn in (PoseEngine.denoise, PoseEngine.p_mean, PoseEngine.p_finish, PoseEngine.ggs_guide, PoseEngine.ggs_optimize,
               PoseEngine.ggs_loss_grad, PoseEngine.sample, SamplingPipeline.submit, GaussianDiffusion.sample, GaussianDiffusion.p_sample_loop):
        p = inspect.signature(fn).parameters
        assert "n_frames" in p and p["n_frames"].default is None, fn.__qualname__
    # the reference's signature is unchanged when the keyword is omitted (gaussian_diffuser.py:284, :303)
    assert list(inspect.signature(GaussianDiffusion.sample).parameters)[:5] == ["self", "shape", "z", "cond_fn", "cond_start_step"]
