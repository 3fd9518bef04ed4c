"""No GPU: the C-ABI of the camera-normalisation kernel (include/pd_engine_cameras.h, posediffusion_amd._lib.CAMERA_SIGNATURES, the built
library), the argument refusals that need no device, and the new drop-in names."""
import ctypes as C
import importlib
import os
import re

import pytest
import torch

import normalize_checks as NC
from posediffusion_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "pd_engine_cameras.h")) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


def test_header_and_camera_signatures_list_the_same_functions():
    hdr = _header()
    assert set(re.findall(r"\b(pd_\w+)\s*\(", hdr)) == set(_lib.CAMERA_SIGNATURES) == {"pd_normalize_cameras"}
    others = (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.TRAIN_SIGNATURES) | set(_lib.VIT_TRAIN_SIGNATURES) |
              set(_lib.OPTIM_SIGNATURES))
    assert not set(_lib.CAMERA_SIGNATURES) & others
    for name, (_, args) in _lib.CAMERA_SIGNATURES.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == len(args), name
    m = re.search(r"typedef struct \{(.*?)\} pd_cam_norm_cfg;", hdr, flags=re.S)
    assert re.findall(r"\bint (\w+);", m.group(1)) == [n for n, _ in _lib.pd_cam_norm_cfg._fields_]
    assert C.sizeof(_lib.pd_cam_norm_cfg) == 12
    codes = dict(re.findall(r"#define (PD_CAM_\w+) (\d+)", hdr))
    assert {k: int(v) for k, v in codes.items()} == {k: getattr(_lib, k) for k in ("PD_CAM_OK", "PD_CAM_ZERO_SCALE", "PD_CAM_RANK",
                                                                                   "PD_CAM_NON_FINITE", "PD_CAM_BAD_COUNT")}
    with open(os.path.join(ROOT, "posediffusion_amd", "csrc", "pd_cameras.hip")) as fh:
        assert float(re.search(r"#define PD_CAM_RANK_TOL (\S+)", fh.read()).group(1)) == NC.RANK_TOL
    assert "1e-10 trace(A)" in open(os.path.join(ROOT, "include", "pd_engine_cameras.h")).read()


def test_the_symbol_is_exported_and_refuses_bad_arguments_before_any_launch():
    assert os.path.isfile(_lib.LIB_PATH), "run `python -c 'import __graft_entry__ as g; g.build()'` first"
    lib = _lib.load()
    fn = lib.pd_normalize_cameras
    assert fn.argtypes == _lib.CAMERA_SIGNATURES["pd_normalize_cameras"][1]
    cfg = _lib.pd_cam_norm_cfg(1, 1, 0)
    p = 0x1000                                                            # never dereferenced: every call below is refused on the host

    def call(R=p, T=p, B=1, N=2, cfg=cfg, R_out=p, T_out=p, focal=None, enc=None, status=p):
        return fn(R, T, B, N, None, C.byref(cfg) if cfg is not None else None, R_out, T_out, focal, 1.8, 0.1, 20.0, enc, None, None, None,
                  None, None, status, None)

    for kw, word in ((dict(R=None), "R is NULL"), (dict(T=None), "T is NULL"), (dict(cfg=None), "cfg is NULL"),
                     (dict(R_out=None), "R_out is NULL"), (dict(T_out=None), "T_out is NULL"), (dict(status=None), "status_out is NULL"),
                     (dict(B=-1), "B = -1"), (dict(N=0), "N = 0"), (dict(enc=p), "enc_out needs focal"),
                     (dict(cfg=_lib.pd_cam_norm_cfg(3, 1, 0)), "scale_mode 3"), (dict(cfg=_lib.pd_cam_norm_cfg(1, -1, 0)), "first_camera -1"),
                     (dict(cfg=_lib.pd_cam_norm_cfg(1, 1, 2)), "normalize_T 2")):
        assert call(**kw) == -1, kw
        assert "pd_normalize_cameras" in _lib.last_error() and word in _lib.last_error(), (kw, _lib.last_error())
    assert call(B=0) == 0                                                  # a no-op


def test_the_dropin_names_import():
    import posediffusion_amd
    from posediffusion_amd import synth
    synth._dropin()
    nc = importlib.import_module("util.normalize_cameras")
    assert nc.__file__.startswith(posediffusion_amd.DROPIN_PATH)
    for name in ("normalize_cameras", "first_camera_transform", "normalize_Trans", "compute_optical_axis_intersection",
                 "normalize_cameras_batch"):
        assert callable(getattr(nc, name)), name
    ct = importlib.import_module("util.camera_transform")
    for name in ("bbox_xyxy_to_xywh", "adjust_camera_to_bbox_crop_", "adjust_camera_to_image_scale_", "_convert_ndc_to_pixels",
                 "_convert_pixels_to_ndc", "pose_encoding_to_camera", "camera_to_pose_encoding"):
        assert callable(getattr(ct, name)), name
    from posediffusion_amd import cameras
    assert posediffusion_amd.normalize_cameras_batch is cameras.normalize_cameras_batch
    import inspect
    sig = inspect.signature(nc.normalize_cameras)
    assert list(sig.parameters) == ["cameras", "compute_optical", "first_camera", "scale", "normalize_T"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [True, True, 1.0, False]
    from models.pose_diffusion_model import PoseDiffusionModel
    assert inspect.signature(PoseDiffusionModel.forward).parameters["normalize_gt"].default is None


def test_cpu_tensors_are_refused():
    from posediffusion_amd import cameras
    from posediffusion_amd.compat import PerspectiveCameras
    R, T = NC.ring(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cameras.normalize_cameras_batch(R.float()[None], T.float()[None])
    from posediffusion_amd import synth
    synth._dropin()
    nc = importlib.import_module("util.normalize_cameras")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nc.normalize_cameras(PerspectiveCameras(focal_length=torch.ones(3, 2), R=R.float(), T=T.float()))
    with pytest.raises(ValueError, match="on_degenerate"):
        cameras.normalize_cameras_batch(R.float()[None], T.float()[None], on_degenerate="ignore")
