"""ctypes binding of libpd_engine.so (the C-ABI declared in include/pd_engine.h).

The product path has NO fallback: if the shared library is missing or cannot be loaded this
module raises, and every engine entry point raises with it.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# PD_ENGINE_LIB: another build of the same C-ABI (same-box A / B of two libraries: tools/ab_ggs.py, bench.py); default = the in-tree build
LIB_PATH = os.environ.get("PD_ENGINE_LIB") or os.path.join(_HERE, "lib", "libpd_engine.so")
CSRC_DIR = os.path.join(_HERE, "csrc")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "pd_engine.h"))

PD_MAX_LAYERS = 16

c_float_p = C.POINTER(C.c_float)


class pd_layer_weights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "norm1_w", "norm1_b", "in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b",
        "norm2_w", "norm2_b", "linear1_w", "linear1_b", "linear2_w", "linear2_b")]


class pd_weights(C.Structure):
    _fields_ = (
        [(n, C.c_int32) for n in ("d_model", "nhead", "dim_ff", "num_layers", "z_dim", "n_harmonic",
                                  "t_emb_dim", "mlp_hidden", "timesteps", "reserved")]
        + [(n, C.c_void_p) for n in ("time_w0", "time_b0", "time_w2", "time_b2", "first_w", "first_b")]
        + [("layers", pd_layer_weights * PD_MAX_LAYERS)]
        + [(n, C.c_void_p) for n in ("last0_w", "last0_b", "last_ln_w", "last_ln_b", "last3_w", "last3_b",
                                     "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
                                     "posterior_mean_coef1", "posterior_mean_coef2",
                                     "posterior_log_variance_clipped")]
    )


class pd_layer_grads(C.Structure):
    """include/pd_engine_train.h: where each tensor's gradient goes (mirrors pd_layer_weights; None = not wanted)"""
    _fields_ = list(pd_layer_weights._fields_)


class pd_weight_grads(C.Structure):
    """include/pd_engine_train.h: mirrors the weight members of pd_weights"""
    _fields_ = (
        [(n, C.c_void_p) for n in ("time_w0", "time_b0", "time_w2", "time_b2", "first_w", "first_b")]
        + [("layers", pd_layer_grads * PD_MAX_LAYERS)]
        + [(n, C.c_void_p) for n in ("last0_w", "last0_b", "last_ln_w", "last_ln_b", "last3_w", "last3_b")]
    )


class pd_vit_layer_weights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("norm1_w", "norm1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "norm2_w", "norm2_b",
                                          "fc1_w", "fc1_b", "fc2_w", "fc2_b")]


class pd_vit_weights(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("dim", "depth", "num_heads", "mlp_hidden", "patch_size", "pos_grid", "reserved0", "reserved1")]
                + [(n, C.c_void_p) for n in ("patch_w", "patch_b", "cls_token", "pos_embed", "norm_w", "norm_b")]
                + [("layers", pd_vit_layer_weights * 16)])


class pd_vit_layer_grads(C.Structure):
    """include/pd_engine_vit_train.h: where each tensor's gradient goes (mirrors pd_vit_layer_weights; None = not wanted)"""
    _fields_ = list(pd_vit_layer_weights._fields_)


class pd_vit_weight_grads(C.Structure):
    """include/pd_engine_vit_train.h: mirrors the pointer members of pd_vit_weights"""
    _fields_ = ([(n, C.c_void_p) for n in ("patch_w", "patch_b", "cls_token", "pos_embed", "norm_w", "norm_b")]
                + [("layers", pd_vit_layer_grads * 16)])


PD_VIT_TRAIN_MAX_TOKENS, PD_VIT_TRAIN_MAX_SCALES = 256, 8   # include/pd_engine_vit_train.h: tokens per image and scale; scales per call

# pd_ggs_cfg.reserved flags and pd_engine_set_option ids (include/pd_engine.h; tests/test_host_cpu.py checks them against the header)
PD_GGS_CFG_FORCE_ONE_HOP = 1
PD_GGS_CFG_NO_LDS_STAGING = 2
PD_GGS_CFG_WAVES8 = 4
PD_WEIGHTS_PRED_X0 = 1
PD_WEIGHTS_POST_NORM = 2     # TransformerEncoderWrapper(norm_first=False) (shape-generic denoiser path)
PD_WEIGHTS_NO_PIVOT = 4      # Denoiser(pivot_cam_onehot=False) (shape-generic denoiser path)
PD_WEIGHTS_GENERIC = 8       # the shape-generic denoiser path even at the default shape (comparison / testing)
PD_GGS_CFG_LANE_ITEMS = 8       # lane-per-item kernel (the throughput shape) whatever the batch size
PD_GGS_CFG_NO_LANE_ITEMS = 16   # never the lane-per-item kernel
PD_GGS_CFG_XCHG_SPREAD = 32     # k > 1: no XCD-local placement of a sequence's workgroups (comparison)
PD_GGS_CFG_LONG_FRAMES = 64     # the kernel of sequences above 64 frames at any N (comparison / testing)
PD_OPT_DENOISER_SPLIT = 2
PD_OPT_WEIGHTS_NON_FINITE = 4   # pd_engine_get_option only
PD_OPT_DENOISER_FUSED_ATTN = 5  # in_proj + attention as one kernel, Q / K / V in LDS (default 1)
PD_OPT_DENOISER_LONG_ATTN = 6   # 1: the key-tiled attention kernel of sequences above 64 frames for every N (default 0; comparison / testing)
PD_OPT_GGS_MAX_FRAMES = 7       # frames GGS admits: 64 (default) or a value in (64, max_N]; reallocates the exchange region, synchronous
PD_OPT_GGS_LONG_PAIR_ITEMS = 8  # 0 (default) / 1: above 64 frames a frame pair may hold more than 512 matches (pd_ggs_longm_kernel)
PD_DROP_ATTN, PD_DROP_RESID1, PD_DROP_FF, PD_DROP_RESID2, PD_DROP_ALL = 1, 2, 4, 8, 15   # pd_train_forward_dropout's sites (include/pd_engine_train.h)
PD_TR_OPT_MAX_FRAMES, PD_TR_OPT_LONG_ATTN = 1, 2   # pd_trainer_set_option (include/pd_engine_train.h): frame limit 64 .. 256; key-tiled attention at every N
PD_MATCH_HINT_ONE_ORDER = 1 << 30   # pd_match_hints.max_pairs flag: every frame pair in one order only (hloc's i < j pairs)
PD_OPTIM_CHUNK = 4096   # include/pd_engine_optim.h: elements of one tensor per partial sum of the gradient norm and per workgroup turn


class pd_ggs_cfg(C.Structure):
    _fields_ = [("alpha", C.c_float), ("learning_rate", C.c_float), ("iter_num", C.c_int32),
                ("sampson_max", C.c_float), ("min_matches", C.c_int32), ("momentum", C.c_float),
                ("wgs_per_seq", C.c_int32), ("reserved", C.c_int32)]


class pd_match_hints(C.Structure):
    _fields_ = [("max_pairs", C.c_int32), ("max_matches_per_pair", C.c_int32)]


class pd_optim_tensor(C.Structure):
    """include/pd_engine_optim.h: one parameter that has a gradient this step (device pointers as integers)"""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("numel", C.c_int64), ("group", C.c_int32), ("step", C.c_int32)]


class pd_optim_group(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("lr", "beta1", "beta2", "eps", "weight_decay")]


class pd_cam_norm_cfg(C.Structure):
    """include/pd_engine_cameras.h: scale_mode 0 none / 1 optical-axis intersection / 2 sqrt(||T||_F); first_camera 0 off / 1 full /
    2 rotation only; normalize_T 0 / 1"""
    _fields_ = [(n, C.c_int) for n in ("scale_mode", "first_camera", "normalize_T")]


PD_CAM_OK, PD_CAM_ZERO_SCALE, PD_CAM_RANK, PD_CAM_NON_FINITE, PD_CAM_BAD_COUNT = range(5)   # pd_normalize_cameras' status_out


class pd_img_frame(C.Structure):
    """include/pd_engine_images.h: one decoded frame inside the pixel buffer and its square crop box (colour: index of its draw, -1 none)"""
    _fields_ = [("offset", C.c_int64)] + [(n, C.c_int32) for n in ("height", "width", "x0", "y0", "side", "colour")]


class pd_img_colour(C.Structure):
    """include/pd_engine_images.h: one sequence's colour draw (order: a permutation of 0 brightness, 1 contrast, 2 saturation, 3 hue)"""
    _fields_ = ([("jitter", C.c_int32), ("order", C.c_int32 * 4)] + [(n, C.c_float) for n in ("brightness", "contrast", "saturation", "hue")]
                + [(n, C.c_int32) for n in ("grayscale", "erase_top", "erase_left", "erase_h", "erase_w")])


PD_IMG_OK, PD_IMG_BAD_SIDE, PD_IMG_BAD_SIZE, PD_IMG_BAD_COLOUR, PD_IMG_BAD_ORDER, PD_IMG_BAD_ERASE = range(6)   # pd_train_images' status_out
PD_IMG_MAX_SIDE, PD_IMG_MAX_SIZE, PD_IMG_MAX_FRAMES = 6144, 1024, 65535


# name -> (restype, argtypes); kept in one table so the "exports every declared symbol" test and
# the binding cannot drift apart.
_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64
SIGNATURES = {
    "pd_engine_create": (_i, [C.POINTER(pd_weights), _i, _i, C.POINTER(_vp)]),
    "pd_engine_destroy": (None, [_vp]),
    "pd_last_error": (C.c_char_p, []),
    "pd_version": (C.c_char_p, []),
    "pd_denoise_step": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "pd_engine_set_q_tables": (_i, [_vp, _vp, _vp]),
    "pd_engine_set_frame_counts": (_i, [_vp, _i, C.POINTER(C.c_int32), _vp]),
    "pd_denoise_step_t": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "pd_p_losses": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "pd_camera_to_pose": (_i, [_vp, _vp, _vp, _i, C.c_float, C.c_float, C.c_float, _vp, _vp]),
    "pd_p_mean": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "pd_p_finish": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "pd_ggs_set_matches": (_i, [_vp, _i, _vp, _vp, _vp, _i64, _i, _i, _i]),
    "pd_ggs_set_matches_csr_async": (_i, [_vp, _i, _i, C.POINTER(_i64), _vp, _vp, _vp, _i, _i, _i, C.POINTER(pd_match_hints), _vp]),
    "pd_ggs_guide": (_i, [_vp, _vp, _i, _i, _i, C.POINTER(pd_ggs_cfg), _vp, _vp]),
    "pd_ggs_optimize": (_i, [_vp, _vp, _i, _i, _i, _i, _i, C.POINTER(pd_ggs_cfg), _vp, _vp, _vp]),
    "pd_ggs_loss_grad": (_i, [_vp, _vp, _i, _i, _i, _i, _i, C.POINTER(pd_ggs_cfg), _vp, _vp, _vp]),
    "pd_engine_set_option": (_i, [_vp, _i, _i]),
    "pd_engine_get_option": (_i, [_vp, _i, C.POINTER(_i)]),
    "pd_time_embedding": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "pd_pose_embedding": (_i, [_vp, C.c_longlong, _i, _vp, _vp]),
    "pd_metrics_rel_pose_errors": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "pd_metrics_summary": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "pd_metrics_are": (_i, [_vp, _vp, _i, _vp, _vp]),
    "pd_vit_create": (_i, [C.POINTER(pd_vit_weights), C.POINTER(_vp)]),
    "pd_vit_destroy": (None, [_vp]),
    "pd_vit_set_option": (_i, [_vp, _i, _i]),
    "pd_vit_forward_scale": (_i, [_vp, _vp, _i, _i, _i, C.c_double, _vp, C.c_float, _i, _vp, _vp]),
    "pd_preprocess_image": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "pd_align_cameras": (_i, [_vp, _vp, _vp, _vp, _i, _i, C.c_float, _vp, _vp, _vp, _vp]),
    "pd_sample": (_i, [_vp, _vp, _vp, _i, _i, _i, C.POINTER(pd_ggs_cfg), _vp, _vp, _vp, _i, _vp]),
    "pd_sample_phase": (_i, [_vp, _vp, _vp, _i, _i, _i, C.POINTER(pd_ggs_cfg), _i, _vp, _vp, _vp, _i, _vp]),
    "pd_pose_to_camera": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "pd_debug_lane_tables": (_i, [_vp, _i, C.POINTER(C.c_int), _i]),
    "pd_ggs_launch_stamps": (_i, [_vp, _vp, _i, C.POINTER(C.c_int), _vp]),
    "pd_ggs_stage_iters": (_i, [C.POINTER(pd_ggs_cfg), C.POINTER(C.c_int)]),
    "pd_pose_to_camera_ex": (_i, [_vp, _vp, _i, _vp, _vp, _vp, C.c_float, C.c_float, C.c_float, _vp]),
    "pd_time_kernel": (_i, [_vp, _i, _i, _i, C.POINTER(pd_ggs_cfg), _i, C.POINTER(C.c_float), _vp]),
    "pd_check_async_error": (_i, [_vp]),
    "pd_debug_ggs_prof": (_i, [_vp, _i, C.POINTER(C.c_longlong)]),
    "pd_debug_ggs_plan": (_i, [_vp, _i, _i, C.POINTER(pd_ggs_cfg), C.POINTER(C.c_int)]),
    "pd_debug_mfma_f16_subnormal": (_i, [C.POINTER(C.c_float), _vp]),
    "pd_debug_vit_tokens": (_i, [_vp, _vp, C.c_longlong, _vp]),
}
# the exports of include/pd_engine_ingest.h (the function list of pd_engine.h, and with it SIGNATURES, is pinned by the tests)
EXT_SIGNATURES = {
    "pd_ggs_set_matches_csr_async_nf": (_i, [_vp, _i, _i, C.POINTER(_i64), _vp, _vp, _vp, C.POINTER(_i), _i, _i, C.POINTER(pd_match_hints), _vp]),
}
# the exports of include/pd_engine_train.h: the training branch with gradients (a table of its own -- tests pin the other two lists)
TRAIN_SIGNATURES = {
    "pd_trainer_create": (_i, [C.POINTER(pd_weights), _vp, _vp, _i, _i, C.POINTER(_vp)]),
    "pd_trainer_destroy": (None, [_vp]),
    "pd_trainer_set_option": (_i, [_vp, _i, _i]),
    "pd_trainer_get_option": (_i, [_vp, _i, C.POINTER(_i)]),
    "pd_trainer_set_frame_counts": (_i, [_vp, _i, C.POINTER(C.c_int32), _vp]),
    "pd_train_forward": (_i, [_vp, C.POINTER(pd_weights), _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "pd_train_forward_dropout": (_i, [_vp, C.POINTER(pd_weights), _vp, _vp, _vp, _vp, _i, _i, _i, C.c_float, C.c_uint, C.c_uint64, C.c_uint32,
                                      _vp, _vp, _vp, _vp, _vp]),
    "pd_train_backward": (_i, [_vp, C.POINTER(pd_weights), _vp, C.POINTER(pd_weight_grads), _vp, _vp]),
    "pd_train_backward_ex": (_i, [_vp, C.POINTER(pd_weights), _vp, _vp, _vp, C.POINTER(pd_weight_grads), _vp, _vp]),
    "pd_pose_to_camera_backward": (_i, [_vp, _vp, _vp, _vp, _i, C.c_float, C.c_float, C.c_float, _vp, _vp]),
    "pd_train_debug_relu": (_i, [_vp, _i, _vp, C.c_longlong, _vp]),
    "pd_trainer_check_async": (_i, [_vp]),
}
# the exports of include/pd_engine_vit_train.h: the image backbone with gradients (again a table of its own)
VIT_TRAIN_SIGNATURES = {
    "pd_vit_trainer_create": (_i, [C.POINTER(pd_vit_weights), _i, _i, _i, C.POINTER(_vp)]),
    "pd_vit_trainer_destroy": (None, [_vp]),
    "pd_vit_train_forward": (_i, [_vp, C.POINTER(pd_vit_weights), _vp, _i, _i, _i, C.POINTER(C.c_double), _i, C.POINTER(_vp), _vp, _vp]),
    "pd_vit_train_backward": (_i, [_vp, C.POINTER(pd_vit_weights), _vp, C.POINTER(pd_vit_weight_grads), _vp]),
}
# the exports of include/pd_engine_optim.h: global-norm clipping and AdamW (a fourth extension table)
OPTIM_SIGNATURES = {
    "pd_optimizer_create": (_i, [_i, _i64, C.POINTER(_vp)]),
    "pd_optimizer_destroy": (None, [_vp]),
    "pd_optim_grad_norm": (_i, [_vp, C.POINTER(pd_optim_tensor), _i, _vp, _vp]),
    "pd_optim_clip_grad_norm": (_i, [_vp, C.POINTER(pd_optim_tensor), _i, C.c_double, _vp, _vp]),
    "pd_optim_adamw_step": (_i, [_vp, C.POINTER(pd_optim_tensor), _i, C.POINTER(pd_optim_group), _i, C.c_double, _vp, _vp]),
}
# the exports of include/pd_engine_cameras.h: ground-truth camera normalisation (a fifth extension table)
CAMERA_SIGNATURES = {
    "pd_normalize_cameras": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(pd_cam_norm_cfg), _vp, _vp, _vp, C.c_float, C.c_float, C.c_float,
                                  _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}

# the exports of include/pd_engine_images.h: training images, crop + antialiased resize + colour draw (a sixth extension table)
IMAGE_SIGNATURES = {
    "pd_train_images_workspace_bytes": (C.c_longlong, [_i, _i]),
    "pd_train_images": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, C.c_longlong, _vp]),
}

_lib = None


def build(verbose: bool = False) -> str:
    """Compile libpd_engine.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC_DIR, "-j4"]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0 or not os.path.isfile(LIB_PATH):
        raise RuntimeError("building libpd_engine.so failed:\n" + res.stdout[-4000:])
    return LIB_PATH


def load():
    """dlopen the engine.  torch is imported first so that libamdhip64.so.7 resolves to the copy
    PyTorch-ROCm already loaded (one HIP runtime per process: device pointers and streams are
    shared with torch)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise RuntimeError(
            f"posediffusion_amd: HIP engine library not found at {LIB_PATH}. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C posediffusion_amd/csrc`). "
            "There is no CPU fallback.")
    import torch  # noqa: F401  (loads the HIP runtime first)
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in {**SIGNATURES, **EXT_SIGNATURES, **TRAIN_SIGNATURES, **VIT_TRAIN_SIGNATURES, **OPTIM_SIGNATURES,
                                   **CAMERA_SIGNATURES, **IMAGE_SIGNATURES}.items():
        if os.environ.get("PD_ENGINE_LIB") and not hasattr(lib, name):
            continue              # an older build under A / B lacks the newest debug exports
        fn = getattr(lib, name)   # AttributeError here = library does not match the header
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def last_error() -> str:
    return (load().pd_last_error() or b"").decode("utf-8", "replace")


def check(rc: int, what: str = "pd_engine"):
    if rc != 0:
        raise RuntimeError(f"{what} failed (code {rc}): {last_error()}")
