"""posediffusion_amd -- MI355X-native sampling engine for PoseDiffusion (gfx950 / CDNA4).

Scope: ONE hot path of facebookresearch/PoseDiffusion -- the DDPM reverse loop over camera-pose
tokens (GaussianDiffusion.p_sample_loop + the transformer Denoiser) and the Geometry-Guided
Sampling step -- as hand-written HIP kernels behind a C-ABI (include/pd_engine.h), plus the
host-side mirror of the reference's Python interface for that path (``dropin/``).

    csrc/      HIP kernels + C-ABI  -> lib/libpd_engine.so   (no CPU fallback)
    _lib.py    ctypes binding        engine.py  PoseEngine wrapper
    host.py    engine cache / cond_fn recognition for the drop-in modules
    dropin/    `models` + `util` packages with the reference's names (Hydra _target_ registry)
    synth.py   synthetic weights / features / matches for tests and bench
    shard.py   one-process-per-GPU sharding of independent sequences + final gather
    optim.py   EngineAdamW / clip_grad_norm_: the optimiser step of training on the engine
    cameras.py normalize_cameras_batch: ground-truth camera normalisation (util/normalize_cameras.py) on the engine
    images.py  prepare_training_images: crop, antialiased resize and colour jitter of a batch's decoded frames (datasets/co3d_v2.py) on the engine
"""
import os

DROPIN_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropin")

__all__ = ["DROPIN_PATH", "EngineAdamW", "clip_grad_norm_", "normalize_cameras_batch", "prepare_training_images"]


def __getattr__(name):
    # the optimiser's names, resolved on first use: importing the package alone must not import torch
    if name in ("EngineAdamW", "clip_grad_norm_"):
        from . import optim
        return getattr(optim, name)
    if name == "normalize_cameras_batch":
        from . import cameras
        return cameras.normalize_cameras_batch
    if name == "prepare_training_images":
        from . import images
        return images.prepare_training_images
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
