"""GPU: the Python layer over pd_train_images (posediffusion_amd.images.prepare_training_images) and the drop-in Co3dDataset's device half
(``finish_batch``) on the synthetic Co3D tree of tests/train_images_checks.py, and its batch through
``PoseDiffusionModel(image=..., gt_cameras=..., training=True)`` with both ``engine_grad`` opt-ins."""
import importlib

import numpy as np
import pytest
import torch

import train_images_checks as IC
from posediffusion_amd import images, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# what the two sequences of the drop-in batch draw, stated here so that the test does not hang on a generator's stream
DRAWS = [dict(jitter=1, order=(3, 0, 2, 1), brightness=1.25, contrast=0.7, saturation=0.9, hue=0.06, grayscale=0, erase=(4, 9, 6, 11)),
         dict(jitter=1, order=(1, 2, 3, 0), brightness=0.75, contrast=1.3, saturation=1.15, hue=-0.08, grayscale=1, erase=(0, 0, 0, 0))]


@pytest.fixture(scope="module")
def colour_bound():
    """4 x the fp32 yardstick's own error over the colour table of tests/test_gpu_train_images.py"""
    return IC.colour_table_bound()


def _model():
    from posediffusion_amd.compat import AttrDict
    models = synth._dropin()
    cfg = {"pose_encoding_type": "absT_quaR_logFL",
           "IMAGE_FEATURE_EXTRACTOR": AttrDict({"_target_": "models.MultiScaleImageFeatureExtractor", "freeze": False, "scale_factors": [1, 1 / 2]}),
           "DENOISER": AttrDict({"_target_": "models.Denoiser", "TRANSFORMER": AttrDict(synth.TRANSFORMER_CFG)}),
           "DIFFUSER": AttrDict({"_target_": "models.GaussianDiffusion", "beta_schedule": "custom"})}
    torch.manual_seed(0)
    return models.PoseDiffusionModel(**cfg).to(DEV).eval()


def _yard(frames, boxes, S, draws, seq, fill=0):
    out, taps = [], 0
    for k, (fr, b) in enumerate(zip(frames, boxes)):
        y, (tx, ty) = IC.yardstick(np.asarray(fr), (int(b[0]), int(b[1]), int(b[2] - b[0])), S, fill, draws[seq[k]] if seq[k] >= 0 else None)
        out.append(y)
        taps = max(taps, tx)
    return torch.stack(out), taps


def test_prepare_training_images_mixed_inputs_workspace_and_strict(colour_bound):
    frames = [IC.picture(40, 50, 1), torch.from_numpy(IC.picture(33, 33, 2)), IC.picture(53, 37, 3), IC.picture(64, 64, 4)]
    boxes = [[-3, 2, 37, 42], [0, 0, 33, 33], [0, 5, 37, 42], [10, 10, 42, 42]]
    draws = [dict(jitter=1, order=(2, 0, 3, 1), brightness=0.8, contrast=1.2, saturation=0.9, hue=0.05, grayscale=0, erase=(0, 0, 0, 0)),
             dict(images.NO_COLOUR, grayscale=1)]
    seq = [0, 1, -1, 0]
    out, st = images.prepare_training_images(frames, boxes, image_size=32, sequence_of_frame=seq, colour=draws, device=DEV)
    assert out.shape == (4, 3, 32, 32) and out.dtype == torch.float32 and out.device.type == "cuda" and st.tolist() == [0] * 4
    ref, taps = _yard(frames, boxes, 32, draws, seq)
    err = (out.cpu().double() - ref).abs().max().item()
    print(f"prepare_training_images: err {err:.3e}, colour bound {colour_bound[0]:.3e}, resize bound {IC.resize_bound(taps, taps):.3e}")
    assert err <= max(colour_bound[0], IC.resize_bound(taps, taps))
    assert (out[2].cpu().double() - ref[2]).abs().max().item() <= IC.resize_bound(taps, taps)       # the frame without a colour entry
    ws = images._CACHE[0]["workspace"]
    ptr, pinned = ws.data_ptr(), images._CACHE[0]["pinned"].data_ptr()
    buf = torch.empty(4, 3, 32, 32, device=DEV)
    again, _ = images.prepare_training_images(frames, boxes, image_size=32, sequence_of_frame=seq, colour=draws, device=DEV, out=buf)
    assert again is buf and torch.equal(again, out)
    assert images._CACHE[0]["workspace"].data_ptr() == ptr and images._CACHE[0]["pinned"].data_ptr() == pinned      # reused
    one, _ = images.prepare_training_images(frames[:1], boxes[:1], image_size=32, colour=draws[0], device=DEV)     # a single draw, no table
    assert torch.equal(one[0], out[0])
    bad = [dict(draws[0], order=(0, 0, 1, 2))]
    with pytest.raises(ValueError, match="frame 1.*permutation"):
        images.prepare_training_images(frames[:2], boxes[:2], image_size=32, sequence_of_frame=[-1, 0], colour=bad, device=DEV)
    out2, st2 = images.prepare_training_images(frames[:2], boxes[:2], image_size=32, sequence_of_frame=[-1, 0], colour=bad, device=DEV,
                                               strict=False)
    assert st2.tolist() == [0, 4] and float(out2[1].abs().max()) == 0.0 and float(out2[0].abs().max()) > 0.0
    with pytest.raises(ValueError, match="square"):
        images.prepare_training_images(frames[:1], [[0, 0, 10, 11]], image_size=32, device=DEV)
    with pytest.raises(ValueError, match="uint8"):
        images.prepare_training_images([np.zeros((4, 4, 3), np.float32)], [[0, 0, 4, 4]], image_size=32, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        images.prepare_training_images(frames[:1], boxes[:1], image_size=32, device="cpu")
    empty, st0 = images.prepare_training_images([], np.zeros((0, 4)), image_size=32, device=DEV)
    assert empty.shape == (0, 3, 32, 32) and st0.numel() == 0


@pytest.fixture(scope="module")
def dataset_and_samples(tmp_path_factory):
    synth._dropin()
    ds_mod = importlib.import_module("datasets.co3d_v2")
    kw = IC.write_co3d_tree(str(tmp_path_factory.mktemp("co3d")))
    ds = ds_mod.Co3dDataset(normalize_cameras=True, compute_optical=True, erase_aug=True, **kw)
    np.random.seed(5)
    torch.manual_seed(5)
    samples = [ds[(0, 3)], ds[(1, 3)]]
    assert all(isinstance(s["colour"], dict) for s in samples)
    return ds, [dict(s, colour=dict(e)) for s, e in zip(samples, DRAWS)]


def test_finish_batch_keys_shapes_images_and_cameras(dataset_and_samples, colour_bound):
    from posediffusion_amd.cameras import normalize_cameras_batch
    ds, samples = dataset_and_samples
    batch = ds.finish_batch(samples, DEV)
    assert sorted(batch) == sorted(["image", "R", "T", "fl", "pp", "crop_params", "R_original", "T_original", "seq_id", "category", "n", "ind"])
    want = {"image": (2, 3, 3, 32, 32), "R": (2, 3, 3, 3), "T": (2, 3, 3), "fl": (2, 3, 2), "pp": (2, 3, 2), "crop_params": (2, 3, 3),
            "R_original": (2, 3, 3, 3), "T_original": (2, 3, 3)}
    for k, shape in want.items():
        assert tuple(batch[k].shape) == shape and batch[k].dtype == torch.float32 and batch[k].device.type == "cuda", k
    assert batch["seq_id"] == ["seq0", "seq1"] and batch["category"] == ["apple", "apple"] and batch["n"].tolist() == [6, 6]
    assert batch["ind"].shape == (2, 3) and batch["ind"].dtype == torch.int64
    frames = [f for s in samples for f in s["frames"]]
    boxes = np.concatenate([s["boxes"] for s in samples])
    ref, taps = _yard(frames, boxes, 32, [s["colour"] for s in samples], [0] * 3 + [1] * 3)
    err = (batch["image"].reshape(6, 3, 32, 32).cpu().double() - ref).abs().max().item()
    bound = max(colour_bound[0], IC.resize_bound(taps, taps))
    print(f"finish_batch image: err {err:.3e}, bound {bound:.3e} (draws {[s['colour'] for s in samples]})")
    assert err <= bound
    R = torch.stack([s["R"] for s in samples]).to(DEV)
    T = torch.stack([s["T"] for s in samples]).to(DEV)
    res = normalize_cameras_batch(R, T, compute_optical=True, first_camera=True)
    assert torch.equal(batch["R"], res.R) and torch.equal(batch["T"], res.T)
    assert torch.equal(batch["R_original"], R) and torch.equal(batch["T_original"], T)
    assert torch.equal(batch["fl"].cpu(), torch.stack([s["fl"] for s in samples]))
    assert torch.equal(batch["pp"].cpu(), torch.stack([s["pp"] for s in samples]))
    with pytest.raises(ValueError, match="same number of frames"):
        ds.finish_batch([samples[0], ds[(1, 2)]], DEV)
    with pytest.raises(RuntimeError, match="normalizing cameras"):                  # all cameras at one centre: the reference's scale-0 branch
        degenerate = dict(samples[0], T=torch.zeros(3, 3))
        ds.finish_batch([degenerate, samples[1]], DEV)


def test_the_batch_trains_through_the_model(dataset_and_samples):
    from posediffusion_amd.compat import PerspectiveCameras
    ds, samples = dataset_and_samples
    batch = ds.finish_batch(samples, DEV)
    model = _model()
    model.image_feature_extractor.engine_grad = model.diffuser.engine_grad = model.diffuser.engine_grad_outputs = True
    cams = PerspectiveCameras(focal_length=batch["fl"].reshape(-1, 2), R=batch["R"].reshape(-1, 3, 3), T=batch["T"].reshape(-1, 3),
                              device=torch.device(DEV))
    torch.manual_seed(2)
    out = model(image=batch["image"], gt_cameras=cams, training=True)
    pc = out["pred_cameras"]
    assert out["x_0_pred"].requires_grad and pc.R.requires_grad
    (out["loss"].mean() + 1e-3 * (pc.T.sum() + pc.focal_length.sum())).backward()
    for name, p in list(model.image_feature_extractor._net.named_parameters()) + list(model.diffuser.model.named_parameters()):
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
