"""Row R2 / BASELINE configs[0]: the call sequence of the reference's `pose_diffusion/demo.py` and the MODEL / GGS nodes of its
`cfgs/default.yaml` on the drop-in packages (posediffusion_amd/run_reference.py + compat/shims + tools/make_synthetic_ckpt.py).

demo.py itself is not part of this repository, so the suite runs its call sequence (`test_demo_call_sequence_on_synthetic_folder`)
and pins the config nodes against tests/golden/default_cfg.json (oracle/make_golden.py `default_cfg`).  Transcripts of demo.py
itself running unchanged on an MI355X are committed under profiles/ (round*_demo_ggs_off.log; tools/round6_end.sh).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(script, overrides, cwd, timeout=900):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "posediffusion_amd.run_reference", script, *overrides], cwd=cwd, env=env,
                          capture_output=True, text=True, timeout=timeout)


# ------------------------------------------------------------------------------------------------ CPU: shims
def test_hydra_and_omegaconf_standins(tmp_path):
    """hydra.main: yaml relative to the decorated function's file, key=value / nested / +new overrides parsed as YAML
    scalars, get_original_cwd; OmegaConf: set_struct / to_yaml / to_container and in-place nested assignment."""
    (tmp_path / "conf").mkdir()
    (tmp_path / "conf" / "c.yaml").write_text("a: 1\ng:\n  enable: true\n  lr: 0.01\nname: x\n")
    (tmp_path / "app.py").write_text(
        "import hydra, json, os\nfrom omegaconf import OmegaConf, DictConfig\nfrom hydra.utils import get_original_cwd\n"
        "@hydra.main(config_path='conf', config_name='c')\n"
        "def main(cfg: DictConfig):\n"
        "    OmegaConf.set_struct(cfg, False)\n"
        "    cfg.g.extra = cfg.name\n"
        "    print('YAML', OmegaConf.to_yaml(cfg).replace('\\n', '|'))\n"
        "    print('JSON', json.dumps(OmegaConf.to_container(cfg.g)), type(OmegaConf.to_container(cfg.g)).__name__)\n"
        "    print('CWD', get_original_cwd() == os.getcwd())\n"
        "if __name__ == '__main__':\n    main()\n")
    r = _run(str(tmp_path / "app.py"), ["a=7", "g.enable=False", "g.lr=1e-3", "+h.k=3", "name=samples/apple"], cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    out = r.stdout
    assert "a: 7" in out and "enable: false" in out and "k: 3" in out
    assert 'JSON {"enable": false, "lr": 0.001, "extra": "samples/apple"} dict' in out
    assert "CWD True" in out


def test_default_cfg_instantiates_through_the_registry_and_checkpoint_round_trips(tmp_path):
    """cfgs/default.yaml's MODEL node -> `instantiate(cfg.MODEL, _recursive_=False)` (demo.py:46) through the drop-in
    `models` registry; tools/make_synthetic_ckpt.py writes the reference key set; `load_state_dict(strict=True)`
    (demo.py:56-57) round-trips bit for bit.  The built-in copy of the MODEL node is pinned against the reference's
    (tests/golden/default_cfg.json), and the checkpoint is also built from a yaml holding the recorded nodes."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_synthetic_ckpt as mk
    from posediffusion_amd.compat import install_shims, to_container
    install_shims()
    from omegaconf import OmegaConf
    import json
    import yaml
    with open(os.path.join(ROOT, "tests", "golden", "default_cfg.json")) as f:
        nodes = json.load(f)
    cfg_path = str(tmp_path / "default.yaml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(nodes, f)
    cfg = OmegaConf.load(cfg_path)
    assert to_container(cfg.MODEL) == mk.DEFAULT_MODEL_CFG, "built-in copy of cfgs/default.yaml MODEL is stale"
    assert to_container(cfg.GGS) == {"enable": True, "start_step": 10, "learning_rate": 0.01, "iter_num": 100,
                                     "sampson_max": 10, "min_matches": 10, "alpha": 0.0001}
    ckpt = str(tmp_path / "synthetic.pth")
    sd = mk.write_checkpoint(ckpt, cfg_path, seed=0)
    keys = set(sd)
    # SURVEY.md section 5 "Checkpoint": the 13 persistent schedule buffers, the denoiser under diffuser.model, DINO under _net
    for k in ("diffuser.betas", "diffuser.posterior_log_variance_clipped", "diffuser.model._first.weight",
              "diffuser.model.time_embed.linear.2.bias", "diffuser.model._trunk.layers.7.self_attn.in_proj_weight",
              "diffuser.model._last.3.bias", "image_feature_extractor._net.blocks.11.mlp.fc2.weight",
              "image_feature_extractor._net.pos_embed", "image_feature_extractor._net.cls_token"):
        assert k in keys, k
    assert not any("_resnet_mean" in k or "_resnet_std" in k for k in keys)        # non-persistent (image_feature_extractor.py:48)
    assert len([k for k in keys if k.startswith("diffuser.") and not k.startswith("diffuser.model.")]) == 13
    model = mk.build_model(cfg_path, seed=123)                                       # other weights
    loaded = torch.load(ckpt, map_location="cpu")
    model.load_state_dict(loaded, strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(v, sd[k]), k


# ------------------------------------------------------------------------------------------------ GPU
def _write_synthetic_folder(folder, n_frames=6, size=(96, 128), with_matches=False):
    from PIL import Image
    from posediffusion_amd import synth
    os.makedirs(folder, exist_ok=True)
    rng = np.random.default_rng(5)
    for k in range(n_frames):
        im = rng.integers(0, 256, size=(size[0], size[1], 3), dtype=np.uint8)
        Image.fromarray(im, "RGB").save(os.path.join(folder, f"frame{k:04d}.png"))
    enc = synth.make_cameras(n_frames, seed=31)
    R = synth._quat_to_R(enc[:, 3:7]).astype(np.float32)
    np.savez(os.path.join(folder, "gt_cameras.npz"), gtR=R, gtT=enc[:, :3].astype(np.float32),
             gtFL=np.exp(enc[:, 7:9] + 1.8).astype(np.float32))
    if with_matches:
        md = synth.make_matches(enc, 224, 224, per_pair=50, seed=31)
        np.savez(os.path.join(folder, "pd_matches.npz"), kp1=md["kp1"], kp2=md["kp2"], i12=md["i12"])


@pytest.mark.gpu
def test_demo_call_sequence_on_synthetic_folder(tmp_path):
    """The call sequence of demo.py:46-133 (not the file: it is absent on the GPU box) on a synthetic image folder,
    through the stand-ins and the drop-in packages in a fresh interpreter: hydra.main + instantiate, image loading,
    strict checkpoint load, forward with and without the GGS partial, camera alignment, ARE."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_synthetic_ckpt as mk
    ckpt = str(tmp_path / "synthetic.pth")
    mk.write_checkpoint(ckpt)
    folder = str(tmp_path / "seq")
    _write_synthetic_folder(folder, n_frames=5, with_matches=True)
    import yaml
    (tmp_path / "conf").mkdir()
    (tmp_path / "conf" / "default.yaml").write_text(yaml.safe_dump({
        "image_folder": folder, "image_size": 224, "ckpt": ckpt, "seed": 0,
        "GGS": {"enable": True, "start_step": 10, "learning_rate": 0.01, "iter_num": 4, "sampson_max": 10, "min_matches": 10,
                "alpha": 0.0001},
        "MODEL": mk.DEFAULT_MODEL_CFG}))
    (tmp_path / "flow.py").write_text('''
import os, numpy as np, torch, hydra
from functools import partial
from omegaconf import OmegaConf
from hydra.utils import instantiate, get_original_cwd
import models
from pytorch3d.renderer.cameras import PerspectiveCameras
from pytorch3d.ops import corresponding_cameras_alignment
from util.utils import seed_all_random_engines
from util.match_extraction import extract_match
from util.load_img_folder import load_and_preprocess_images
from util.geometry_guided_sampling import geometry_guided_sampling
from util.metric import compute_ARE

@hydra.main(config_path="conf", config_name="default")
def flow(cfg):
    device = torch.device("cuda")
    model = instantiate(cfg.MODEL, _recursive_=False)
    images, info = load_and_preprocess_images(os.path.join(get_original_cwd(), cfg.image_folder), cfg.image_size)
    model.load_state_dict(torch.load(cfg.ckpt, map_location=device), strict=True)
    model = model.to(device).eval()
    images = images.to(device)
    outs = {}
    for enable in (False, True):
        seed_all_random_engines(cfg.seed)
        cond_fn = None
        if enable:
            kp1, kp2, i12 = extract_match(image_folder_path=cfg.image_folder, image_info=info)
            cfg.GGS.pose_encoding_type = cfg.MODEL.pose_encoding_type
            md = dict(kp1=kp1, kp2=kp2, i12=i12, img_shape=images.shape)
            cond_fn = partial(geometry_guided_sampling, matches_dict=md, GGS_cfg=OmegaConf.to_container(cfg.GGS))
        with torch.no_grad():
            pred = model(image=images.unsqueeze(0), cond_fn=cond_fn, cond_start_step=cfg.GGS.start_step, training=False)["pred_cameras"]
        gt = np.load(os.path.join(cfg.image_folder, "gt_cameras.npz"))
        gt = PerspectiveCameras(focal_length=gt["gtFL"], R=gt["gtR"], T=gt["gtT"], device=device)
        al = corresponding_cameras_alignment(cameras_src=pred, cameras_tgt=gt, estimate_scale=True, mode="extrinsics", eps=1e-9)
        are = compute_ARE(al.R, gt.R).mean()
        outs[enable] = pred.R.clone()
        print(f"FLOW ggs={enable} cameras={tuple(pred.R.shape)} finite={bool(torch.isfinite(pred.R).all())} ARE={are:.4f}")
    print("FLOW differs", not torch.equal(outs[False], outs[True]))

if __name__ == "__main__":
    flow()
''')
    r = _run(str(tmp_path / "flow.py"), [], cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "FLOW ggs=False cameras=(5, 3, 3) finite=True" in r.stdout
    assert "FLOW ggs=True cameras=(5, 3, 3) finite=True" in r.stdout
