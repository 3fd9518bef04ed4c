"""No GPU: the yardstick of the training-image kernels (tests/train_images_checks.py) against torch's own antialiased resize in fp64 and
PIL's crop, the C-ABI of include/pd_engine_images.h, the draws, and the host half of the drop-in Co3dDataset -- against the reference's
datasets/co3d_v2.py executed in place where that tree exists, and on a synthetic Co3D tree always."""
import ctypes as C
import importlib
import os
import re
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

import train_images_checks as IC
from oracle import ref_stubs
from posediffusion_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_FILE = os.path.join(ref_stubs.REF_PKG, "datasets", "co3d_v2.py")     # where the reference tree lies, if it is there at all


# ---- yardstick ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", [1, 2, 5, 31, 32, 33, 64, 97, 225, 320, 500])
@pytest.mark.parametrize("S", [32, 224])
def test_resize_yardstick_is_torch_antialiased_bilinear_in_fp64(side, S):
    crop = IC.picture(side, side, seed=side)
    ours, _ = IC.resize(crop, S)
    x = torch.from_numpy(crop).permute(2, 0, 1).double()[None] / 255
    ref = F.interpolate(x, size=(S, S), mode="bilinear", antialias=True, align_corners=False)[0]
    assert (ours - ref).abs().max().item() <= 1e-14


@pytest.mark.parametrize("side", [1, 2, 5, 31, 32, 33, 64, 97, 225, 320, 1280, 6144])
@pytest.mark.parametrize("S", [1, 32, 224])
def test_integer_weights_are_the_closed_form(side, S):
    a, _ = IC.aa_weights(side, S)
    b = IC.aa_weights_integer(side, S)
    # the closed form rounds its centres (up to `side` in magnitude) and distances in fp64; the integer form rounds once, at the division
    assert (a - b).abs().max().item() <= 16 * max(side, S) * 2.0 ** -53
    assert torch.allclose(b.sum(1), torch.ones(S, dtype=torch.float64), atol=1e-15)


@pytest.mark.parametrize("name,H,W,box", IC.BORDER_CASES + [("inside", 80, 100, (10, 20, 40))])
@pytest.mark.parametrize("fill", [0, 255])
def test_crop_yardstick_is_pil_crop(name, H, W, box, fill):
    img = IC.case_picture(name, H, W)
    x0, y0, side = box
    ours = IC.padded_crop(img, x0, y0, side, fill)
    if fill == 0:
        ref = np.array(Image.fromarray(img).crop((x0, y0, x0 + side, y0 + side)))
    else:                                                        # the reference's white_bg path
        canvas = Image.new("RGB", (side, side), (255, 255, 255))
        canvas.paste(Image.fromarray(img), (-x0, -y0))
        ref = np.array(canvas)
    assert np.array_equal(ours, ref)


def test_colour_ops_against_torchvision():
    tvf = pytest.importorskip("torchvision.transforms.functional")
    x, _ = IC.resize(IC.palette(32), 32)
    for f in IC.FACTOR_SETS:
        e = dict(brightness=f[0], contrast=f[1], saturation=f[2], hue=f[3])
        for op, fn in enumerate((tvf.adjust_brightness, tvf.adjust_contrast, tvf.adjust_saturation, tvf.adjust_hue)):
            assert (IC.colour_op(x, op, e) - fn(x, f[op])).abs().max().item() <= 1e-12
    assert (IC.grey(x) - tvf.rgb_to_grayscale(x)[0]).abs().max().item() <= 1e-12


def test_colour_yardstick_properties():
    """What holds whatever torchvision is installed: identity factors change nothing, hue by a whole turn is the identity up to rounding,
    greys stay grey under every operation, grayscale and erase do what their names say."""
    x, _ = IC.resize(IC.palette(32), 32)
    ident = dict(brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0)
    for op in range(3):
        assert torch.equal(IC.colour_op(x, op, ident), x)
    assert (IC.colour_op(x, 3, ident) - x).abs().max().item() <= 1e-14
    for f in IC.FACTOR_SETS:
        e = dict(brightness=f[0], contrast=f[1], saturation=f[2], hue=f[3])
        for op in range(4):
            y = IC.colour_op(x, op, e)
            assert y.min().item() >= 0.0 and y.max().item() <= 1.0
            g = y[:, 1, 0:4]                                       # the block of (128, 128, 128)
            assert (g[0] - g[1]).abs().max().item() <= 1e-15 and (g[0] - g[2]).abs().max().item() <= 1e-15
    y = IC.apply_colour(x, dict(jitter=0, grayscale=1, erase=(1, 2, 3, 4)))
    assert torch.equal(y[0], y[1]) and torch.equal(y[0], y[2]) and float(y[:, 1:4, 2:6].abs().max()) == 0.0 and float(y[0, 0].max()) > 0.0


# ---- C-ABI ----------------------------------------------------------------------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, "include", "pd_engine_images.h")) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


def test_header_signatures_structs_and_makefile_agree():
    hdr = _header()
    assert set(re.findall(r"\b(pd_\w+)\s*\(", hdr)) == set(_lib.IMAGE_SIGNATURES) == {"pd_train_images", "pd_train_images_workspace_bytes"}
    others = (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) | set(_lib.TRAIN_SIGNATURES) | set(_lib.VIT_TRAIN_SIGNATURES) |
              set(_lib.OPTIM_SIGNATURES) | set(_lib.CAMERA_SIGNATURES))
    assert not set(_lib.IMAGE_SIGNATURES) & others
    for name, (_, args) in _lib.IMAGE_SIGNATURES.items():
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == len(args), name
    for struct, cls in (("pd_img_frame", _lib.pd_img_frame), ("pd_img_colour", _lib.pd_img_colour)):
        body = re.search(r"typedef struct \{([^}]*)\} " + struct + ";", hdr, flags=re.S).group(1)
        names = [n.split("[")[0] for decl in re.findall(r"(?:int64_t|int32_t|float) ([^;]+);", body) for n in re.split(r",\s*", decl)]
        assert names == [n for n, _ in cls._fields_], struct
    assert C.sizeof(_lib.pd_img_frame) == 32 and C.sizeof(_lib.pd_img_colour) == 56
    codes = {k: int(v) for k, v in re.findall(r"#define (PD_IMG_\w+) (\d+)", hdr)}
    assert codes == {k: getattr(_lib, k) for k in ("PD_IMG_MAX_SIDE", "PD_IMG_MAX_SIZE", "PD_IMG_MAX_FRAMES", "PD_IMG_OK", "PD_IMG_BAD_SIDE", "PD_IMG_BAD_SIZE",
                                                  "PD_IMG_BAD_COLOUR", "PD_IMG_BAD_ORDER", "PD_IMG_BAD_ERASE")}
    with open(os.path.join(ROOT, "posediffusion_amd", "csrc", "Makefile")) as fh:
        mk = fh.read()
    assert "build/pd_images.o" in mk and "pd_engine_images.h" in mk


def test_symbols_are_exported_and_workspace_bytes():
    assert os.path.isfile(_lib.LIB_PATH), "run `python -c 'import __graft_entry__ as g; g.build()'` first"
    lib = _lib.load()
    assert lib.pd_train_images.argtypes == _lib.IMAGE_SIGNATURES["pd_train_images"][1]
    ws = lib.pd_train_images_workspace_bytes
    assert ws(0, 224) == 0 and ws(-1, 224) == 0 and ws(3, 0) == 0 and ws(3, _lib.PD_IMG_MAX_SIZE + 1) == 0 and ws(_lib.PD_IMG_MAX_FRAMES + 1, 32) == 0
    assert ws(1, 224) > 0 and ws(7, 224) == 7 * ws(1, 224) and ws(1, 224) % 8 == 0 and ws(1, _lib.PD_IMG_MAX_SIZE) > 0 and ws(1, 1) == 8


def test_package_names_and_cpu_refusal():
    import posediffusion_amd
    from posediffusion_amd import images, synth
    assert posediffusion_amd.prepare_training_images is images.prepare_training_images
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            images.prepare_training_images([np.zeros((4, 4, 3), np.uint8)], [[0, 0, 4, 4]], image_size=4)
    synth._dropin()
    ds = importlib.import_module("datasets.co3d_v2")
    assert ds.__file__.startswith(posediffusion_amd.DROPIN_PATH)
    assert len(ds.TRAINING_CATEGORIES) == 41 and len(ds.TEST_CATEGORIES) == 10 and ds.DEBUG_CATEGORIES == ["apple", "teddybear"]
    import inspect
    assert list(inspect.signature(ds.Co3dDataset.__init__).parameters)[1:] == [
        "category", "split", "transform", "debug", "random_aug", "jitter_scale", "jitter_trans", "min_num_images", "img_size", "eval_time",
        "normalize_cameras", "first_camera_transform", "mask_images", "CO3D_DIR", "CO3D_ANNOTATION_DIR", "foreground_crop", "center_box",
        "sort_by_filename", "compute_optical", "color_aug", "erase_aug"]


# ---- draws ----------------------------------------------------------------------------------------------------------------------------
def test_draw_colour_ranges_order_and_reproducibility():
    from posediffusion_amd import images
    g = torch.Generator().manual_seed(3)
    draws = [images.draw_colour(erase=dict(image_size=32, p=0.5), generator=g) for _ in range(400)]
    g = torch.Generator().manual_seed(3)
    assert draws == [images.draw_colour(erase=dict(image_size=32, p=0.5), generator=g) for _ in range(400)]
    jit = [d for d in draws if d["jitter"]]
    assert 0.5 < len(jit) / 400 < 0.8 and 0.05 < sum(d["grayscale"] for d in draws) / 400 < 0.3
    assert {tuple(sorted(d["order"])) for d in jit} == {(0, 1, 2, 3)} and len({d["order"] for d in jit}) > 12
    for d in jit:
        assert 0.6 <= d["brightness"] <= 1.4 and 0.6 <= d["contrast"] <= 1.4 and 0.8 <= d["saturation"] <= 1.2 and -0.1 <= d["hue"] <= 0.1
    for d in draws:
        if not d["jitter"]:
            assert (d["brightness"], d["contrast"], d["saturation"], d["hue"]) == (1.0, 1.0, 1.0, 0.0)
        top, left, h, w = d["erase"]
        assert (h == 0 and w == 0) or (0 < h < 32 and 0 < w < 32 and 0 <= top <= 32 - h and 0 <= left <= 32 - w)
    assert any(d["erase"][2] for d in draws)
    e = images.colour_entry(jit[0])
    assert list(e.order) == list(jit[0]["order"]) and e.jitter == 1 and abs(e.hue - jit[0]["hue"]) < 1e-7


# ---- the reference's file, executed in place -----------------------------------------------------------------------------------------------
def _load_reference_dataset_module():
    """datasets/co3d_v2.py of the reference tree on top of stand-ins for what it imports and this machine lacks; util.camera_transform is
    the drop-in's (checked bitwise against the reference's by tests/test_normalize_checks_cpu.py)."""
    from posediffusion_amd import synth
    synth._dropin()
    ct = importlib.import_module("util.camera_transform")
    tv, tr, fn = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms"), types.SimpleNamespace()
    fn.crop = lambda image, top, left, height, width: image.crop((left, top, left + width, top + height))
    tr.functional, tv.transforms = fn, tr
    p3, p3r = types.ModuleType("pytorch3d"), types.ModuleType("pytorch3d.renderer")
    p3r.PerspectiveCameras = object
    nc = types.ModuleType("util.normalize_cameras")
    nc.normalize_cameras = None
    tq = types.ModuleType("tqdm")
    stubs = {"torchvision": tv, "torchvision.transforms": tr, "pytorch3d": p3, "pytorch3d.renderer": p3r, "util.normalize_cameras": nc,
             "util.camera_transform": ct, "tqdm": tq}
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    try:
        spec = importlib.util.spec_from_file_location("_ref_co3d_v2", REF_FILE)
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return m


@pytest.mark.skipif(not os.path.isfile(REF_FILE), reason="reference tree not present (GPU box)")
def test_draws_and_host_half_against_the_reference_executed_in_place(tmp_path):
    from posediffusion_amd import images
    ref = _load_reference_dataset_module()
    ds_mod = importlib.import_module("datasets.co3d_v2")
    assert ds_mod.TRAINING_CATEGORIES == ref.TRAINING_CATEGORIES and ds_mod.TEST_CATEGORIES == ref.TEST_CATEGORIES
    rng = np.random.default_rng(0)
    for k in range(50):
        bbox = np.concatenate((rng.integers(0, 200, 2), rng.integers(210, 900, 2)))
        for dt in (np.int64, np.float32):
            a, b = ds_mod.square_bbox(bbox.astype(dt)), ref.square_bbox(bbox.astype(dt))
            assert a.dtype == b.dtype and np.array_equal(a, b)
        me = types.SimpleNamespace(jitter_scale=[0.8, 1.2], jitter_trans=[-0.07, 0.07])
        np.random.seed(k)
        r = ref.Co3dDataset._jitter_bbox(me, bbox)
        np.random.seed(k)
        o = images.draw_bbox_jitter(bbox, me.jitter_scale, me.jitter_trans)
        assert o.dtype == r.dtype and np.array_equal(o, r) and o[2] - o[0] == o[3] - o[1]
    kw = IC.write_co3d_tree(str(tmp_path))
    for center_box in (True, False):
        ours = ds_mod.Co3dDataset(center_box=center_box, color_aug=False, **kw)
        theirs = ref.Co3dDataset(center_box=center_box, color_aug=False, transform=lambda im: torch.zeros(3, 2, 2), **kw)
        assert ours.sequence_list == theirs.sequence_list and ours.low_quality_translations == theirs.low_quality_translations
        for index in range(len(ours)):
            np.random.seed(100 + index)
            a = ours[(index, 4)]
            np.random.seed(100 + index)
            b = theirs[(index, 4)]
            for key in ("R", "T", "fl", "pp", "crop_params", "ind"):
                assert a[key].dtype == b[key].dtype and torch.equal(a[key], b[key]), key
            assert a["seq_id"] == b["seq_id"] and a["category"] == b["category"] and a["n"] == b["n"]


def test_host_half_on_a_synthetic_tree(tmp_path):
    from posediffusion_amd import synth
    synth._dropin()
    ds_mod = importlib.import_module("datasets.co3d_v2")
    kw = IC.write_co3d_tree(str(tmp_path))
    ds = ds_mod.Co3dDataset(**kw)
    assert ds.sequence_list == ["seq0", "seq1"] and ds.low_quality_translations == ["far"] and len(ds) == 2
    assert set(ds.rotations["seq0"][0]) == {"filepath", "bbox", "R", "T", "focal_length", "principal_point"}
    np.random.seed(1)
    torch.manual_seed(1)
    s = ds[(1, 3)]
    assert s["seq_id"] == "seq1" and s["category"] == "apple" and s["n"] == 6 and len(set(s["ind"].tolist())) == 3
    assert len(s["frames"]) == 3 and all(f.dtype == np.uint8 and f.shape == (75, 50, 3) for f in s["frames"])
    b = s["boxes"]
    assert b.shape == (3, 4) and np.array_equal(b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]) and s["fill"] == 0
    assert s["R"].shape == (3, 3, 3) and s["T"].shape == (3, 3) and s["fl"].shape == (3, 2) and s["pp"].shape == (3, 2)
    assert s["crop_params"].shape == (3, 3) and s["crop_params"].dtype == torch.float32 and isinstance(s["colour"], dict)
    for k in range(3):                                               # crop_params: (-cc, 2 side / min(h, w)) of the drawn box
        cx, cy, side = (b[k, 0] + b[k, 2]) / 2, (b[k, 1] + b[k, 3]) / 2, b[k, 2] - b[k, 0]
        want = torch.tensor([-(2 * cx / 50 - 1), -(2 * cy / 50 - 1), 2 * side / 50]).float()
        assert torch.equal(s["crop_params"][k], want)
    frame0 = np.array(Image.open(os.path.join(str(tmp_path), ds.rotations["seq1"][int(s["ind"][0])]["filepath"])).convert("RGB"))
    assert np.array_equal(s["frames"][0], frame0)
    ev = ds_mod.Co3dDataset(eval_time=True, sort_by_filename=True, **kw).get_data(index=0, ids=(3, 1))
    assert ev["colour"] is None and np.array_equal(ev["boxes"], np.array([[15, 0, 75, 60]] * 2))   # the centre box of a 60 x 90 picture
    with pytest.raises(NotImplementedError):
        ds_mod.Co3dDataset(transform=lambda x: x, **kw)
    with pytest.raises(ValueError, match="CO3D_DIR"):
        ds_mod.Co3dDataset(**dict(kw, CO3D_DIR=None))


# ---- kernel resources ---------------------------------------------------------------------------------------------------------------------
def test_image_kernels_do_not_spill_and_keep_their_lds(tmp_path):
    """hipcc's own resource remarks (cross-compiled for gfx950): no spill, no scratch; the resize kernel's LDS is exactly its 64 KB carve
    (a private array the compiler moves to LDS would show up here: two workgroups per CU need 80 KB each at the most)."""
    import shutil
    import subprocess
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not installed")
    src = os.path.join(ROOT, "posediffusion_amd", "csrc", "pd_images.hip")
    out = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", "-Rpass-analysis=kernel-resource-usage",
                          "-c", src, "-o", str(tmp_path / "pd_images.o")], capture_output=True, text=True, timeout=900)
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
    assert len(kernels) == 2, sorted(kernels)
    for name, r in kernels.items():
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["ScratchSize"] == 0, (name, r)
        assert r["LDS Size"] == (65536 if "resize" in name else 0), (name, r)
