"""Drop-in ``datasets.co3d_v2`` (pose_diffusion/datasets/co3d_v2.py): ``Co3dDataset`` with the reference's constructor arguments, plus
``square_bbox`` and the category lists, written from the behaviour.

DataLoader workers cannot touch the GPU, so the reference's ``get_data`` is split in two:

* the HOST half -- ``__getitem__((index, n_per_seq))`` / ``get_data(...)`` -- reads the annotation, decodes the frames with PIL, draws
  the frame ids, the jittered boxes and the sequence's colour parameters, adjusts the intrinsics and computes ``crop_params``.  It
  returns CPU data only: the decoded ``uint8`` frames and their boxes in place of the reference's transformed ``image``.  Use
  ``collate_fn=list`` (or any collate that keeps the samples as a list).
* the DEVICE half -- ``Co3dDataset.finish_batch(samples, device)``, run in the main process -- makes ONE ``prepare_training_images``
  launch for all frames of the batch (crop, antialiased resize, colour draw) and, with ``normalize_cameras=True``, one
  ``normalize_cameras_batch`` launch, and returns the reference's collated batch: ``image`` [B, N, 3, S, S], ``R`` [B, N, 3, 3], ``T``
  [B, N, 3], ``fl`` / ``pp`` [B, N, 2], ``crop_params`` [B, N, 3] (``R_original`` / ``T_original`` with ``normalize_cameras=True``),
  ``seq_id``, ``category`` (lists), ``n`` [B], ``ind`` [B, N].

Limits that raise and do not fall back: a ``transform`` other than the default (ToTensor + antialiased Resize to ``img_size``) raises
``NotImplementedError``; the sequences of one batch hold the same number of frames (what the reference's sampler yields).
``mask_images=True`` composites the mask on the host, as the reference does, and crops with a white border (``fill = 255``)."""
import gzip
import json
import os.path as osp

import numpy as np
import torch
from PIL import Image, ImageFile
from torch.utils.data import Dataset

from posediffusion_amd import images as _img
from util.camera_transform import adjust_camera_to_bbox_crop_, adjust_camera_to_image_scale_

Image.MAX_IMAGE_PIXELS = None
ImageFile.LOAD_TRUNCATED_IMAGES = True


class Co3dDataset(Dataset):
    def __init__(self, category=("all",), split="train", transform=None, debug=False, random_aug=True, jitter_scale=[0.8, 1.2],
                 jitter_trans=[-0.07, 0.07], min_num_images=50, img_size=224, eval_time=False, normalize_cameras=False,
                 first_camera_transform=True, mask_images=False, CO3D_DIR=None, CO3D_ANNOTATION_DIR=None, foreground_crop=True,
                 center_box=True, sort_by_filename=False, compute_optical=False, color_aug=True, erase_aug=False):
        if transform is not None:
            raise NotImplementedError("Co3dDataset: only the default transform (ToTensor + antialiased Resize to img_size) runs on the "
                                      "engine; a custom transform is not supported")
        if "seen" in category:
            category = TRAINING_CATEGORIES
        if "unseen" in category:
            category = TEST_CATEGORIES
        if "all" in category:
            category = TRAINING_CATEGORIES + TEST_CATEGORIES
        self.category = sorted(category)
        if split not in ("train", "test"):
            raise ValueError(f"split must be 'train' or 'test' (got {split!r})")
        if CO3D_DIR is None:
            raise ValueError("CO3D_DIR is not specified")
        self.CO3D_DIR, self.CO3D_ANNOTATION_DIR = CO3D_DIR, CO3D_ANNOTATION_DIR
        self.center_box, self.split_name, self.min_num_images, self.foreground_crop = center_box, split, min_num_images, foreground_crop
        self.low_quality_translations, self.rotations, self.category_map = [], {}, {}
        keys = ("filepath", "bbox", "R", "T", "focal_length", "principal_point")
        for c in self.category:
            with gzip.open(osp.join(self.CO3D_ANNOTATION_DIR, f"{c}_{split}.jgz"), "r") as fin:
                annotation = json.loads(fin.read())
            for seq_name, seq_data in annotation.items():
                if len(seq_data) < min_num_images:
                    continue
                self.category_map[seq_name] = c
                if any(d["T"][0] + d["T"][1] + d["T"][2] > 1e5 for d in seq_data):     # translations that are not ridiculous
                    self.low_quality_translations.append(seq_name)
                    continue
                self.rotations[seq_name] = [{k: d[k] for k in keys} for d in seq_data]
        self.sequence_list = list(self.rotations.keys())
        self.split, self.debug, self.sort_by_filename = split, debug, sort_by_filename
        self.transform = None
        if random_aug and not eval_time:
            self.jitter_scale, self.jitter_trans = jitter_scale, jitter_trans
        else:
            self.jitter_scale, self.jitter_trans = [1, 1], [0, 0]
        self.img_size, self.eval_time = img_size, eval_time
        self.normalize_cameras, self.first_camera_transform = normalize_cameras, first_camera_transform
        self.mask_images, self.compute_optical, self.color_aug, self.erase_aug = mask_images, compute_optical, color_aug, erase_aug

    def __len__(self):
        return len(self.sequence_list)

    def _jitter_bbox(self, bbox):
        return _img.draw_bbox_jitter(bbox, self.jitter_scale, self.jitter_trans)

    def __getitem__(self, idx_N):
        """``idx_N`` = (index, n_per_seq), as the reference's DynamicBatchSampler yields it: ``n_per_seq`` distinct frames drawn from
        numpy's generator."""
        index, n_per_seq = idx_N
        n_available = len(self.rotations[self.sequence_list[index]])
        return self.get_data(index=index, ids=np.random.choice(n_available, n_per_seq, replace=False))

    def _decode(self, anno, category, sequence_name):
        """One frame as uint8 [H, W, 3]; with ``mask_images`` everything outside the foreground mask (> 125, brought to the frame's size
        by PIL's default resize) is white."""
        path = osp.join(self.CO3D_DIR, anno["filepath"])
        rgb = np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)
        if self.mask_images:
            stem = osp.basename(anno["filepath"].replace(".jpg", ".png"))
            alpha = Image.open(osp.join(self.CO3D_DIR, category, sequence_name, "masks", stem)).convert("L")
            if alpha.size != (rgb.shape[1], rgb.shape[0]):
                alpha = alpha.resize((rgb.shape[1], rgb.shape[0]))
            rgb = np.where((np.asarray(alpha) > 125)[:, :, None], rgb, np.uint8(255))
        return path, rgb

    def _box_of(self, anno, height, width):
        """The frame's crop box before the jitter: the centred largest square (``center_box``) or the annotated box."""
        if not self.center_box:
            return np.array(anno["bbox"])
        short = min(height, width)
        x0, y0 = (width - short) // 2, (height - short) // 2
        return np.array([x0, y0, x0 + short, y0 + short])

    def get_data(self, index=None, sequence_name=None, ids=(0, 1), no_images=False, return_path=False):
        """The host half: CPU data of one sequence's frames ``ids`` (see the module docstring).  Per frame, in frame order: decode, then
        one box draw; after all frames one colour draw."""
        if sequence_name is None:
            sequence_name = self.sequence_list[index]
        metadata, category = self.rotations[sequence_name], self.category_map[sequence_name]
        annos = [metadata[i] for i in ids]
        if self.sort_by_filename:
            annos.sort(key=lambda a: a["filepath"])
        target_wh = torch.FloatTensor([self.img_size, self.img_size])
        paths, frames, boxes, fls, pps = [], [], [], [], []
        for anno in annos:
            path, rgb = self._decode(anno, category, sequence_name)
            height, width = rgb.shape[:2]
            box = self._box_of(anno, height, width)
            if not self.eval_time:
                box = self._jitter_bbox(box)
            # intrinsics of the crop, then of the crop resized to img_size (util.camera_transform, the datasets' helpers)
            wh = box[2:] - box[:2]
            fl, pp = adjust_camera_to_bbox_crop_(torch.tensor(anno["focal_length"]), torch.tensor(anno["principal_point"]),
                                                 torch.FloatTensor([width, height]), torch.FloatTensor(np.concatenate([box[:2], wh])))
            fl, pp = adjust_camera_to_image_scale_(fl, pp, torch.FloatTensor(wh), target_wh)
            paths.append(path), frames.append(rgb), boxes.append(np.asarray(box, dtype=np.int64)), fls.append(fl), pps.append(pp)
        boxes = np.stack(boxes)
        # crop_params per frame: minus the box centre and the box width, in units of half the frame's shorter side, centre relative to 1
        short = np.array([min(f.shape[0], f.shape[1]) for f in frames], dtype=np.float64)
        params = np.stack([1 - (boxes[:, 0] + boxes[:, 2]) / short, 1 - (boxes[:, 1] + boxes[:, 3]) / short,
                           2 * (boxes[:, 2] - boxes[:, 0]) / short], axis=1)
        colour = None
        if self.color_aug and not self.eval_time:
            erase = dict(image_size=self.img_size, p=0.1, scale=(0.02, 0.33), ratio=(0.3, 3.3)) if self.erase_aug else None
            colour = _img.draw_colour(brightness=0.4, contrast=0.4, saturation=0.2, hue=0.1, p_jitter=0.65, p_gray=0.15, erase=erase)
        sample = {"seq_id": sequence_name, "category": category, "n": len(metadata), "ind": torch.tensor(ids),
                  "R": torch.tensor([a["R"] for a in annos]), "T": torch.tensor([a["T"] for a in annos]),
                  "fl": torch.stack(fls), "pp": torch.stack(pps), "crop_params": torch.from_numpy(params).float(),
                  "frames": None if no_images else frames, "boxes": boxes, "colour": colour, "fill": 255 if self.mask_images else 0}
        return (sample, paths) if return_path else sample

    def finish_batch(self, samples, device=None):
        """The device half: ``samples`` (a list of what the host half returned) -> the reference's collated batch on ``device``."""
        from posediffusion_amd.cameras import normalize_cameras_batch
        samples = list(samples)
        n = {len(s["boxes"]) for s in samples}
        if len(n) != 1:
            raise ValueError(f"finish_batch: the sequences of one batch must hold the same number of frames (got {sorted(n)})")
        B, N, S = len(samples), n.pop(), self.img_size
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        frames = [fr for s in samples for fr in s["frames"]]
        seq_of_frame = [b if samples[b]["colour"] is not None else -1 for b in range(B) for _ in range(N)]
        images, _ = _img.prepare_training_images(frames, np.concatenate([s["boxes"] for s in samples]), image_size=S,
                                                 sequence_of_frame=seq_of_frame, colour=[s["colour"] for s in samples],
                                                 fill=samples[0]["fill"], device=dev)
        batch = {"seq_id": [s["seq_id"] for s in samples], "category": [s["category"] for s in samples],
                 "n": torch.tensor([s["n"] for s in samples]), "ind": torch.stack([s["ind"] for s in samples]),
                 "image": images.view(B, N, 3, S, S), "crop_params": torch.stack([s["crop_params"] for s in samples]).to(dev),
                 "fl": torch.stack([s["fl"] for s in samples]).to(dev), "pp": torch.stack([s["pp"] for s in samples]).to(dev)}
        R, T = torch.stack([s["R"] for s in samples]).to(dev), torch.stack([s["T"] for s in samples]).to(dev)
        if self.normalize_cameras:
            res = normalize_cameras_batch(R, T, compute_optical=bool(self.compute_optical), first_camera=self.first_camera_transform,
                                          on_degenerate="status")
            status = res.status.cpu().tolist()
            if any(status):
                raise RuntimeError(f"Error in normalizing cameras (status per sequence {status}): camera scale was 0, or the cameras "
                                   "cannot be normalised")
            batch["R"], batch["T"], batch["R_original"], batch["T_original"] = res.R, res.T, R, T
            if torch.any(torch.isnan(batch["T"])):
                raise RuntimeError(f"NaN translation after normalisation in {batch['seq_id']}")
        else:
            batch["R"], batch["T"] = R, T
        return batch


def square_bbox(bbox, padding=0.0, astype=None):
    """The square xyxy box around ``bbox`` (xyxy): same centre, half side = the larger half extent times (1 + padding); the result has the
    type of the box's entries unless ``astype`` names another."""
    return _img.square_box(bbox, padding, type(bbox[0]) if astype is None else astype)


TRAINING_CATEGORIES = [
    "apple", "backpack", "banana", "baseballbat", "baseballglove", "bench", "bicycle", "bottle", "bowl", "broccoli", "cake", "car", "carrot",
    "cellphone", "chair", "cup", "donut", "hairdryer", "handbag", "hydrant", "keyboard", "laptop", "microwave", "motorcycle", "mouse",
    "orange", "parkingmeter", "pizza", "plant", "stopsign", "teddybear", "toaster", "toilet", "toybus", "toyplane", "toytrain", "toytruck",
    "tv", "umbrella", "vase", "wineglass",
]

TEST_CATEGORIES = ["ball", "book", "couch", "frisbee", "hotdog", "kite", "remote", "sandwich", "skateboard", "suitcase"]

DEBUG_CATEGORIES = ["apple", "teddybear"]
