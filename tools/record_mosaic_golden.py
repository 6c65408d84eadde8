"""Records tests/golden/mosaic_ref.npz: the reference's ``MosaicDetection`` / ``MosaicWQDetection`` / ``MosaicWQNewDetection``
``__getitem__`` (daod/data/mappers/mosaic.py, mosaic_wq.py, mosaic_wq_new.py, loaded by file path behind
oracle/ref_stub/hook.py) run on small hand-sized cases.

Usage: python tools/record_mosaic_golden.py <reference checkout> [out.npz]        (CPU only; no test reads the reference)

Neither cv2, yolox nor skimage is installed where this runs; the tool defines STAND-INS for them:

  * ``yolox``: a ``Dataset`` base whose ``mosaic_getitem`` is the identity decorator, ``get_local_rank`` -> 0,
    ``adjust_box_anns`` (unused by ``__getitem__``), a ``random_affine`` that raises (the reference's call is commented out);
  * ``skimage``: an empty module (imported, never used);
  * ``cv2``: A STAND-IN, NOT OpenCV -- ``resize`` is Pillow's bilinear when up-scaling (and a copy at equal size), and the
    rounded 2x2 mean at the exact half; anything else raises.  So this golden pins everything of the reference's mosaic (tile
    scale, rectangles, paste order, box arithmetic, clipping, what the item reports, where each variant applies its strong
    augmentation) EXCEPT cv2's own arithmetic, which stays unpinned (README, "still parity unpinned");
  * ``build_strong_augmentation`` is replaced by a marker transform, ``ImageOps.invert``: under ``wq_new`` the fill stays
    114, under ``wq`` it becomes 141.

Python's ``random`` is seeded per case; the drawn indices are recorded by the dataset stand-in and stored as inputs.  Stored
per case ``<c>``: ``<c>/tile<k>`` uint8 [3,h0,w0], ``<c>/boxes<k>`` float32 [n,4], ``<c>/classes<k>`` int64 [n] of the four
mapped tiles in paste order, ``<c>/native`` int32 [4,2] = (height, width), ``<c>/indices``; per variant ``<c>/<v>/image``
uint8 [3,H0,W0] (the reference's float32 image holds these integers), ``<c>/<v>/boxes`` float32, ``<c>/<v>/classes``,
``<c>/<v>/hw`` = (height, width) of the item."""
import importlib.util
import os
import random
import sys
import types

import numpy as np
import torch
from PIL import Image, ImageOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = {"mosaic": ("mosaic.py", "MosaicDetection"), "mosaic_wq": ("mosaic_wq.py", "MosaicWQDetection"),
            "mosaic_wq_new": ("mosaic_wq_new.py", "MosaicWQNewDetection")}


def stand_in_resize(img, dsize, interpolation=None):
    w, h = int(dsize[0]), int(dsize[1])
    H, W = img.shape[:2]
    if (h, w) == (H, W):
        return img.copy()
    if h >= H and w >= W:
        return np.asarray(Image.fromarray(img).resize((w, h), Image.BILINEAR))
    if (2 * h, 2 * w) == (H, W):
        c = img.astype(np.uint16)
        return ((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    raise NotImplementedError(f"the cv2 stand-in resizes up or to the exact half, not {H}x{W} -> {h}x{w}")


def install_stand_ins():
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        m.__path__ = []
        sys.modules[name] = m
        return m

    class Dataset:
        def __init__(self, input_dimension, mosaic=True):
            self.input_dim = input_dimension
            self.enable_mosaic = mosaic

        @staticmethod
        def mosaic_getitem(fn):
            return fn

    def random_affine(*a, **k):
        raise AssertionError("random_affine is commented out in the reference's __getitem__")

    def adjust_box_anns(bbox, scale_ratio, padw, padh, w_max, h_max):
        bbox[:, 0::2] = np.clip(bbox[:, 0::2] * scale_ratio + padw, 0, w_max)
        bbox[:, 1::2] = np.clip(bbox[:, 1::2] * scale_ratio + padh, 0, h_max)
        return bbox

    module("cv2", resize=stand_in_resize, INTER_LINEAR=1)
    module("skimage")
    module("skimage.transform", resize=None)
    module("yolox")
    module("yolox.utils", adjust_box_anns=adjust_box_anns, get_local_rank=lambda: 0)
    module("yolox.data")
    module("yolox.data.data_augment", random_affine=random_affine)
    module("yolox.data.datasets")
    module("yolox.data.datasets.datasets_wrapper", Dataset=Dataset)


class MappedSet:
    """Stands in for the mapped training set: ``__getitem__`` returns the mapper's dict (six keys in the order the reference
    unpacks) and records which indices were asked for."""

    def __init__(self, items):
        self.items, self.calls = items, []

    def __len__(self):
        return len(self.items)

    def __getitem__(self, idx):
        from detectron2.structures import Boxes, Instances
        self.calls.append(int(idx))
        tile, boxes, classes, (H, W) = self.items[idx]
        inst = Instances(tuple(tile.shape[1:]))
        inst.gt_boxes = Boxes(torch.from_numpy(boxes.copy()))
        inst.gt_classes = torch.from_numpy(classes.copy())
        return {"file_name": f"{idx}.png", "height": H, "width": W, "image_id": idx, "image": torch.from_numpy(tile.copy()),
                "instances": inst}


def make_item(rng, mapped_hw, native_hw, n_boxes, overshoot=False):
    h0, w0 = mapped_hw
    tile = rng.integers(0, 256, (3, h0, w0), dtype=np.uint8)
    x = np.sort(rng.uniform(0, w0, (n_boxes, 2)), 1)
    y = np.sort(rng.uniform(0, h0, (n_boxes, 2)), 1)
    if overshoot:                       # boxes that leave the frame on every side: the clip changes them
        x = x * 1.6 - 0.3 * w0
        y = y * 1.6 - 0.3 * h0
    boxes = np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], 1).astype(np.float32)
    return tile, boxes, rng.integers(0, 8, n_boxes).astype(np.int64), native_hw


def cases(rng):
    """name -> (items, idx, requirement on the drawn indices)"""
    def same(mapped, native, counts, **kw):
        return [make_item(rng, mapped, native, n, **kw) for n in counts]
    anything = lambda ind: True                                                                     # noqa: E731
    out = {
        "a_exact": (same((16, 24), (32, 48), (3, 1, 2, 4, 2, 3)), 2, anything),
        "b_letterbox_h": (same((18, 30), (32, 52), (2, 3, 1, 2, 4, 1)), 0, anything),
        "c_letterbox_w": (same((16, 30), (32, 66), (1, 2, 3, 2, 1, 2)), 5, anything),
        "d_one_empty": (same((12, 20), (24, 40), (2, 0, 3, 0, 1, 0)), 1,
                        lambda ind: 0 < sum(i in (1, 3, 5) for i in ind) < 4),
        "d_all_empty": (same((12, 20), (24, 40), (0, 0, 0, 0)), 3, anything),
        "e_clip": (same((16, 24), (32, 48), (4, 4, 4, 4, 4), overshoot=True), 4, anything),
        "f_smaller_native": ([make_item(rng, (16, 24), (32, 48), 3)] + same((12, 20), (24, 40), (2, 1, 3, 2, 2)), 0,
                             lambda ind: all(i != 0 for i in ind[1:])),
        "g_identity": (same((20, 36), (20, 36), (2, 2, 1, 3, 2)), 1, anything),
    }
    return out


def main():
    ref = sys.argv[1]
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "mosaic_ref.npz")
    from oracle.ref_stub import hook
    hook.install()
    install_stand_ins()
    mods = {}
    for v, (fname, cls) in VARIANTS.items():
        spec = importlib.util.spec_from_file_location("ref_" + v, os.path.join(ref, "daod", "data", "mappers", fname))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build_strong_augmentation = lambda cfg, is_train: ImageOps.invert            # the marker transform
        mods[v] = getattr(mod, cls)
    store = {}
    rng = np.random.default_rng(20241020)
    for name, (items, idx, ok) in cases(rng).items():
        seed = 0
        while True:                       # the first seed whose draws make the case what its name says
            random.seed(seed)
            probe = MappedSet(items)
            mods["mosaic"](probe, None)[idx]
            if ok(probe.calls[1:]):
                break
            seed += 1
        indices = probe.calls[1:]         # calls[0] is the reference's extra D[idx] (it reads only height / width)
        assert probe.calls[0] == idx and indices[0] == idx and len(indices) == 4
        for k, i in enumerate(indices):
            tile, boxes, classes, _ = items[i]
            assert tile.shape[1] <= 24 and tile.shape[2] <= 40
            store[f"{name}/tile{k}"], store[f"{name}/boxes{k}"], store[f"{name}/classes{k}"] = tile, boxes, classes
        store[f"{name}/native"] = np.array([items[i][3] for i in indices], np.int32)
        store[f"{name}/indices"] = np.array(indices, np.int32)
        for v, cls in mods.items():
            random.seed(seed)
            ds = MappedSet(items)
            d = cls(ds, None)[idx]
            assert ds.calls[1:] == indices
            img = d["image"].numpy()
            assert img.dtype == np.float32 and np.array_equal(img, np.round(img)) and img.min() >= 0 and img.max() <= 255
            b = d["instances"].gt_boxes.tensor
            assert b.dtype == torch.float32
            store[f"{name}/{v}/image"] = img.astype(np.uint8)
            store[f"{name}/{v}/boxes"] = b.numpy().reshape(-1, 4)
            store[f"{name}/{v}/classes"] = d["instances"].gt_classes.numpy().astype(np.int64)
            store[f"{name}/{v}/hw"] = np.array([d["height"], d["width"]], np.int32)
            assert tuple(d["instances"].image_size) == (d["height"], d["width"])
    hook.uninstall()
    np.savez_compressed(out_path, **store)
    print(out_path, os.path.getsize(out_path), "bytes;", len(store), "arrays")


if __name__ == "__main__":
    main()
