"""The yardstick of the weak-augmentation tests, written out independently of the product: Pillow itself on the numpy-sliced
window, then ``np.flip``; and Detectron2's box rule in float64 (CropTransform, ResizeTransform, HFlip / VFlip transform,
clip to the image, float32 cast, filter_empty_instances at 1e-5).  Neither the product's CPU path nor oracle/resize.py is
used.  Shared by tests/test_weak_augment_host.py (CPU loader) and tests/test_gpu_weak_augment.py (device loader)."""
import os

import numpy as np
from PIL import Image

HOT_YAML = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "configs",
                        "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free.yaml")
SRC_YAML = os.path.join(os.path.dirname(HOT_YAML), "faster_rcnn_VGG_cityscapes_source_new.yaml")

# the loader-level case of both files: eight 96 x 160 frames, short edge uniform in [32, 48], relative_range crop
# [0.6, 0.7], vertical flip.  SEED 3: among the first 16 items at least one loses a box to filter_empty_instances (asserted
# where it is used; found by running the CPU loader, which makes the same draws as the device loader).
LOADER_SEED = 3
FRAME_H, FRAME_W, N_FRAMES, N_BOXES = 96, 160, 8, 6
LOADER_OPTS = ["OUTPUT_DIR", "", "SEED", str(LOADER_SEED), "SFOD.SYNTHETIC.HEIGHT", str(FRAME_H), "SFOD.SYNTHETIC.WIDTH", str(FRAME_W),
               "SFOD.SYNTHETIC.NUM_IMAGES", str(N_FRAMES), "SFOD.SYNTHETIC.BOXES_PER_IMAGE", str(N_BOXES),
               "SOLVER.IMS_PER_BATCH_TARGET", "2", "SOLVER.IMS_PER_BATCH", "2",
               "INPUT.MIN_SIZE_TRAIN", "(32, 48)", "INPUT.MIN_SIZE_TRAIN_SAMPLING", "range",
               "INPUT.CROP.ENABLED", "True", "INPUT.CROP.TYPE", "relative_range", "INPUT.CROP.SIZE", "[0.6, 0.7]",
               "INPUT.RANDOM_FLIP", "vertical"]


def pillow_weak(img_chw, window, out_hw, flip_mode):
    """uint8 numpy [C,H,W] -> flip(PIL.resize(img[:, y0:y0+ch, x0:x0+cw], (w, h), BILINEAR)), channel by channel (Pillow's
    8-bit resample treats the bands of an image independently, so C != 3 needs no image mode of its own)."""
    C, H, W = img_chw.shape
    y0, x0, ch, cw = (0, 0, H, W) if window is None else window
    win = img_chw[:, y0:y0 + ch, x0:x0 + cw]
    h, w = out_hw
    out = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(p)).resize((w, h), Image.BILINEAR)) for p in win])
    if flip_mode == 1:
        out = np.flip(out, axis=2)
    elif flip_mode == 2:
        out = np.flip(out, axis=1)
    return np.ascontiguousarray(out)


def d2_boxes(boxes_native, classes, window, native_hw, out_hw, flip_mode):
    """-> (float32 [m,4], classes [m]): the float64 rule, then the float32 cast, then the 1e-5 filter on float32 extents."""
    b = np.asarray(boxes_native, dtype=np.float64).reshape(-1, 4).copy()
    y0, x0, ch, cw = (0, 0) + tuple(native_hw) if window is None else window
    h, w = out_hw
    x1, y1, x2, y2 = b[:, 0] - x0, b[:, 1] - y0, b[:, 2] - x0, b[:, 3] - y0
    sx, sy = w * 1.0 / cw, h * 1.0 / ch
    x1, x2, y1, y2 = x1 * sx, x2 * sx, y1 * sy, y2 * sy
    if flip_mode == 1:
        x1, x2 = w - x2, w - x1
    elif flip_mode == 2:
        y1, y2 = h - y2, h - y1
    out = np.stack([np.clip(x1, 0, w), np.clip(y1, 0, h), np.clip(x2, 0, w), np.clip(y2, 0, h)], axis=1).astype(np.float32)
    keep = ((out[:, 2] - out[:, 0]) > 1e-5) & ((out[:, 3] - out[:, 1]) > 1e-5)
    return out[keep], np.asarray(classes)[keep]


def check_items_against_the_replay(syn, items, seed):
    """items: the loader's weak dicts (with their recorded ``weak_plan``) -> number of boxes the filter dropped in total.
    The native frame and boxes are regenerated with make_frame (the dataset's recipe), not read from the loader."""
    dropped = 0
    for d in items:
        plan = d["weak_plan"]
        img, boxes, classes = syn.make_frame(d["image_id"], FRAME_H, FRAME_W, N_BOXES, seed=seed)
        assert plan.native_hw == (FRAME_H, FRAME_W)
        ref = pillow_weak(img.numpy(), plan.window, plan.out_hw, plan.flip_mode)
        got = d["image"].cpu().numpy()
        assert got.shape == ref.shape and np.array_equal(got, ref), (d["image_id"], plan)
        rb, rc = d2_boxes(boxes.numpy(), classes.numpy(), plan.window, plan.native_hw, plan.out_hw, plan.flip_mode)
        gb = d["instances"].gt_boxes.tensor.cpu().numpy()
        assert gb.dtype == np.float32 and np.array_equal(gb, rb), (d["image_id"], plan, gb, rb)
        assert np.array_equal(d["instances"].gt_classes.cpu().numpy(), rc)
        assert d["instances"].image_size == tuple(plan.out_hw)
        dropped += N_BOXES - len(rb)
    return dropped
