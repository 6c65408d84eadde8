"""Test-time augmentation (``TEST.AUG``) restated in numpy from Detectron2's published source: ``DatasetMapperTTA``,
``GeneralizedRCNNWithTTA._get_augmented_boxes`` / ``_merge_detections`` and ``fast_rcnn_inference_single_image``.  d2 is not
installed here; nothing below calls the library.  Greedy NMS is oracle/box_ops.py's.

Per input dict:
  1. the starting image is the input's ``"image"`` tensor (h, w); ``pre = ResizeTransform(H0, W0 -> h, w)`` when
     ``(h, w) != (height, width)``, else no transform;
  2. for every ``s`` in MIN_SIZES, in order: ``[ResizeShortestEdge(s, MAX_SIZE)]``, then, with FLIP, ``[that resize, HFlip]``;
     the output size is ``get_output_shape``'s; the resize is Pillow bilinear on uint8, the flip mirrors columns;
  3. every augmented tensor goes through the model without post-processing;
  4. its boxes go through the inverse transform list in reverse order, each ``Transform.apply_box`` on the four corners with
     min / max over them, in float32: ``x -> w_a - x``; ``* (w / w_a, h / h_a)``; ``* (W0 / w, H0 / h)`` -- numpy multiplies a
     float32 array by a Python float as by that float rounded to float32;
  5. all boxes / scores / classes are concatenated in augmentation order and ``fast_rcnn_inference_single_image`` runs with
     score threshold 1e-8 on ``[N, K + 1]`` scores that hold each detection's score in its class column.

``fault`` plants one wrong rule (tests/test_tta_host.py checks that the edge cases tell each from the definition):
"ratio_order" multiplies by the two ratios in the other order, "ratio_fused" by their float32 product at once, "unflip_w"
mirrors about the test tensor's width instead of the augmented one's, "ge" keeps ``score >= 1e-8``.
"""
import numpy as np
import torch

from oracle import box_ops as OB

F32 = np.float32
SCORE_THRESH = 1e-8
FAULTS = ("ratio_order", "ratio_fused", "unflip_w", "ge")


# ---- 2. the augmentations ----------------------------------------------------------------------------------------------------
def output_shape(h, w, short, max_size):
    """d2 ResizeShortestEdge.get_output_shape"""
    scale = short * 1.0 / min(h, w)
    if h < w:
        newh, neww = short, scale * w
    else:
        newh, neww = scale * h, short
    if max(newh, neww) > max_size:
        scale = max_size * 1.0 / max(newh, neww)
        newh, neww = newh * scale, neww * scale
    return int(newh + 0.5), int(neww + 0.5)


def augmentations(h, w, H0, W0, min_sizes, max_size, flip):
    """-> list of dicts in d2's order: ``size`` (h_a, w_a), ``flip``, ``transforms``: the forward list as tuples
    ("resize", h_from, w_from, h_to, w_to) / ("hflip", width)"""
    pre = [("resize", H0, W0, h, w)] if (h, w) != (H0, W0) else []
    out = []
    for s in min_sizes:
        ha, wa = output_shape(h, w, s, max_size)
        rs = ("resize", h, w, ha, wa)
        out.append({"size": (ha, wa), "flip": False, "transforms": pre + [rs]})
        if flip:
            out.append({"size": (ha, wa), "flip": True, "transforms": pre + [rs, ("hflip", wa)]})
    return out


def augmented_image(img_chw_u8, aug):
    """the augmented uint8 tensor of one augmentation (numpy [C,H,W]) with Pillow"""
    from PIL import Image
    arr = np.ascontiguousarray(np.asarray(img_chw_u8).transpose(1, 2, 0))
    ha, wa = aug["size"]
    if (ha, wa) != arr.shape[:2]:
        arr = np.asarray(Image.fromarray(arr).resize((wa, ha), Image.BILINEAR))
    if aug["flip"]:
        arr = arr[:, ::-1]
    return np.ascontiguousarray(arr.transpose(2, 0, 1))


# ---- 4. Transform.apply_box ---------------------------------------------------------------------------------------------------
def _apply_coords(t, coords):
    coords = coords.copy()
    if t[0] == "hflip":
        coords[:, 0] = t[1] - coords[:, 0]
    elif t[0] == "resize":
        _, h, w, nh, nw = t
        coords[:, 0] = coords[:, 0] * F32(nw * 1.0 / w)
        coords[:, 1] = coords[:, 1] * F32(nh * 1.0 / h)
    else:
        assert t[0] == "scale"           # planted faults only: multiply by float32 factors given directly
        coords[:, 0] = coords[:, 0] * t[1]
        coords[:, 1] = coords[:, 1] * t[2]
    return coords


def apply_box(t, boxes):
    """d2 Transform.apply_box: the four corners through apply_coords, then min / max"""
    boxes = np.asarray(boxes, dtype=F32).reshape(-1, 4)
    idxs = np.array([(0, 1), (2, 1), (0, 3), (2, 3)]).flatten()
    coords = boxes[:, idxs].reshape(-1, 2)
    coords = _apply_coords(t, coords).reshape((-1, 4, 2))
    with np.errstate(invalid="ignore"):
        return np.concatenate((coords.min(axis=1), coords.max(axis=1)), axis=1).astype(F32)


def inverse_of(t):
    if t[0] == "hflip":
        return t
    _, h, w, nh, nw = t
    return ("resize", nh, nw, h, w)


def forward_boxes(boxes, aug):
    for t in aug["transforms"]:
        boxes = apply_box(t, boxes)
    return boxes


def inverse_boxes(boxes, aug, fault=None):
    """boxes of one augmented pass -> the original frame (float32 [n, 4])"""
    inv = [inverse_of(t) for t in reversed(aug["transforms"])]
    if fault == "unflip_w":
        w_test = aug["transforms"][-2 if aug["flip"] else -1][2]
        inv = [("hflip", w_test) if t[0] == "hflip" else t for t in inv]
    resizes = [t for t in inv if t[0] == "resize"]
    if fault == "ratio_order" and len(resizes) == 2:
        inv = [t for t in inv if t[0] == "hflip"] + resizes[::-1]
    if fault == "ratio_fused" and len(resizes) == 2:
        (_, h1, w1, nh1, nw1), (_, h2, w2, nh2, nw2) = resizes
        inv = [t for t in inv if t[0] == "hflip"] + [("scale", F32(nw1 * 1.0 / w1) * F32(nw2 * 1.0 / w2),
                                                      F32(nh1 * 1.0 / h1) * F32(nh2 * 1.0 / h2))]
    boxes = np.asarray(boxes, dtype=F32).reshape(-1, 4)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in inv:
            boxes = apply_box(t, boxes)
    return boxes


# ---- 5. fast_rcnn_inference_single_image --------------------------------------------------------------------------------------
def fast_rcnn_inference_single_image(boxes, scores, image_shape, score_thresh, nms_thresh, topk_per_image, numel_limit=20000,
                                     ge=False):
    """d2's, for class-agnostic boxes [N, 4] or per-class boxes [N, 4K] and scores [N, K + 1] -> (boxes [m, 4], scores [m],
    classes [m]) float32 / float32 / int64, and the number of (row, class) pairs that passed the score test"""
    boxes, scores = np.asarray(boxes, dtype=F32), np.asarray(scores, dtype=F32)
    valid = np.isfinite(boxes).all(axis=1) & np.isfinite(scores).all(axis=1)
    boxes, scores = boxes[valid], scores[valid]
    scores = scores[:, :-1]
    nreg = boxes.shape[1] // 4
    b = OB.clip_boxes(torch.from_numpy(boxes.reshape(-1, 4)), image_shape).numpy().reshape(-1, nreg, 4)
    mask = (scores >= F32(score_thresh)) if ge else (scores > F32(score_thresh))
    rows, cols = np.nonzero(mask)                        # row-major, as torch's nonzero
    b = b[rows, 0] if nreg == 1 else b[rows, cols]
    s = scores[rows, cols]
    keep = OB.batched_nms(torch.from_numpy(b).reshape(-1, 4), torch.from_numpy(s), torch.from_numpy(cols), nms_thresh,
                          numel_limit=numel_limit).numpy()
    if topk_per_image >= 0:
        keep = keep[:topk_per_image]
    return b[keep].reshape(-1, 4), s[keep], cols[keep].astype(np.int64), int(mask.sum())


def merge_detections(all_boxes, all_scores, all_classes, native_hw, num_classes, nms_thresh, topk, numel_limit=20000, fault=None):
    """d2 _merge_detections on the concatenated detections of one image (already in the original frame)"""
    all_boxes = np.asarray(all_boxes, dtype=F32).reshape(-1, 4)
    all_scores = np.asarray(all_scores, dtype=F32).reshape(-1)
    all_classes = np.asarray(all_classes).reshape(-1).astype(np.int64)
    n = len(all_boxes)
    scores_2d = np.zeros((n, num_classes + 1), dtype=F32)
    scores_2d[np.arange(n), all_classes] = all_scores
    return fast_rcnn_inference_single_image(all_boxes, scores_2d, native_hw, SCORE_THRESH, nms_thresh, topk, numel_limit,
                                            ge=(fault == "ge"))


def tta_image(passes, augs, native_hw, num_classes, nms_thresh, topk, numel_limit=20000, fault=None):
    """``passes``: per augmentation (boxes [n, 4], scores [n], classes [n]) as the model returned them at the augmented size
    -> merge_detections' result for the image"""
    assert len(passes) == len(augs)
    bs = [inverse_boxes(p[0], a, fault) for p, a in zip(passes, augs)]
    return merge_detections(np.concatenate(bs) if bs else np.zeros((0, 4), F32),
                            np.concatenate([np.asarray(p[1], dtype=F32).reshape(-1) for p in passes]),
                            np.concatenate([np.asarray(p[2]).reshape(-1) for p in passes]),
                            native_hw, num_classes, nms_thresh, topk, numel_limit, fault)
