"""Test-time augmentation options and plans, read from the config (no device needed).

``TEST.AUG.{ENABLED, MIN_SIZES, MAX_SIZE, FLIP}`` are Detectron2's keys with Detectron2's defaults; whatever cannot run raises
a ``ValueError`` that names the key.  ``TTAOptions.plan(h, w, H0, W0)`` is the host side of one input dict, as
``DatasetMapperTTA`` builds it: the starting tensor is the input's ``"image"`` (the frame already resized to the test size
``(h, w)``; the native frame is ``(H0, W0)``), every ``s`` in ``MIN_SIZES`` gives ``ResizeShortestEdge(s, MAX_SIZE)`` of it
and, with ``FLIP``, that resize followed by a horizontal flip.  A plan holds the augmented sizes in that order and the table
``sfod_tta_merge`` reads per augmentation: ``(w_a, h_a, flip, w / w_a, h / h_a, W0 / w, H0 / h, 0)``, each ratio the double
quotient rounded to float32 once -- what numpy does when ``ResizeTransform.apply_coords`` multiplies a float32 array by
``new_w * 1.0 / w``.  Plans are cached per ``(h, w, H0, W0)``.
"""
import collections

import numpy as np

from ..data.weak_augment import resize_shortest_edge_shape

MERGE_CAPACITY = 4096         # augmentations x detections per image the merge kernel is built for (include/sfod_hip.h)
MAX_AUGMENTATIONS = 64
TABLE_ROW = 8

# sizes: ((h_a, w_a), ...) one per MIN_SIZES entry; table: tuple of A rows (one per augmentation, in d2's order) of TABLE_ROW
# python floats, each exactly a float32 value
TTAPlan = collections.namedtuple("TTAPlan", "hw native_hw sizes table")


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _f32(x):
    return float(np.float32(x))


class TTAOptions:
    """The validated keys.  ``plan(h, w, H0, W0)`` -> TTAPlan (cached)."""

    def __init__(self, cfg):
        aug = cfg.TEST.AUG
        sizes = aug.MIN_SIZES
        if _is_int(sizes):
            sizes = (sizes,)
        if not isinstance(sizes, (tuple, list)) or len(sizes) == 0:
            raise ValueError(f"TEST.AUG.MIN_SIZES must be a non-empty sequence of positive integers, got {sizes!r}")
        if not all(_is_int(v) and v > 0 for v in sizes):
            raise ValueError(f"TEST.AUG.MIN_SIZES must hold positive integers only, got {sizes!r}")
        self.min_sizes = tuple(int(v) for v in sizes)
        if not _is_int(aug.MAX_SIZE) or aug.MAX_SIZE < 1:
            raise ValueError(f"TEST.AUG.MAX_SIZE must be an integer >= 1, got {aug.MAX_SIZE!r}")
        self.max_size = int(aug.MAX_SIZE)
        if not isinstance(aug.FLIP, bool):
            raise ValueError(f"TEST.AUG.FLIP must be True or False (horizontal flip; no other flip is built), got {aug.FLIP!r}")
        self.flip = aug.FLIP
        self.per_size = 2 if self.flip else 1
        self.num_aug = len(self.min_sizes) * self.per_size
        self.max_det = int(cfg.TEST.DETECTIONS_PER_IMAGE)
        if self.max_det < 1:
            raise ValueError(f"TEST.DETECTIONS_PER_IMAGE must be >= 1 under TEST.AUG, got {cfg.TEST.DETECTIONS_PER_IMAGE!r}")
        if self.num_aug > MAX_AUGMENTATIONS or self.num_aug * self.max_det > MERGE_CAPACITY:
            raise ValueError(f"TEST.AUG.MIN_SIZES: {len(self.min_sizes)} sizes x {self.per_size} (TEST.AUG.FLIP) x "
                             f"TEST.DETECTIONS_PER_IMAGE {self.max_det} = {self.num_aug * self.max_det} candidates per image; "
                             f"the merge kernel takes at most {MAX_AUGMENTATIONS} augmentations and {MERGE_CAPACITY} candidates")
        if cfg.MODEL.LOAD_PROPOSALS:
            raise ValueError("MODEL.LOAD_PROPOSALS must be False under TEST.AUG (precomputed proposals cannot follow an "
                             "augmented frame), got True")
        self._plans = {}

    def plan(self, h, w, H0, W0):
        key = (int(h), int(w), int(H0), int(W0))
        p = self._plans.get(key)
        if p is None:
            p = self._plans[key] = build_plan(*key, self.min_sizes, self.max_size, self.flip)
        return p


def build_plan(h, w, H0, W0, min_sizes, max_size, flip):
    if min(h, w, H0, W0) < 1:
        raise ValueError(f"test-time augmentation of an empty frame: tensor {h} x {w}, frame {H0} x {W0}")
    # pre = ResizeTransform(H0, W0, h, w) (the identity when the sizes agree); its inverse multiplies by (W0 / w, H0 / h)
    rx2, ry2 = _f32(W0 * 1.0 / w), _f32(H0 * 1.0 / h)
    sizes, table = [], []
    for s in min_sizes:
        ha, wa = resize_shortest_edge_shape(h, w, s, max_size)
        if min(ha, wa) < 1:
            raise ValueError(f"TEST.AUG.MIN_SIZES {s} with TEST.AUG.MAX_SIZE {max_size} resizes a {h} x {w} tensor to {ha} x {wa}")
        sizes.append((ha, wa))
        for f in range(2 if flip else 1):
            table.append((float(wa), float(ha), float(f), _f32(w * 1.0 / wa), _f32(h * 1.0 / ha), rx2, ry2, 0.0))
    return TTAPlan((h, w), (H0, W0), tuple(sizes), tuple(table))


def validate_tta_cfg(cfg):
    """Every key above, checked without building a module."""
    TTAOptions(cfg)
