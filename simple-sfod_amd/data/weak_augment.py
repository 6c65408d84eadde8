"""Options of the weak augmentation: INPUT.CROP, INPUT.MIN_SIZE_TRAIN (all of it) with INPUT.MIN_SIZE_TRAIN_SAMPLING, and
INPUT.RANDOM_FLIP horizontal | vertical | none.

The reference's training mapper (``daod/data/mappers/two_crop_augmentation_mapper.py:35-48``) builds its weak augmentation as
``[T.RandomCrop(CROP.TYPE, CROP.SIZE)] + utils.build_augmentation(cfg, True)`` = RandomCrop, ResizeShortestEdge(MIN_SIZE_TRAIN,
MAX_SIZE_TRAIN, MIN_SIZE_TRAIN_SAMPLING), RandomFlip(horizontal or vertical), and filters empty instances afterwards.  This
module validates those keys (a ``ValueError`` names the key), draws the plan of one item with Detectron2's DISTRIBUTIONS in
Detectron2's order -- from the loader's own ``torch.Generator`` (the project never used numpy's global RNG, so the streams are
not Detectron2's) -- and transforms the boxes on the host in float64 as Detectron2 does.  The image itself is one
``native.weak_augment_u8`` launch (``sfod_resize_bilinear_u8_opt``), or Pillow on a CPU device (``apply_host``).

``WeakAugmentOptions.default``: one MIN_SIZE_TRAIN value, sampling "choice", flip horizontal or none, no crop -- the loaders
then take the path they always took (pre-scaled device boxes, one ``torch.rand(1)`` per item when flipping is on).
"""
import collections

import numpy as np
import torch

FLIP_MODES = {"none": 0, "horizontal": 1, "vertical": 2}
CROP_TYPES = ("relative", "relative_range", "absolute", "absolute_range")

# window = (y0, x0, ch, cw) inside the native frame or None (no crop); out_hw = (h, w); flip_mode 0 / 1 / 2 as APPLIED to
# this item; native_hw = the frame's size, short = the short edge drawn (0: no resize)
WeakPlan = collections.namedtuple("WeakPlan", "window out_hw flip_mode native_hw short")


def resize_shortest_edge_shape(h, w, short, max_size):
    """d2 ResizeShortestEdge.get_output_shape."""
    scale = short * 1.0 / min(h, w)
    if h < w:
        newh, neww = short, scale * w
    else:
        newh, neww = scale * h, short
    if max(newh, neww) > max_size:
        scale = max_size * 1.0 / max(newh, neww)
        newh, neww = newh * scale, neww * scale
    return int(newh + 0.5), int(neww + 0.5)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _is_num(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def crop_size(crop_type, size, h, w, uniform=None, randint=None):
    """d2 RandomCrop.get_crop_size on an (h, w) frame -> (ch, cw).  ``uniform()`` -> float64 in [0, 1), ``randint(lo, hi)`` ->
    integer in [lo, hi] (both ends); only the ``*_range`` types draw."""
    if crop_type == "relative":
        return int(h * size[0] + 0.5), int(w * size[1] + 0.5)
    if crop_type == "relative_range":
        # d2: crop_size = np.asarray(self.crop_size, dtype=np.float32); ch, cw = crop_size + np.random.rand(2) * (1 - crop_size)
        # -- SIZE rounded to float32, (1 - SIZE) formed in float32 (exact for SIZE >= 0.5), the rest in float64
        s = np.asarray(size, dtype=np.float32)
        u = np.array([uniform(), uniform()], dtype=np.float64)
        c = s + u * (1 - s)
        return int(h * c[0] + 0.5), int(w * c[1] + 0.5)
    if crop_type == "absolute":
        return min(size[0], h), min(size[1], w)
    if crop_type == "absolute_range":
        ch = randint(min(h, size[0]), min(h, size[1]))
        cw = randint(min(w, size[0]), min(w, size[1]))
        return ch, cw
    raise ValueError(f"INPUT.CROP.TYPE must be one of {' | '.join(CROP_TYPES)}, got {crop_type!r}")


class WeakAugmentOptions:
    """The validated keys.  ``sample(h, w, gen)`` draws one item's plan."""

    def __init__(self, cfg):
        inp = cfg.INPUT
        flip = inp.RANDOM_FLIP
        if flip not in FLIP_MODES:
            raise ValueError(f"INPUT.RANDOM_FLIP must be one of horizontal | vertical | none, got {flip!r}")
        self.flip_mode = FLIP_MODES[flip]
        sizes = inp.MIN_SIZE_TRAIN
        if _is_int(sizes):
            sizes = (sizes,)
        if not isinstance(sizes, (tuple, list)) or len(sizes) == 0 or not all(_is_int(v) and v >= 0 for v in sizes):
            raise ValueError(f"INPUT.MIN_SIZE_TRAIN must be a non-empty sequence of non-negative integers (0: no resize), got {sizes!r}")
        self.sizes = tuple(int(v) for v in sizes)
        self.sampling = inp.MIN_SIZE_TRAIN_SAMPLING if "MIN_SIZE_TRAIN_SAMPLING" in inp else "choice"
        if self.sampling not in ("choice", "range"):
            raise ValueError(f"INPUT.MIN_SIZE_TRAIN_SAMPLING must be one of choice | range, got {self.sampling!r}")
        if self.sampling == "range" and (len(self.sizes) != 2 or self.sizes[0] > self.sizes[1]):
            raise ValueError("INPUT.MIN_SIZE_TRAIN_SAMPLING 'range' needs INPUT.MIN_SIZE_TRAIN = (lo, hi) with lo <= hi, got "
                             f"{self.sizes!r}")
        self.max_size = int(inp.MAX_SIZE_TRAIN)
        self.crop = None
        crop = inp.CROP if "CROP" in inp else None
        if crop is not None and crop.ENABLED:
            ctype, size = crop.TYPE, crop.SIZE
            if ctype not in CROP_TYPES:
                raise ValueError(f"INPUT.CROP.TYPE must be one of {' | '.join(CROP_TYPES)}, got {ctype!r}")
            if not isinstance(size, (tuple, list)) or len(size) != 2 or not all(_is_num(v) for v in size):
                raise ValueError(f"INPUT.CROP.SIZE must be two numbers, got {size!r}")
            if ctype.startswith("relative"):
                if not all(0.0 < float(v) <= 1.0 for v in size):
                    raise ValueError(f"INPUT.CROP.SIZE must lie in (0, 1] for INPUT.CROP.TYPE {ctype!r}, got {size!r}")
                size = (float(size[0]), float(size[1]))
            else:
                if not all(float(v) == int(v) and int(v) > 0 for v in size):
                    raise ValueError(f"INPUT.CROP.SIZE must be two positive integers for INPUT.CROP.TYPE {ctype!r}, got {size!r}")
                size = (int(size[0]), int(size[1]))
                if ctype == "absolute_range" and size[0] > size[1]:
                    raise ValueError(f"INPUT.CROP.SIZE needs SIZE[0] <= SIZE[1] for INPUT.CROP.TYPE 'absolute_range', got {size!r}")
            self.crop = (ctype, size)
        self.default = (self.crop is None and len(self.sizes) == 1 and self.sizes[0] > 0 and self.sampling == "choice"
                        and self.flip_mode in (0, 1))

    # ---- draws: the loader's torch.Generator, Detectron2's distributions --------------------------------------------------
    @staticmethod
    def _uniform(gen):
        return float(torch.rand(1, generator=gen, dtype=torch.float64).item())

    @staticmethod
    def _randint(gen, lo, hi):
        """uniform integer in [lo, hi], both ends (np.random.randint(lo, hi + 1))"""
        return int(torch.randint(int(lo), int(hi) + 1, (1,), generator=gen).item())

    def sample(self, h, w, gen):
        """-> WeakPlan for a native (h, w) frame.  Draw order = Detectron2's augmentation list: RandomCrop (size, then y0,
        then x0), ResizeShortestEdge (no draw for a single "choice" value), RandomFlip (``torch.rand(1) < 0.5``)."""
        window = None
        ch, cw = h, w
        if self.crop is not None:
            ctype, size = self.crop
            ch, cw = crop_size(ctype, size, h, w, uniform=lambda: self._uniform(gen),
                               randint=lambda lo, hi: self._randint(gen, lo, hi))
            if not (h >= ch >= 1 and w >= cw >= 1):
                raise ValueError(f"INPUT.CROP.SIZE {size!r} ({ctype}) gives a {ch} x {cw} crop of a {h} x {w} frame")
            y0 = self._randint(gen, 0, h - ch)
            x0 = self._randint(gen, 0, w - cw)
            window = (y0, x0, ch, cw)
        if self.sampling == "range":
            short = self._randint(gen, self.sizes[0], self.sizes[1])
        elif len(self.sizes) > 1:
            short = self.sizes[self._randint(gen, 0, len(self.sizes) - 1)]
        else:
            short = self.sizes[0]
        out_hw = (ch, cw) if short == 0 else resize_shortest_edge_shape(ch, cw, short, self.max_size)
        flip = 0
        if self.flip_mode and torch.rand(1, generator=gen).item() < 0.5:
            flip = self.flip_mode
        return WeakPlan(window, out_hw, flip, (h, w), short)


def transform_boxes(boxes_native, plan, filter_empty=True):
    """Detectron2's box path for one item: native-scale XYXY boxes (any float array [n, 4]) through crop, resize and flip in
    float64 on the host, clipped to the output frame, cast to float32; ``filter_empty``: rows whose float32 width or height
    is <= 1e-5 are dropped (filter_empty_instances).  -> (float32 array [m, 4], kept row indices int64 [m])."""
    b = np.array(boxes_native, dtype=np.float64).reshape(-1, 4)
    h, w = plan.out_hw
    y0, x0, ch, cw = plan.window if plan.window is not None else (0, 0) + tuple(plan.native_hw)
    b[:, 0::2] -= x0
    b[:, 1::2] -= y0
    b[:, 0::2] *= w * 1.0 / cw
    b[:, 1::2] *= h * 1.0 / ch
    if plan.flip_mode == 1:
        b[:, 0], b[:, 2] = w - b[:, 2], w - b[:, 0].copy()
    elif plan.flip_mode == 2:
        b[:, 1], b[:, 3] = h - b[:, 3], h - b[:, 1].copy()
    b[:, 0::2] = np.clip(b[:, 0::2], 0, w)
    b[:, 1::2] = np.clip(b[:, 1::2], 0, h)
    b32 = b.astype(np.float32)
    keep = np.arange(b32.shape[0], dtype=np.int64)
    if filter_empty:
        keep = keep[((b32[:, 2] - b32[:, 0]) > 1e-5) & ((b32[:, 3] - b32[:, 1]) > 1e-5)]
    return b32[keep], keep


def apply_host(img_chw, plan):
    """The image side of a plan with Pillow on a CPU uint8 [C,H,W] tensor (CPU devices; host tests): crop, resize, flip."""
    from PIL import Image
    arr = img_chw.numpy()
    if plan.window is not None:
        y0, x0, ch, cw = plan.window
        arr = arr[:, y0:y0 + ch, x0:x0 + cw]
    h, w = plan.out_hw
    if (h, w) != tuple(arr.shape[1:]):
        if arr.shape[0] == 3:
            arr = np.asarray(Image.fromarray(np.ascontiguousarray(arr.transpose(1, 2, 0))).resize((w, h), Image.BILINEAR))
            arr = arr.transpose(2, 0, 1)
        else:
            arr = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(p)).resize((w, h), Image.BILINEAR)) for p in arr])
    if plan.flip_mode == 1:
        arr = arr[:, :, ::-1]
    elif plan.flip_mode == 2:
        arr = arr[:, ::-1, :]
    return torch.from_numpy(np.ascontiguousarray(arr))
