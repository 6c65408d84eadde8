"""The mosaic source trainers' loader (TRAINER base_mosaic / base_mosaic_wq / base_mosaic_wq_new) and the strong-augmented
source loader (TRAINER base_wq).

The reference wraps its mapped training set in ``MosaicDetection`` (``daod/data/mappers/mosaic.py:81-265``; the ``_wq`` and
``_wq_new`` copies differ in where ``build_strong_augmentation`` is applied): every item is four mapped frames, each scaled
back up to its native size, pasted around the centre of a 2H x 2W canvas filled with 114, and the canvas halved.  Here:

  * ``build_plan`` is the host part -- tile scales, paste rectangles, box offsets -- pure integer / float64 arithmetic on
    the frames' sizes, testable without a device;
  * the image is ONE ``native.mosaic_u8`` launch on a CUDA device (the canvas and the up-scaled tiles never exist), the
    numpy / Pillow composition ``compose_host`` on a CPU device;
  * the boxes follow in float32 (``transform_boxes`` on the host, ``_boxes_torch`` on the items' device), one rounding
    after the product and one after the sum.

What follows the reference and what does not: the three extra indices are drawn uniformly over the
dataset like the reference's ``random.randint``, but from the loader's own torch generator (the stance of data/augment.py);
the reference's extra ``D[idx]`` call that reads only height / width, and its two discarded ``uniform`` draws, are not made;
the up-scale is the project's Pillow-exact bilinear where the reference calls ``cv2.resize(INTER_LINEAR)``, the halving is
the rounded 2x2 mean.  ``height`` / ``width`` of an item are the CANVAS's, the box clip uses the LAST tile's native size:
the reference's quirks, kept.
"""
import numpy as np
import torch

from .. import native
from ..structures import Boxes, Instances
from .synthetic import TwoCropLoader

FILL = 114
VARIANTS = ("mosaic", "mosaic_wq", "mosaic_wq_new")


def mosaic_coordinate(k, xc, yc, w, h, input_h, input_w):
    """Where tile k (0 top-left, 1 top-right, 2 bottom-left, 3 bottom-right) of up-scaled size (h, w) lands around the centre
    (xc, yc) of a canvas of (2 * input_h, 2 * input_w): -> ((l_x1, l_y1, l_x2, l_y2) on the canvas, (s_x1, s_y1, s_x2, s_y2)
    in the tile).  Left / top tiles end at the centre and lose their far side when they do not fit; right / bottom tiles
    start at the centre and lose their far side."""
    if k not in (0, 1, 2, 3):
        raise ValueError(f"mosaic tile index {k} outside 0..3")
    if k in (0, 2):
        x1, x2 = max(xc - w, 0), xc
        sx1, sx2 = w - (x2 - x1), w
    else:
        x1, x2 = xc, min(xc + w, input_w * 2)
        sx1, sx2 = 0, min(w, x2 - x1)
    if k in (0, 1):
        y1, y2 = max(yc - h, 0), yc
        sy1, sy2 = h - (y2 - y1), h
    else:
        y1, y2 = yc, min(input_h * 2, yc + h)
        sy1, sy2 = 0, min(y2 - y1, h)
    return (x1, y1, x2, y2), (sx1, sy1, sx2, sy2)


class TilePlan:
    __slots__ = ("mapped_hw", "native_hw", "scale", "up_hw", "large", "small", "pad")

    def __init__(self, mapped_hw, native_hw, scale, up_hw, large, small):
        self.mapped_hw, self.native_hw, self.scale, self.up_hw = mapped_hw, native_hw, scale, up_hw
        self.large, self.small = large, small
        self.pad = (large[0] - small[0], large[1] - small[1])       # (padw, padh)


class MosaicPlan:
    """The geometry of one mosaic: ``tiles`` (TilePlan per tile, paste order), ``canvas_hw`` = (2*H0, 2*W0), ``out_hw`` =
    (H0, W0), ``clip_hw`` = the LAST tile's native size (what the reference clips the boxes with), ``indices`` (dataset indices
    of the tiles, when a loader built it)."""
    __slots__ = ("tiles", "canvas_hw", "out_hw", "clip_hw", "indices")

    def __init__(self, tiles, indices=None):
        self.tiles = tiles
        H0, W0 = tiles[0].native_hw
        self.canvas_hw, self.out_hw = (2 * H0, 2 * W0), (H0, W0)
        self.clip_hw = tiles[-1].native_hw
        self.indices = indices

    @property
    def identity(self):
        return all(t.up_hw == t.mapped_hw for t in self.tiles)


def build_plan(mapped_hws, native_hws, indices=None):
    """``mapped_hws[k]`` = (h0, w0) of mapped tile k, ``native_hws[k]`` = (Hk, Wk) its item's height / width -> MosaicPlan.
    ValueError when a paste rectangle leaves the canvas (sized by tile 0) or its two sides differ in extent -- where the
    reference dies with numpy's broadcast error; only native sizes that differ inside one mosaic can get there."""
    if len(mapped_hws) != 4 or len(native_hws) != 4:
        raise ValueError("a mosaic takes four tiles")
    H0, W0 = int(native_hws[0][0]), int(native_hws[0][1])
    tiles = []
    for k in range(4):
        h0, w0 = int(mapped_hws[k][0]), int(mapped_hws[k][1])
        Hk, Wk = int(native_hws[k][0]), int(native_hws[k][1])
        if min(h0, w0, Hk, Wk) < 1:
            raise ValueError(f"mosaic tile {k}: empty frame (mapped {h0}x{w0}, native {Hk}x{Wk})")
        s = min(1.0 * Hk / h0, 1.0 * Wk / w0)
        h, w = int(h0 * s), int(w0 * s)
        large, small = mosaic_coordinate(k, Wk, Hk, w, h, Hk, Wk)
        lw, lh, sw, sh = large[2] - large[0], large[3] - large[1], small[2] - small[0], small[3] - small[1]
        if min(large) < 0 or large[2] > 2 * W0 or large[3] > 2 * H0 or lw < 0 or lh < 0:
            raise ValueError(f"mosaic tile {k}: the paste rectangle x {large[0]}:{large[2]}, y {large[1]}:{large[3]} leaves the "
                             f"{2 * H0}x{2 * W0} canvas (native {Hk}x{Wk} against tile 0's {H0}x{W0})")
        if (lw, lh) != (sw, sh) or min(small) < 0 or small[2] > w or small[3] > h or h < 1 or w < 1:
            raise ValueError(f"mosaic tile {k}: the paste rectangle is {lh}x{lw}, the tile's window {sh}x{sw} of its {h}x{w} "
                             f"(native {Hk}x{Wk})")
        tiles.append(TilePlan((h0, w0), (Hk, Wk), s, (h, w), large, small))
    return MosaicPlan(tiles, indices)


def transform_boxes(boxes_list, plan):
    """float32 boxes [n_k, 4] (XYXY, mapped scale) per tile -> the mosaic's float32 boxes [sum n_k, 4]:
    ``b * float32(s) + (padw, padh, padw, padh)`` (one rounding after the product, one after the sum), concatenated in tile
    order, x clipped to [0, 2*W3] and y to [0, 2*H3] with the LAST tile's native size, times 0.5."""
    parts = []
    for b, t in zip(boxes_list, plan.tiles):
        b = np.asarray(b, dtype=np.float32).reshape(-1, 4)
        prod = b * np.float32(t.scale)
        parts.append(prod + np.array([t.pad[0], t.pad[1], t.pad[0], t.pad[1]], dtype=np.float32))
    out = np.concatenate(parts, 0).astype(np.float32)
    H3, W3 = plan.clip_hw
    hi = np.array([2 * W3, 2 * H3, 2 * W3, 2 * H3], dtype=np.float32)
    return np.minimum(np.maximum(out, np.float32(0)), hi) * np.float32(0.5)


def _boxes_torch(boxes_list, plan):
    """``transform_boxes`` in float32 torch ops on the boxes' own device (separate multiply and add: no fused multiply-add)."""
    dev = boxes_list[0].device
    parts = []
    for b, t in zip(boxes_list, plan.tiles):
        prod = b.to(torch.float32).reshape(-1, 4) * float(np.float32(t.scale))
        parts.append(prod + _const((t.pad[0], t.pad[1], t.pad[0], t.pad[1]), dev))
    H3, W3 = plan.clip_hw
    out = torch.cat(parts, 0)
    return torch.minimum(out.clamp(min=0), _const((2 * W3, 2 * H3, 2 * W3, 2 * H3), dev)) * 0.5


def _const(values, dev):
    if dev.type == "cuda":
        return native.dev_const(tuple(float(v) for v in values), torch.float32, dev)      # cached: no blocking upload per item
    return torch.tensor(values, dtype=torch.float32)


def _resize_hwc(arr, h, w):
    from PIL import Image
    if arr.shape[:2] == (h, w):
        return arr
    return np.asarray(Image.fromarray(arr).resize((w, h), Image.BILINEAR))


def halve(canvas):
    """[2H, 2W, C] uint8 -> [H, W, C]: the rounded mean of every 2x2 cell."""
    c = canvas.astype(np.uint16)
    return ((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def compose_host(tiles, plan, fill=FILL, strong_tile=None):
    """The image of a mosaic on the host (numpy + Pillow), what a CPU device runs: ``tiles`` uint8 [3, h0, w0] arrays ->
    uint8 [3, H0, W0].  ``strong_tile``: callable on an HWC uint8 array, applied to every up-scaled tile (base_mosaic_wq_new)."""
    Hc, Wc = plan.canvas_hw
    canvas = np.full((Hc, Wc, 3), fill, dtype=np.uint8)
    for tile, t in zip(tiles, plan.tiles):
        up = _resize_hwc(np.ascontiguousarray(np.asarray(tile).transpose(1, 2, 0)), t.up_hw[0], t.up_hw[1])
        if strong_tile is not None:
            up = np.asarray(strong_tile(up))
        (lx1, ly1, lx2, ly2), (sx1, sy1, sx2, sy2) = t.large, t.small
        canvas[ly1:ly2, lx1:lx2] = up[sy1:sy2, sx1:sx2]
    return np.ascontiguousarray(halve(canvas).transpose(2, 0, 1))


def _sampler_tap(loader, it):
    for idx in it:
        loader._last_index = idx
        yield idx


def _default_strong(cfg, device, rank, strong, who):
    if strong is not None:
        return strong
    if torch.device(device).type != "cuda":
        raise ValueError(f"{who}: the strong augmentation runs on a CUDA device (data/augment.py); on a CPU device pass "
                         "strong= (a callable on a uint8 [3,H,W] tensor)")
    from .augment import StrongAugmentation
    return StrongAugmentation(torch.Generator().manual_seed(max(cfg.SEED, 0) + 7919 * (rank + 1)))


def _apply_strong(strong, img, record):
    """``strong`` on one uint8 [3,H,W] frame.  A ``StrongAugmentation`` is sampled and applied apart, and its parameters and
    erasing noises are appended to ``record`` (tests replay them); any other callable is just called."""
    from .augment import StrongAugmentation
    if not isinstance(strong, StrongAugmentation):
        return strong(img)
    params = strong.sample(int(img.shape[1]), int(img.shape[2]))
    noises = [torch.randn(3, h, w, device=img.device) for _, _, h, w in params["erase"]]
    record.append((params, noises))
    return strong.apply(img, params, noises)


class MosaicLoader(TwoCropLoader):
    """``build_detection_train_loader`` of the reference's base_mosaic trainers (``daod/engine/trainers/base_mosaic*.py``):
    the labelled ``DATASETS.TRAIN`` frames through the loader's per-item mapper (every weak-augmentation option composes),
    four at a time into one mosaic.  ``variant``: "mosaic" | "mosaic_wq" (the strong augmentation once, on the mosaic) |
    "mosaic_wq_new" (on every up-scaled tile, before the paste).  Yields lists of ``SOLVER.IMS_PER_BATCH // world`` items,
    grouped by the item's ``width > height`` like every loader here; the look-ahead stream and ``record_stream`` handling are
    ``TwoCropLoader``'s.  Each item carries its ``mosaic_plan`` and, with a ``StrongAugmentation``, ``strong_params``."""

    def __init__(self, cfg, device, rank=0, world=1, variant="mosaic", dataset=None, strong=None, fill=FILL):
        if variant not in VARIANTS:
            raise ValueError(f"mosaic variant {variant!r} is not one of {VARIANTS}")
        super().__init__(cfg, device, rank, world, labeled=True, dataset=dataset)
        self.variant, self.fill = variant, int(fill)
        self.strong = _default_strong(cfg, device, rank, strong, f"TRAINER base_{variant}") if variant != "mosaic" else None
        self._last_index = None
        self.sampler = _sampler_tap(self, self.sampler)

    def _map(self, item):
        n = len(self.dataset)
        # [idx] + three more, uniform over the dataset, drawn BEFORE any tile is mapped (mosaic.py:99)
        extra = torch.randint(0, n, (3,), generator=self.gen).tolist()
        indices = [self._last_index] + extra
        mapped = [super(MosaicLoader, self)._map(it) for it in [item] + [self.dataset.items[i] for i in extra]]
        return self.compose(mapped, indices)

    def compose(self, mapped, indices=None):
        """Four mapped items -> the mosaic item."""
        imgs = [d["image"] for d in mapped]
        plan = build_plan([tuple(im.shape[1:]) for im in imgs], [(int(d["height"]), int(d["width"])) for d in mapped], indices)
        record = []
        if self.device.type == "cuda":
            if self.variant == "mosaic_wq_new":
                # blur and erasing need the whole up-scaled tile: the existing resize launch, the strong augmentation at canvas
                # scale, then the identity-scale body of the mosaic kernel
                ups = [im if t.up_hw == t.mapped_hw else native.resize_bilinear_u8(im, t.up_hw[0], t.up_hw[1])
                       for im, t in zip(imgs, plan.tiles)]
                imgs = [_apply_strong(self.strong, u, record) for u in ups]
            img = native.mosaic_u8(imgs, [t.up_hw for t in plan.tiles], [(t.large, t.small) for t in plan.tiles], plan.out_hw,
                                   fill=self.fill)
        else:
            strong_tile = None
            if self.variant == "mosaic_wq_new":
                def strong_tile(up):
                    t = torch.from_numpy(np.ascontiguousarray(up.transpose(2, 0, 1)))
                    return _apply_strong(self.strong, t, record).numpy().transpose(1, 2, 0)
            img = torch.from_numpy(compose_host([im.numpy() for im in imgs], plan, self.fill, strong_tile))
        if self.variant == "mosaic_wq":
            img = _apply_strong(self.strong, img, record)
        boxes = _boxes_torch([d["instances"].gt_boxes.tensor for d in mapped], plan)
        classes = torch.cat([d["instances"].gt_classes for d in mapped], 0)
        Hc, Wc = plan.canvas_hw
        inst = Instances((Hc, Wc))            # the reference reports the canvas: Instances((height, width)), mosaic.py:260
        inst.gt_boxes = Boxes(boxes)
        inst.gt_classes = classes
        out = {"image": img, "instances": inst, "height": Hc, "width": Wc, "image_id": mapped[0]["image_id"],
               "file_name": mapped[0]["file_name"], "mosaic_plan": plan}
        if record:
            out["strong_params"] = record
        return out


class StrongLoader(TwoCropLoader):
    """TRAINER base_wq (``daod/engine/trainers/base_wq.py``, ``BaseWQDetection`` in ``daod/data/mappers/strong_aug.py``): the
    ``base`` loader with the strong augmentation applied to every mapped frame.  No mosaic."""

    def __init__(self, cfg, device, rank=0, world=1, dataset=None, strong=None):
        super().__init__(cfg, device, rank, world, labeled=True, dataset=dataset)
        self.strong = _default_strong(cfg, device, rank, strong, "TRAINER base_wq")

    def _map(self, item):
        d = super()._map(item)
        record = []
        d["image"] = _apply_strong(self.strong, d["image"], record)
        if record:
            d["strong_params"] = record
        return d
