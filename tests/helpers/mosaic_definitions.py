"""The mosaic of the base_mosaic trainers, stated in numpy + Pillow: the yardstick of tests/test_mosaic_host.py and
tests/test_gpu_mosaic.py (written from the rule in DESIGN.md section 4.11, not from the package's data/mosaic.py; pinned to
the reference's ``MosaicDetection`` / ``MosaicWQDetection`` / ``MosaicWQNewDetection`` through tests/golden/mosaic_ref.npz).

For four mapped tiles ``tile_k`` uint8 [3, h0, w0] with native sizes (Hk, Wk), float32 boxes and classes:

  1. s = min(1.0 * Hk / h0, 1.0 * Wk / w0) in float64, (h, w) = (int(h0 * s), int(w0 * s)), U_k = Pillow bilinear resize of the
     tile to (h, w);
  2. ``wq_new``: U_k = strong(U_k);
  3. the canvas is [2*H0, 2*W0] (tile 0's native size) filled with 114; tile k's corner touches the centre (Wk, Hk) of ITS OWN
     2*Hk x 2*Wk frame -- tile 0 ends there, tile 1 ends above and starts to the right, tile 2 starts below and ends to the
     left, tile 3 starts there -- and what leaves that frame is cut; pasted in order, later tiles overwrite earlier ones;
  4. boxes: b * float32(s) + (padw, padh, padw, padh) in float32, concatenated, x clipped to [0, 2*W3], y to [0, 2*H3]
     (the LAST tile's size), times 0.5; classes concatenated;
  5. image: rounded mean of every 2x2 canvas cell; ``wq``: strong(image);
  6. height / width = the canvas's.
"""
import numpy as np
from PIL import Image

FILL = 114
VARIANTS = ("mosaic", "mosaic_wq", "mosaic_wq_new")


def tile_geometry(h0, w0, Hk, Wk):
    s = min(1.0 * Hk / h0, 1.0 * Wk / w0)
    return s, (int(h0 * s), int(w0 * s))


def rectangles(k, w, h, Hk, Wk):
    """-> ((l_x1, l_y1, l_x2, l_y2), (s_x1, s_y1, s_x2, s_y2)) of tile k of up-scaled size (h, w) whose corner touches (Wk, Hk),
    cut to the frame [0, 2*Hk) x [0, 2*Wk)."""
    ox = Wk - w if k in (0, 2) else Wk            # canvas position of the tile's column 0 / row 0
    oy = Hk - h if k in (0, 1) else Hk
    lx1, lx2 = max(ox, 0), min(ox + w, 2 * Wk)
    ly1, ly2 = max(oy, 0), min(oy + h, 2 * Hk)
    return (lx1, ly1, lx2, ly2), (lx1 - ox, ly1 - oy, lx2 - ox, ly2 - oy)


def pil_resize(chw, h, w):
    hwc = np.ascontiguousarray(np.asarray(chw).transpose(1, 2, 0))
    if hwc.shape[:2] == (h, w):
        return hwc
    return np.asarray(Image.fromarray(hwc).resize((w, h), Image.BILINEAR))


def halve(canvas):
    c = canvas.astype(np.int64)
    return ((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def compose(tiles, up_hw, rects, out_hw, fill=FILL, upscaled=False):
    """The image alone, for explicit geometry (what ``native.mosaic_u8`` takes): -> uint8 [3, H0, W0].  ``upscaled``: the
    tiles are already at (h, w)."""
    H0, W0 = out_hw
    canvas = np.full((2 * H0, 2 * W0, 3), fill, np.uint8)
    for k, tile in enumerate(tiles):
        up = np.ascontiguousarray(np.asarray(tile).transpose(1, 2, 0)) if upscaled else pil_resize(tile, up_hw[k][0], up_hw[k][1])
        (lx1, ly1, lx2, ly2), (sx1, sy1, sx2, sy2) = rects[k]
        if not (0 <= lx1 <= lx2 <= 2 * W0 and 0 <= ly1 <= ly2 <= 2 * H0) or (lx2 - lx1, ly2 - ly1) != (sx2 - sx1, sy2 - sy1) \
                or not (0 <= sx1 and sx2 <= up.shape[1] and 0 <= sy1 and sy2 <= up.shape[0]):
            raise ValueError(f"mosaic tile {k}: paste {rects[k][0]} / window {rects[k][1]} of {up.shape[:2]} on a "
                             f"{2 * H0}x{2 * W0} canvas")
        canvas[ly1:ly2, lx1:lx2] = up[sy1:sy2, sx1:sx2]
    return np.ascontiguousarray(halve(canvas).transpose(2, 0, 1))


def mosaic(tiles, boxes, classes, native_hw, variant="mosaic", strong=None, fill=FILL):
    """-> dict(image uint8 [3,H0,W0], boxes float32 [n,4], classes, height, width).  ``strong``: callable on an HWC uint8
    array (the variants with a strong augmentation)."""
    assert variant in VARIANTS and len(tiles) == 4
    H0, W0 = (int(v) for v in native_hw[0])
    ups, rects, out_boxes = [], [], []
    for k in range(4):
        h0, w0 = tiles[k].shape[1:]
        Hk, Wk = (int(v) for v in native_hw[k])
        s, (h, w) = tile_geometry(h0, w0, Hk, Wk)
        up = pil_resize(tiles[k], h, w)
        if variant == "mosaic_wq_new":
            up = np.asarray(strong(up))
        ups.append(np.ascontiguousarray(up.transpose(2, 0, 1)))
        large, small = rectangles(k, w, h, Hk, Wk)
        rects.append((large, small))
        b = np.asarray(boxes[k], np.float32).reshape(-1, 4)
        prod = (b * np.float32(s)).astype(np.float32)
        padw, padh = large[0] - small[0], large[1] - small[1]
        out_boxes.append((prod + np.array([padw, padh, padw, padh], np.float32)).astype(np.float32))
    image = compose(ups, None, rects, (H0, W0), fill, upscaled=True)
    if variant == "mosaic_wq":
        image = np.ascontiguousarray(np.asarray(strong(np.ascontiguousarray(image.transpose(1, 2, 0)))).transpose(2, 0, 1))
    b = np.concatenate(out_boxes, 0)
    H3, W3 = (int(v) for v in native_hw[3])
    b[:, 0::2] = np.clip(b[:, 0::2], 0, 2 * W3)
    b[:, 1::2] = np.clip(b[:, 1::2], 0, 2 * H3)
    return {"image": image, "boxes": (b * np.float32(0.5)).astype(np.float32),
            "classes": np.concatenate([np.asarray(c).reshape(-1) for c in classes], 0), "height": 2 * H0, "width": 2 * W0}


def invert(hwc):
    """The marker transform of the golden: shows WHERE each variant applies its strong augmentation."""
    return 255 - np.asarray(hwc)
