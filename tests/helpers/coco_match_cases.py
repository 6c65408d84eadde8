"""Hand-built inputs of ``sfod_coco_match`` (tests/test_coco_match_host.py, tests/test_gpu_coco_match.py): batches of at most
four images at the edges where COCOeval's matching goes wrong -- an IoU exactly on a threshold, tied scores, tied IoUs, crowd
and ignored ground truth, areas exactly on a range bound, counts at and around the wavefront width and the capacities.

An image is ``(dets, gts)``: ``dets`` rows ``(x1, y1, x2, y2, score, class)``, ``gts`` rows ``(x, y, w, h, area, class,
iscrowd)`` (``area`` None: w * h).  Coordinates are integers, so every area, intersection and union is exact.  Each generator
checks that its input holds the edge it is named for and raises ``EdgeMissed`` otherwise (it never skips)."""
import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)      # pycocotools Params.iouThrs
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
D_CAP, G_CAP = 100, 256


class EdgeMissed(AssertionError):
    """a generated input does not contain the edge it is named for"""


def require(cond, what):
    if not cond:
        raise EdgeMissed(what)


def iou_xyxy_xywh(d, g, crowd=False):
    """the definition's IoU of one detection row and one ground-truth row, in doubles"""
    dx, dy, dw, dh = float(d[0]), float(d[1]), float(np.float32(d[2]) - np.float32(d[0])), float(np.float32(d[3]) - np.float32(d[1]))
    w = min(dx + dw, g[0] + g[2]) - max(dx, g[0])
    h = min(dy + dh, g[1] + g[3]) - max(dy, g[1])
    if w <= 0 or h <= 0:
        return 0.0
    inter = w * h
    return inter / (dw * dh if crowd else dw * dh + g[2] * g[3] - inter)


def pack(images, D=D_CAP, G=None, poison=True):
    """images -> the fixed-capacity arrays.  ``poison``: the slots beyond the counts hold a detection / ground truth copied
    from slot 0 of the image (class and box that WOULD match) or, in an empty list, a full-frame box of class 0."""
    B = len(images)
    G = G or max(max(len(g) for _, g in images), 1)
    a = {"det_boxes": np.zeros((B, D, 4), np.float32), "det_scores": np.zeros((B, D), np.float32),
         "det_classes": np.zeros((B, D), np.int32), "det_count": np.zeros(B, np.int32),
         "gt_boxes": np.zeros((B, G, 4), np.float64), "gt_area": np.zeros((B, G), np.float64),
         "gt_classes": np.zeros((B, G), np.int32), "gt_iscrowd": np.zeros((B, G), np.int32), "gt_count": np.zeros(B, np.int32)}
    for b, (dets, gts) in enumerate(images):
        require(len(dets) <= D and len(gts) <= G, "pack: a list above the capacity")
        a["det_count"][b], a["gt_count"][b] = len(dets), len(gts)
        if poison:
            x1, y1, x2, y2, _, c = dets[0] if dets else (0, 0, 2048, 1024, 0, 0)
            a["det_boxes"][b], a["det_scores"][b], a["det_classes"][b] = (x1, y1, x2, y2), 2.0, c
            x, y, w, h, _, c, _ = gts[0] if gts else (0, 0, 2048, 1024, None, 0, 0)
            a["gt_boxes"][b], a["gt_area"][b], a["gt_classes"][b] = (x, y, w, h), w * h, c
        for i, (x1, y1, x2, y2, s, c) in enumerate(dets):
            a["det_boxes"][b, i], a["det_scores"][b, i], a["det_classes"][b, i] = (x1, y1, x2, y2), s, c
        for j, (x, y, w, h, area, c, crowd) in enumerate(gts):
            a["gt_boxes"][b, j], a["gt_area"][b, j] = (x, y, w, h), w * h if area is None else area
            a["gt_classes"][b, j], a["gt_iscrowd"][b, j] = c, crowd
    return a


def to_coco(images):
    """images -> (gt_anns, dt_anns, img_ids) as ``COCOevalBBox`` takes them; detections the way ``instances_to_coco_json``
    writes them (fp32 subtraction, then Python floats)."""
    gt_anns, dt_anns = [], []
    for b, (dets, gts) in enumerate(images):
        for x, y, w, h, area, c, crowd in gts:
            gt_anns.append({"image_id": b, "category_id": int(c), "bbox": [float(x), float(y), float(w), float(h)],
                            "iscrowd": int(crowd), "area": float(w * h if area is None else area)})
        if dets:
            boxes = np.array([d[:4] for d in dets], dtype=np.float32)
            boxes[:, 2] -= boxes[:, 0]
            boxes[:, 3] -= boxes[:, 1]
            scores = np.array([d[4] for d in dets], dtype=np.float32).tolist()
            for i, d in enumerate(dets):
                dt_anns.append({"image_id": b, "category_id": int(d[5]), "bbox": boxes[i].tolist(), "score": scores[i]})
    return gt_anns, dt_anns, list(range(len(images)))


def to_dataset_dicts(images):
    """images -> d2 dataset records for ``NewCOCOEvaluator`` (ids 0 .. B-1)"""
    return [{"image_id": b, "annotations": [{"bbox": [float(x), float(y), float(w), float(h)], "bbox_mode": 1, "category_id": int(c),
                                             "iscrowd": int(crowd), "area": float(w * h if area is None else area)}
                                            for x, y, w, h, area, c, crowd in gts]} for b, (_, gts) in enumerate(images)]


# ================================================================================================================================
def threshold_edges():
    """ground truth 200 x 10, detection 10k x 10 inside it: IoU = k / 20 -- on IOU_THRS[k - 10] bit for bit, except 18 / 20,
    which lies above IOU_THRS[8]; and the detection one lattice step narrower, below the threshold"""
    dets, gts, on, under = [], [], [], []
    for i, k in enumerate(range(10, 20)):
        for j, width in enumerate((10 * k, 10 * k - 1)):
            y = 20 * (2 * i + j)
            gts.append((0, y, 200, 10, None, 0, 0))
            dets.append((0, y, width, y + 10, 0.9 - 0.01 * (2 * i + j), 0))
            v = iou_xyxy_xywh(dets[-1], gts[-1])
            (on, under)[j].append(v)
    for i in range(10):
        require(on[i] == IOU_THRS[i] if i != 8 else on[i] > IOU_THRS[8] and on[i] == 0.9, f"IoU {on[i]!r} is not on threshold {i}")
        require(under[i] < IOU_THRS[i] and (i == 0 or under[i] > IOU_THRS[i - 1]), f"IoU {under[i]!r} is not just below threshold {i}")
    require(IOU_THRS[8] == 0.8999999999999999, "IOU_THRS[8]")
    return {"name": "threshold_edges", "K": 1, "images": [(dets, gts)]}


def tied_scores():
    """equal fp32 scores inside one category (two detections on one ground truth: the earlier index takes it) and across
    categories, and a NaN score on the best-placed detection, which ranks last"""
    s = np.float32(0.7)
    gts = [(0, 0, 20, 20, None, 0, 0), (100, 0, 20, 20, None, 1, 0), (200, 0, 20, 20, None, 0, 0)]
    dets = [(0, 0, 20, 18, s, 0), (0, 0, 20, 19, s, 0),                 # same class, same score, both >= 0.9 on gts[0]
            (100, 0, 20, 20, s, 1),                                     # another class, the same score
            (200, 0, 220, 20, float("nan"), 0), (200, 0, 220, 19, 0.1, 0),   # NaN: the exact box, still behind score 0.1
            (0, 0, 20, 17, np.float32(0.7) + np.float32(1e-7), 0)]       # one ulp region above: first of class 0
    sc = np.array([d[4] for d in dets], dtype=np.float32)
    require(sc[0] == sc[1] == sc[2] and np.isnan(sc[3]) and sc[5] > sc[0], "tied_scores: ties / NaN / next float missing")
    return {"name": "tied_scores", "K": 2, "images": [(dets, gts)]}


def tied_iou():
    """two ground truths at equal IoU to the first detection (the later-visited one is taken) and a second detection whose
    match depends on which one that was"""
    gts = [(0, 0, 20, 10, None, 0, 0), (4, 0, 20, 10, None, 0, 0)]
    dets = [(2, 0, 22, 10, 0.9, 0), (0, 0, 20, 10, 0.8, 0)]
    a, b = iou_xyxy_xywh(dets[0], gts[0]), iou_xyxy_xywh(dets[0], gts[1])
    require(a == b and a >= 0.8, "tied_iou: the first detection's IoUs differ")
    require(iou_xyxy_xywh(dets[1], gts[0]) == 1.0 and 0.65 < iou_xyxy_xywh(dets[1], gts[1]) < 0.7, "tied_iou: second detection")
    return {"name": "tied_iou", "K": 1, "images": [(dets, gts)]}


def crowd():
    """class 0: a crowd ground truth matched by three detections; class 1: a counted ground truth at IoU 0.6 visited before a
    crowd one at IoU 1 (the ``break`` keeps the counted one); class 2: only a crowd ground truth; class 3: only a ground truth
    that the small / large ranges ignore by area"""
    gts = [(0, 0, 100, 100, None, 0, 1),
           (200, 0, 12, 10, None, 1, 1), (200, 0, 20, 10, None, 1, 0),          # the crowd one comes FIRST in annotation order
           (400, 0, 50, 50, None, 2, 1),
           (600, 0, 50, 50, None, 3, 0)]
    dets = [(0, 0, 40, 40, 0.9, 0), (10, 10, 60, 60, 0.8, 0), (50, 50, 100, 100, 0.7, 0),
            (200, 0, 212, 10, 0.9, 1),
            (400, 0, 450, 50, 0.9, 2),
            (600, 0, 650, 50, 0.9, 3)]
    require(all(iou_xyxy_xywh(d, gts[0], True) == 1.0 for d in dets[:3]), "crowd: intersection over detection area")
    require(iou_xyxy_xywh(dets[3], gts[2]) == 0.6 and iou_xyxy_xywh(dets[3], gts[1], True) == 1.0, "crowd: break case")
    return {"name": "crowd", "K": 4, "images": [(dets, gts)]}


def area_edges():
    """``area`` fields and detection areas of exactly 32^2 and 96^2 (inside both neighbouring ranges), an ``area`` field that
    differs from w * h, and unmatched detections at the same edges"""
    gts = [(0, 0, 32, 32, None, 0, 0), (100, 0, 96, 96, None, 0, 0),
           (300, 0, 40, 40, 500.0, 0, 0),                                # 1600 by its box, "small" by its field
           (400, 0, 32, 32, 1024.0 + 2 ** -42, 0, 0), (500, 0, 32, 32, 1024.0 - 2 ** -42, 0, 0)]
    dets = [(0, 0, 32, 32, 0.9, 0), (100, 0, 196, 96, 0.8, 0), (300, 0, 340, 40, 0.7, 0),
            (400, 0, 432, 32, 0.65, 0), (500, 0, 532, 32, 0.64, 0),
            (700, 200, 732, 232, 0.6, 0), (800, 200, 896, 296, 0.5, 0),  # unmatched, areas 1024 and 9216
            (900, 200, 933, 231, 0.4, 0)]                                # unmatched, 33 x 31 = 1023
    require(gts[0][2] * gts[0][3] == AREA_RNG[1][1] == AREA_RNG[2][0] and gts[1][2] * gts[1][3] == AREA_RNG[2][1] == AREA_RNG[3][0],
            "area_edges: the boxes are not on the range bounds")
    require(gts[3][4] > 1024.0 and gts[4][4] < 1024.0, "area_edges: neighbours of 1024")
    return {"name": "area_edges", "K": 1, "images": [(dets, gts)]}


def extents():
    """empty detections with ground truth, empty ground truth with detections, both empty, and one ordinary image; classes
    -1 and K on both sides; a zero-width detection"""
    K = 3
    full = ([(0, 0, 20, 20, 0.9, 0), (0, 0, 20, 20, 0.8, -1), (0, 0, 20, 20, 0.7, K), (5, 0, 5, 20, 0.6, 0), (0, 0, 20, 19, 0.5, 0)],
            [(0, 0, 20, 20, None, 0, 0), (0, 0, 20, 20, None, -1, 0), (0, 0, 20, 20, None, K, 0), (40, 0, 20, 20, None, 2, 0)])
    images = [([], [(0, 0, 20, 20, None, 1, 0), (30, 0, 20, 20, None, 1, 1)]),
              ([(0, 0, 20, 20, 0.9, 1), (0, 0, 200, 200, 0.8, 2)], []),
              ([], []),
              full]
    require(any(d[0] == d[2] for d in full[0]) and {-1, K} <= {d[5] for d in full[0]} and {-1, K} <= {g[5] for g in full[1]},
            "extents: zero width / classes outside [0, K)")
    return {"name": "extents", "K": K, "images": images}


def full_detections():
    """D = 100 detections in one image over three classes, scores in a shuffled order with ties"""
    rng = np.random.RandomState(5)
    gts = [(40 * j, 0, 30, 30, None, j % 3, int(j == 7)) for j in range(10)]
    dets = []
    for i in range(D_CAP):
        j = int(rng.randint(10))
        dx, dy = int(rng.randint(0, 6)), int(rng.randint(0, 6))
        dets.append((40 * j + dx, dy, 40 * j + 30, 30, float(np.float32(rng.randint(1, 40) / 40.0)), int(rng.randint(3))))
    require(len(dets) == D_CAP and len({d[4] for d in dets}) < D_CAP, "full_detections: 100 detections with tied scores")
    return {"name": "full_detections", "K": 3, "images": [(dets, gts)]}


def gt_counts(n):
    """``n`` ground truths of one class (63 / 64 / 65: around the wavefront width; 256: the cap), the LAST one the only one the
    detections overlap, and one of another class in the middle"""
    gts = [(30 * (j % 60), 40 * (j // 60), 20, 20, None, 0, 0) for j in range(n)]
    gts[n // 2] = gts[n // 2][:5] + (1, 0)
    x, y = gts[-1][0], gts[-1][1]
    dets = [(x, y, x + 20, y + 19, 0.9, 0), (x, y, x + 20, y + 20, 0.8, 0), (gts[n // 2][0], gts[n // 2][1], gts[n // 2][0] + 20, gts[n // 2][1] + 20, 0.7, 1),
            (gts[0][0], gts[0][1], gts[0][0] + 20, gts[0][1] + 15, 0.6, 0)]
    require(all(iou_xyxy_xywh(dets[0], g) == 0.0 for g in gts[:-1]) and iou_xyxy_xywh(dets[0], gts[-1]) == 0.95, "gt_counts: last ground truth")
    return {"name": f"gt_count_{n}", "K": 2, "images": [(dets, gts)], "G": n}


def class_counts(K):
    """K = 1 and K = 80: every class holds one ground truth and one detection on it; with K = 80 the highest class too"""
    gts = [(30 * (k % 40), 40 * (k // 40), 20, 20, None, k, 0) for k in range(K)]
    dets = [(g[0], g[1], g[0] + 20, g[1] + 20 - (k % 3), 0.9 - 0.01 * k, k) for k, g in enumerate(gts)]
    return {"name": f"classes_{K}", "K": K, "images": [(dets, gts)]}


def too_many_ground_truths():
    """the cap + 1 in one image: the refusal"""
    gts = [(30 * (j % 60), 40 * (j // 60), 20, 20, None, 0, 0) for j in range(G_CAP + 1)]
    require(len(gts) == G_CAP + 1, "cap + 1")
    return [([], gts)]


def all_cases():
    return [threshold_edges(), tied_scores(), tied_iou(), crowd(), area_edges(), extents(), full_detections(),
            gt_counts(63), gt_counts(64), gt_counts(65), gt_counts(G_CAP), class_counts(1), class_counts(80)]


def random_images(seed, n, K, max_det=40, max_gt=20):
    """a randomised set on a half-integer lattice (exact in fp32): detections are jittered ground truths plus clutter"""
    rng = np.random.RandomState(seed)
    images = []
    for _ in range(n):
        ng, gts, dets = int(rng.randint(0, max_gt + 1)), [], []
        for _ in range(ng):
            w, h = rng.randint(8, 200, size=2)
            x, y = rng.randint(0, 800), rng.randint(0, 400)
            gts.append((int(x), int(y), int(w), int(h), None, int(rng.randint(K)), int(rng.rand() < 0.15)))
        for _ in range(int(rng.randint(0, max_det + 1))):
            if gts and rng.rand() < 0.7:
                x, y, w, h, _, c, _ = gts[int(rng.randint(len(gts)))]
                j = rng.randint(-4, 5, size=4) / 2.0
                box = (x + j[0], y + j[1], x + w + j[2], y + h + j[3])
                c = c if rng.rand() < 0.9 else int(rng.randint(K))
            else:
                x, y = rng.randint(0, 800), rng.randint(0, 400)
                box, c = (x, y, x + rng.randint(4, 150), y + rng.randint(4, 150)), int(rng.randint(K))
            dets.append(tuple(float(v) for v in box) + (float(np.float32(rng.randint(1, 64) / 64.0)), c))
        images.append((dets, gts))
    return images


def instances(sfod, images, device, first_id=0):
    """images -> (inputs, outputs) as ``inference_on_dataset`` hands them to an evaluator"""
    import torch
    S = sfod.structures
    inputs, outputs = [], []
    for b, (dets, _) in enumerate(images):
        oi = S.Instances((1024, 2048))
        oi.pred_boxes = S.Boxes(torch.tensor([d[:4] for d in dets], dtype=torch.float32).reshape(-1, 4).to(device))
        oi.scores = torch.tensor([d[4] for d in dets], dtype=torch.float32).to(device)
        oi.pred_classes = torch.tensor([d[5] for d in dets], dtype=torch.int64).to(device)
        inputs.append({"image_id": first_id + b})
        outputs.append({"instances": oi})
    return inputs, outputs
