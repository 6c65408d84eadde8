"""Hand-computed F1Evaluator cases and the packing of images into the fixed-capacity arrays, shared by
tests/test_f1_evaluator.py (host rule), tests/test_gpu_f1_evaluator.py (``sfod_f1_count``) and tools/record_f1_golden.py
(which runs the same images through the reference's evaluator for tests/golden/f1_ref.npz).

A case: ``name``, ``K``, ``params`` (iou, top_n, score), ``images`` = [(dets, gts, (h, w))] with dets = [(box, score, class)]
and gts = [(box, class)], and ``counts`` = the expected [K][3] (TP, FP, FN) summed over the images, worked out by hand in the
comment above each case.  Boxes are x1, y1, x2, y2 with the "+1" pixel convention: [0, 0, 9, 9] covers 10 x 10 = 100 pixels.
All boxes lie inside the image and are non-empty, so ``detector_postprocess`` at scale 1 leaves them as they are."""
import numpy as np

S = (100, 100)
DEFAULT = (0.5, 5, 0.5)

HAND_CASES = [
    # ga = 100, da = 10 * 5 = 50, inter = 50: IoU = 50 / (100 + 50 - 50) = 0.5 exactly, and the rule is strict '>'
    dict(name="iou_exactly_half_is_no_match", K=1, params=DEFAULT,
         images=[([([0, 0, 9, 4], 0.9, 0)], [([0, 0, 9, 9], 0)], S)], counts=[[0, 1, 1]]),
    # truncated to [10, 10, 28, 19]: da = 19 * 10 = 190, inter = 100, IoU = 100 / 190 = 0.526 > 0.5.  Left in fp32 the
    # intersection would be (19 - 10.9 + 1) * 10 = 91 and the IoU 91 / (100 + 190 - 91) = 0.457: no match
    dict(name="matches_only_because_it_truncates", K=1, params=DEFAULT,
         images=[([([10.9, 10.0, 28.9, 19.0], 0.9, 0)], [([10, 10, 19, 19], 0)], S)], counts=[[1, 0, 0]]),
    # the boxes share the single pixel (9, 9): inter = 1, IoU = 1 / 199 > 0 = iou (without the "+1" it would be 0)
    dict(name="touching_boxes_overlap_by_one_pixel", K=1, params=(0.0, 5, 0.5),
         images=[([([9, 9, 18, 18], 0.9, 0)], [([0, 0, 9, 9], 0)], S)], counts=[[1, 0, 0]]),
    # '>=' on the score: 0.5 is kept and matches; the largest fp32 below 0.5 is dropped and is not even a false positive
    dict(name="score_exactly_at_the_threshold_is_kept", K=1, params=DEFAULT,
         images=[([([50, 50, 59, 59], float(np.nextafter(np.float32(0.5), np.float32(0))), 0), ([0, 0, 9, 9], 0.5, 0)],
                  [([0, 0, 9, 9], 0)], S)], counts=[[1, 0, 0]]),
    # six detections >= 0.5: the class-1 one (first by index, sixth by score) lies exactly on the class-1 ground truth but is cut
    # by top_n = 5, which ranks over all classes together: class 0 has five false positives, class 1 one false negative
    dict(name="top_n_cuts_across_classes", K=2, params=DEFAULT,
         images=[([([50, 50, 59, 59], 0.70, 1), ([0, 0, 9, 9], 0.95, 0), ([20, 0, 29, 9], 0.90, 0), ([40, 0, 49, 9], 0.85, 0),
                   ([60, 0, 69, 9], 0.80, 0), ([80, 0, 89, 9], 0.75, 0)], [([50, 50, 59, 59], 1)], S)],
         counts=[[0, 5, 0], [0, 0, 1]]),
    # g0 = rows 0..9, g1 = rows 10..19 of a 10-wide column; d0 (0.9, column 0 although it is second by index) covers both,
    # d1 (0.8) covers g0 and the 10 columns right of it.  IoU matrix (rows g0, g1; columns d0, d1) = [[.5, .5], [.5, 0]]:
    # three equal maxima.  The first in row-major order, (g0, d0), leaves only (g1, d1) = 0: TP 1, FP 1, FN 1.  Either other
    # maximum, or columns in index order, leaves a second match: TP 2
    dict(name="equal_maxima_take_the_first_in_row_major_order", K=1, params=(0.3, 5, 0.5),
         images=[([([0, 0, 19, 9], 0.8, 0), ([0, 0, 9, 19], 0.9, 0)], [([0, 0, 9, 9], 0), ([0, 10, 9, 19], 0)], S)],
         counts=[[1, 1, 1]]),
    # one row of height 10: g0 = x 0..19, g1 = x 20..39 (width 20 each), d0 (0.9) = x 4..33 (width 30), d1 (0.8) = x 0..17.
    # IoU(g0, d0) = 16 / 34 = .47, IoU(g1, d0) = 14 / 36 = .39, IoU(g0, d1) = 18 / 20 = .9, IoU(g1, d1) = 0.  By global maximum:
    # (g0, d1), then (g1, d0) = .39 > .3: TP 2.  In score order d0 would take g0 and leave d1 without a partner: TP 1
    dict(name="global_maximum_differs_from_score_order", K=1, params=(0.3, 5, 0.5),
         images=[([([4, 0, 33, 9], 0.9, 0), ([0, 0, 17, 9], 0.8, 0)], [([0, 0, 19, 9], 0), ([20, 0, 39, 9], 0)], S)],
         counts=[[2, 0, 0]]),
    dict(name="wrong_class_on_a_ground_truth_is_fp_plus_fn", K=2, params=DEFAULT,
         images=[([([0, 0, 9, 9], 0.9, 1)], [([0, 0, 9, 9], 0)], S)], counts=[[0, 0, 1], [0, 1, 0]]),
    dict(name="no_detections", K=1, params=DEFAULT,
         images=[([], [([0, 0, 9, 9], 0), ([20, 20, 29, 29], 0)], S)], counts=[[0, 0, 2]]),
    dict(name="no_ground_truth", K=1, params=DEFAULT, images=[([([0, 0, 9, 9], 0.9, 0)], [], S)], counts=[[0, 1, 0]]),
    dict(name="neither", K=1, params=DEFAULT, images=[([], [], S)], counts=[[0, 0, 0]]),
    dict(name="all_detections_below_the_score_threshold", K=1, params=DEFAULT,
         images=[([([0, 0, 9, 9], 0.4, 0), ([0, 0, 9, 9], 0.3, 0)], [([0, 0, 9, 9], 0)], S)], counts=[[0, 0, 1]]),
    # classes 2 and -1 with K = 2: a perfect pair of class 2 and a stray of class -1 are counted nowhere
    dict(name="out_of_range_class_is_counted_nowhere", K=2, params=DEFAULT,
         images=[([([0, 0, 9, 9], 0.9, 2), ([50, 50, 59, 59], 0.8, 0), ([70, 70, 79, 79], 0.7, -1)],
                  [([0, 0, 9, 9], 2), ([50, 50, 59, 59], 0)], S)], counts=[[1, 0, 0], [0, 0, 0]]),
    # two images: the counts add up (first: one match; second: a miss and a false positive of class 1)
    dict(name="two_images_add_up", K=2, params=DEFAULT,
         images=[([([0, 0, 9, 9], 0.9, 0)], [([0, 0, 9, 9], 0)], S),
                 ([([60, 60, 69, 69], 0.9, 1)], [([0, 0, 9, 9], 1)], (80, 120))], counts=[[1, 0, 0], [0, 1, 1]]),
]


def pack(images, cap_d=None, cap_g=None, poison=False):
    """[(dets, gts, (h, w))] -> dict of numpy arrays in the fixed-capacity layout (scale 1, clip = the image size).
    ``poison``: the entries beyond the counts hold boxes that would match (a copy of the image's first box, score 0.99,
    class 0) instead of zeros."""
    B = len(images)
    D = cap_d if cap_d is not None else max([len(d) for d, _, _ in images] + [1])
    G = cap_g if cap_g is not None else max([len(g) for _, g, _ in images] + [1])
    out = dict(det_boxes=np.zeros((B, D, 4), np.float32), det_scores=np.zeros((B, D), np.float32),
               det_classes=np.zeros((B, D), np.int32), det_count=np.zeros(B, np.int32),
               gt_boxes=np.zeros((B, G, 4), np.float32), gt_classes=np.zeros((B, G), np.int32),
               gt_count=np.zeros(B, np.int32), scale=np.ones((B, 2), np.float32), clip_size=np.zeros((B, 2), np.int32))
    for i, (dets, gts, size) in enumerate(images):
        if poison:
            first = (gts[0][0] if gts else (dets[0][0] if dets else [0, 0, 9, 9]))
            out["det_boxes"][i], out["gt_boxes"][i], out["det_scores"][i] = first, first, 0.99
        for j, (box, score, cls) in enumerate(dets):
            out["det_boxes"][i, j], out["det_scores"][i, j], out["det_classes"][i, j] = box, score, cls
        for j, (box, cls) in enumerate(gts):
            out["gt_boxes"][i, j], out["gt_classes"][i, j] = box, cls
        out["det_count"][i], out["gt_count"][i], out["clip_size"][i] = len(dets), len(gts), size
    return out


def fixture_images(z):
    """tests/golden/f1_ref.npz -> [(K, det_boxes [n,4], det_scores [n], det_classes [n], gt_boxes [m,4], gt_classes [m], (h, w))]"""
    do, go = np.concatenate([[0], np.cumsum(z["nd"])]), np.concatenate([[0], np.cumsum(z["ng"])])
    return [(int(z["K"][i]), z["det_boxes"][do[i]:do[i + 1]], z["det_scores"][do[i]:do[i + 1]], z["det_classes"][do[i]:do[i + 1]],
             z["gt_boxes"][go[i]:go[i + 1]], z["gt_classes"][go[i]:go[i + 1]], tuple(int(v) for v in z["sizes"][i]))
            for i in range(len(z["K"]))]


def pack_arrays(imgs, cap_d=100, cap_g=100):
    """a list of ``fixture_images`` entries -> the fixed-capacity layout (as ``pack``)"""
    return pack([([(b, s, c) for b, s, c in zip(db, ds, dc)], [(b, c) for b, c in zip(gb, gc)], size)
                 for _, db, ds, dc, gb, gc, size in imgs], cap_d, cap_g)
