"""numpy producer of what ``sfod_coco_match`` writes (include/sfod_hip.h), written from ``COCOevalBBox._evaluate_img``
(simple-sfod_amd/evaluation.py), which is the definition: tests/test_coco_match_host.py holds this producer to that code on
every case of tests/helpers/coco_match_cases.py, tests/test_gpu_coco_match.py holds the kernel to this producer.

Plain Python loops over Python floats (IEEE doubles, no contraction): slow and literal on purpose."""
import numpy as np


def _iou(d, g, crowd):
    """one entry of ``bbox_iou_xywh``: d, g are (x, y, w, h) doubles"""
    w = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    h = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if w <= 0 or h <= 0:
        return 0.0
    inter = w * h
    da, ga = d[2] * d[3], g[2] * g[3]
    return inter / (da if crowd else da + ga - inter)


def coco_match(a, K, iou_thrs, area_rng):
    """``a``: the arrays of one packed batch (coco_match_cases.pack) -> rank [B,D] i32, match [B,D] u64, ignore [B,D] u64,
    npig [B,K,A] i32.  Entries beyond the counts are not read."""
    db, ds, dc = a["det_boxes"], a["det_scores"], a["det_classes"]
    B, D = ds.shape
    G = a["gt_classes"].shape[1]
    T, A = len(iou_thrs), len(area_rng)
    rank = np.full((B, D), -1, dtype=np.int32)
    match = np.zeros((B, D), dtype=np.uint64)
    ignore = np.zeros((B, D), dtype=np.uint64)
    npig = np.zeros((B, K, A), dtype=np.int32)
    for b in range(B):
        nd, ng = int(np.clip(a["det_count"][b], 0, D)), int(np.clip(a["gt_count"][b], 0, G))
        w32, h32 = db[b, :nd, 2] - db[b, :nd, 0], db[b, :nd, 3] - db[b, :nd, 1]            # fp32, like instances_to_coco_json
        dxywh = [(float(db[b, i, 0]), float(db[b, i, 1]), float(w32[i]), float(h32[i])) for i in range(nd)]
        gxywh = [tuple(float(v) for v in a["gt_boxes"][b, j]) for j in range(ng)]
        for k in range(K):
            dts = [i for i in range(nd) if dc[b, i] == k]
            gts = [j for j in range(ng) if a["gt_classes"][b, j] == k]
            order = np.argsort([-float(ds[b, i]) for i in dts], kind="mergesort")
            dts = [dts[i] for i in order]
            for r, i in enumerate(dts):
                rank[b, i] = r
            for ai, (lo, hi) in enumerate(area_rng):
                ig = [1 if (a["gt_iscrowd"][b, j] or a["gt_area"][b, j] < lo or a["gt_area"][b, j] > hi) else 0 for j in gts]
                npig[b, k, ai] = ig.count(0)
                vis = [gts[j] for j in np.argsort(ig, kind="mergesort")]
                vig = sorted(ig)
                crowd = [int(a["gt_iscrowd"][b, j]) for j in vis]
                ious = [[_iou(dxywh[i], gxywh[j], c) for j, c in zip(vis, crowd)] for i in dts]
                for ti, t in enumerate(iou_thrs):
                    bit = np.uint64(1) << np.uint64(ai * T + ti)
                    taken = [False] * len(vis)
                    for di, i in enumerate(dts):
                        iou, m = min([t, 1 - 1e-10]), -1
                        for gi in range(len(vis)):
                            if taken[gi] and not crowd[gi]:
                                continue
                            if m > -1 and vig[m] == 0 and vig[gi] == 1:
                                break
                            if ious[di][gi] < iou:
                                continue
                            iou, m = ious[di][gi], gi
                        if m > -1:
                            taken[m] = True
                            match[b, i] |= bit
                            if vig[m]:
                                ignore[b, i] |= bit
                        else:
                            area = dxywh[i][2] * dxywh[i][3]
                            if area < lo or area > hi:
                                ignore[b, i] |= bit
    return rank, match, ignore, npig
