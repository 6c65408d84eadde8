"""Evaluation path: ``Trainer.test`` -> ``inference_on_dataset`` -> COCO-style
box AP with the per-class AP / AP50 table of ``daod/evaluation/new_cocoevaluator.py:33-112``.

The reference's evaluator is Detectron2's ``COCOEvaluator`` (``process`` / ``evaluate``) around pycocotools'
``COCOeval``; neither is vendored nor installed here, so the scoring arithmetic below restates pycocotools'
published algorithm (``cocoeval.py``: ``computeIoU``, ``evaluateImg``, ``accumulate``, ``summarize``; bbox
IoU type, default parameters: IoU .50:.05:.95, 101 recall points, maxDets 1/10/100, areas all / small <32^2 /
medium / large >96^2, crowd ground truth matched as "ignore" with intersection-over-detection-area).
Parity unpinned: checked against hand-computed cases (``tests/test_evaluation.py``), not against pycocotools.
Host-side numpy like the reference's (the model's forward is the device work); not on the timed path.
The reference also appends an ``F1Evaluator`` (``base.py:149``): built here as ``F1Evaluator`` (below), the one evaluator
that counts on the device (``sfod_f1_count``) and reads back once, in ``evaluate()``; ``SFOD.EVALUATORS ("coco", "f1")``
puts both behind ``DatasetEvaluators`` as the reference does.
``SFOD.COCO_EVAL_DEVICE`` (``NewCOCOEvaluator(device_match=True)``) moves COCOeval's matching to the device the same way:
``process`` packs the batch, ``sfod_coco_match`` applies ``COCOevalBBox._evaluate_img``'s rule per image, ``evaluate()`` makes
one copy and hands ``accumulate()`` what it consumes.  ``COCOevalBBox.evaluate`` stays the definition of that rule.
"""
import copy
import itertools
import logging
import time
from collections import OrderedDict, defaultdict

import numpy as np
import torch

from .modeling.batched import GT_CAP, BatchedGT

logger = logging.getLogger("sfod")

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
COCO_DET_CAP = MAX_DETS[-1]       # detections per image the device path packs (TEST.DETECTIONS_PER_IMAGE's default)
COCO_GT_CAP = 256                 # ground truths per image the device path packs (sfod_coco_match: G <= 256)


def bbox_iou_xywh(dt, gt, iscrowd):
    """pycocotools ``maskUtils.iou`` for boxes: [D,4] x [G,4] (x,y,w,h) -> [D,G]; for a crowd ground truth
    the union is the detection's area."""
    dt = np.asarray(dt, dtype=np.float64).reshape(-1, 4)
    gt = np.asarray(gt, dtype=np.float64).reshape(-1, 4)
    out = np.zeros((len(dt), len(gt)))
    for j in range(len(gt)):
        ga = gt[j, 2] * gt[j, 3]
        for i in range(len(dt)):
            da = dt[i, 2] * dt[i, 3]
            w = min(dt[i, 0] + dt[i, 2], gt[j, 0] + gt[j, 2]) - max(dt[i, 0], gt[j, 0])
            h = min(dt[i, 1] + dt[i, 3], gt[j, 1] + gt[j, 3]) - max(dt[i, 1], gt[j, 1])
            if w <= 0 or h <= 0:
                continue
            inter = w * h
            out[i, j] = inter / (da if iscrowd[j] else da + ga - inter)
    return out


class COCOevalBBox:
    """``COCOeval(cocoGt, cocoDt, "bbox")``: ``evaluate(); accumulate(); summarize()`` -> ``stats`` [12],
    ``eval["precision"]`` [T,R,K,A,M] and ``eval["recall"]`` [T,K,A,M]."""

    def __init__(self, gt_anns, dt_anns, cat_ids, img_ids):
        self.cat_ids, self.img_ids = sorted(set(cat_ids)), sorted(set(img_ids))
        self._gts, self._dts = defaultdict(list), defaultdict(list)
        for i, g in enumerate(gt_anns):
            g = dict(g)
            g.setdefault("iscrowd", 0)
            g.setdefault("area", g["bbox"][2] * g["bbox"][3])
            g.setdefault("id", i + 1)
            g["ignore"] = g.get("ignore", 0) or g["iscrowd"]
            self._gts[g["image_id"], g["category_id"]].append(g)
        for i, d in enumerate(dt_anns):            # COCO.loadRes: area = w*h, id = running index
            d = dict(d)
            d["area"] = d["bbox"][2] * d["bbox"][3]
            d["id"] = i + 1
            self._dts[d["image_id"], d["category_id"]].append(d)
        self.eval, self.stats = {}, None

    def _evaluate_img(self, img, cat, arng, max_det, ious_cache):
        gt, dt = self._gts[img, cat], self._dts[img, cat]
        if len(gt) == 0 and len(dt) == 0:
            return None
        g_ignore = np.array([1 if (g["ignore"] or g["area"] < arng[0] or g["area"] > arng[1]) else 0 for g in gt])
        gtind = np.argsort(g_ignore, kind="mergesort")
        gt = [gt[i] for i in gtind]
        dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
        dt = [dt[i] for i in dtind[0:max_det]]
        iscrowd = [int(o["iscrowd"]) for o in gt]
        ious = ious_cache[img, cat]
        ious = ious[:, gtind] if len(ious) > 0 else ious
        T, G, D = len(IOU_THRS), len(gt), len(dt)
        gtm, dtm = np.zeros((T, G)), np.zeros((T, D))
        gt_ig = np.array([g_ignore[i] for i in gtind]) if G else np.zeros(0)
        dt_ig = np.zeros((T, D))
        if len(ious) != 0:
            for tind, t in enumerate(IOU_THRS):
                for dind in range(D):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind in range(G):
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:
                            continue
                        if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                            break
                        if ious[dind, gind] < iou:
                            continue
                        iou = ious[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dt_ig[tind, dind] = gt_ig[m]
                    dtm[tind, dind] = gt[m]["id"]
                    gtm[tind, m] = dt[dind]["id"]
        a = np.array([d["area"] < arng[0] or d["area"] > arng[1] for d in dt]).reshape((1, len(dt)))
        dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return {"dtMatches": dtm, "dtScores": [d["score"] for d in dt], "gtIgnore": gt_ig, "dtIgnore": dt_ig}

    def evaluate(self):
        ious = {}
        for img in self.img_ids:
            for cat in self.cat_ids:
                gt, dt = self._gts[img, cat], self._dts[img, cat]
                if len(gt) == 0 and len(dt) == 0:
                    ious[img, cat] = []
                    continue
                inds = np.argsort([-d["score"] for d in dt], kind="mergesort")
                dt = [dt[i] for i in inds][: MAX_DETS[-1]]
                ious[img, cat] = bbox_iou_xywh([d["bbox"] for d in dt], [g["bbox"] for g in gt],
                                               [int(g["iscrowd"]) for g in gt])
        self._eval_imgs = [self._evaluate_img(img, cat, arng, MAX_DETS[-1], ious)
                           for cat in self.cat_ids for arng in AREA_RNG for img in self.img_ids]

    def accumulate(self):
        T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(self.cat_ids), len(AREA_RNG), len(MAX_DETS)
        precision = -np.ones((T, R, K, A, M))
        recall = -np.ones((T, K, A, M))
        I0 = len(self.img_ids)
        for k in range(K):
            for a in range(A):
                for m, max_det in enumerate(MAX_DETS):
                    E = [self._eval_imgs[k * A * I0 + a * I0 + i] for i in range(I0)]
                    E = [e for e in E if e is not None]
                    if len(E) == 0:
                        continue
                    dt_scores = np.concatenate([e["dtScores"][0:max_det] for e in E])
                    inds = np.argsort(-dt_scores, kind="mergesort")
                    dtm = np.concatenate([e["dtMatches"][:, 0:max_det] for e in E], axis=1)[:, inds]
                    dt_ig = np.concatenate([e["dtIgnore"][:, 0:max_det] for e in E], axis=1)[:, inds]
                    gt_ig = np.concatenate([e["gtIgnore"] for e in E])
                    npig = np.count_nonzero(gt_ig == 0)
                    if npig == 0:
                        continue
                    tps = np.logical_and(dtm, np.logical_not(dt_ig))
                    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                    tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                    fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                    for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                        nd = len(tp)
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        q = np.zeros((R,))
                        recall[t, k, a, m] = rc[-1] if nd else 0
                        pr = pr.tolist()
                        for i in range(nd - 1, 0, -1):
                            if pr[i] > pr[i - 1]:
                                pr[i - 1] = pr[i]
                        inds_r = np.searchsorted(rc, REC_THRS, side="left")
                        for ri, pi in enumerate(inds_r):
                            if pi >= nd:
                                break
                            q[ri] = pr[pi]
                        precision[t, :, k, a, m] = q
        self.eval = {"precision": precision, "recall": recall}

    def _summarize(self, ap, iou_thr=None, area=0, max_det=100):
        mind = MAX_DETS.index(max_det)
        s = self.eval["precision"] if ap else self.eval["recall"]
        if iou_thr is not None:
            s = s[np.where(np.isclose(IOU_THRS, iou_thr))[0]]
        s = s[:, :, :, area, mind] if ap else s[:, :, area, mind]
        return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))

    def summarize(self):
        z = self._summarize
        self.stats = np.array([z(1), z(1, .5), z(1, .75), z(1, area=1), z(1, area=2), z(1, area=3),
                               z(0, max_det=1), z(0, max_det=10), z(0), z(0, area=1), z(0, area=2), z(0, area=3)])
        return self.stats


def instances_to_coco_json(instances, img_id):
    """d2 ``instances_to_coco_json`` for boxes: XYXY -> XYWH, one dict per detection."""
    if len(instances) == 0:
        return []
    boxes = instances.pred_boxes.tensor.detach().float().cpu().numpy().copy()
    boxes[:, 2] -= boxes[:, 0]
    boxes[:, 3] -= boxes[:, 1]
    scores = instances.scores.detach().float().cpu().tolist()
    classes = instances.pred_classes.detach().cpu().tolist()
    return [{"image_id": img_id, "category_id": int(classes[k]), "bbox": boxes[k].tolist(), "score": scores[k]}
            for k in range(len(scores))]


def coco_compact(image_ids, det_count, det_scores, det_classes, rank, match, ignore, npig):
    """What ``sfod_coco_match`` leaves of a set of images, without the padding: a dict of numpy arrays keyed by image id.
    ``image_id`` (list, I entries), ``count`` [I] i32, ``npig`` [I,K,A] i32, and per detection below its image's count
    (N = sum of the counts, image after image, index order) ``det_image`` (the row in ``image_id``), ``det_class``,
    ``det_score`` f32, ``det_rank`` (-1: in no category), ``det_match`` / ``det_ignore`` u64 (bit a * T + t)."""
    count = np.clip(np.asarray(det_count, dtype=np.int32).reshape(-1), 0, np.asarray(rank).shape[1])
    I, D = np.asarray(rank).shape
    assert len(image_ids) == I == len(count)
    img, slot = np.nonzero(np.arange(D)[None, :] < count[:, None])
    return {"image_id": list(image_ids), "count": count, "npig": np.asarray(npig, dtype=np.int32).reshape(I, *np.shape(npig)[1:]),
            "det_image": img.astype(np.int32), "det_class": np.asarray(det_classes, dtype=np.int32)[img, slot],
            "det_score": np.asarray(det_scores, dtype=np.float32)[img, slot], "det_rank": np.asarray(rank, dtype=np.int32)[img, slot],
            "det_match": np.asarray(match).view(np.uint64)[img, slot], "det_ignore": np.asarray(ignore).view(np.uint64)[img, slot]}


def coco_compact_merge(parts):
    """The compact arrays of several shares (the ranks', in rank order) as one: rows appended, ``det_image`` shifted."""
    parts = [p for p in parts if len(p["image_id"])]
    if len(parts) == 1:
        return parts[0]
    if not parts:
        raise ValueError("coco_compact_merge: nothing to merge")
    base = np.cumsum([0] + [len(p["image_id"]) for p in parts[:-1]])
    out = {"image_id": list(itertools.chain(*[p["image_id"] for p in parts])),
           "det_image": np.concatenate([p["det_image"] + np.int32(b) for p, b in zip(parts, base)])}
    for k in ("count", "npig", "det_class", "det_score", "det_rank", "det_match", "det_ignore"):
        out[k] = np.concatenate([p[k] for p in parts])
    return out


class NewCOCOEvaluator:
    """``NewCOCOEvaluator(dataset_name, output_dir=...)`` (``new_cocoevaluator.py:33``): d2's ``reset`` /
    ``process`` / ``evaluate`` protocol; ``evaluate`` returns ``OrderedDict(bbox={AP, AP50, AP75, APs, APm,
    APl, "AP-<class>", "AP-<class>_AP50"})`` in percent, NaN where undefined.  ``dataset_dicts`` are d2
    dataset records (``annotations`` with ``bbox`` XYWH_ABS / ``category_id`` / ``iscrowd``).
    ``device_match`` (``SFOD.COCO_EVAL_DEVICE``): CUDA instances are packed into fixed-capacity arrays next to their image's
    rows of the ground-truth table and matched by ``native.coco_match`` -- no ``.cpu()``, no synchronisation in ``process``;
    ``evaluate()`` copies the kernel's words once, rebuilds ``COCOevalBBox._eval_imgs`` from them and runs the same
    ``accumulate`` / ``summarize``.  Host instances take the host path whatever the flag says; both kinds
    in one round are a ``ValueError`` in ``evaluate()``.  ``timings`` holds the seconds
    the last device-path ``evaluate()`` spent in the copy, the rebuild and ``accumulate`` + ``summarize``, ``coco_eval`` its
    ``COCOevalBBox``."""

    METRICS = ["AP", "AP50", "AP75", "APs", "APm", "APl"]

    def __init__(self, dataset_name, dataset_dicts, class_names, distributed=True, output_dir=None, device_match=False):
        self.dataset_name, self.class_names = dataset_name, list(class_names)
        self._device_match = bool(device_match)
        self._distributed, self._output_dir = distributed, output_dir
        self._gt = []
        self._img_ids = []
        for rec in dataset_dicts:
            self._img_ids.append(rec["image_id"])
            for ann in rec.get("annotations", []):
                x, y, w, h = ann["bbox"]
                if ann.get("bbox_mode", 1) == 0:          # XYXY_ABS -> XYWH_ABS
                    w, h = w - x, h - y
                self._gt.append({"image_id": rec["image_id"], "category_id": int(ann["category_id"]),
                                 "bbox": [x, y, w, h], "iscrowd": int(ann.get("iscrowd", 0)),
                                 "area": float(ann.get("area", w * h))})
        if self._device_match:
            self._build_gt_table()
        self.reset()

    def reset(self):
        self._predictions = []
        if self._device_match:
            self._matched, self.timings = [], {}

    def _build_gt_table(self):
        """``self._gt`` as arrays, annotation order, and each image's rows in them (what ``process`` stages per batch)."""
        n = len(self._gt)
        self._gt_f64 = np.zeros((n, 5), dtype=np.float64)                    # bbox XYWH | area
        self._gt_i32 = np.zeros((n, 2), dtype=np.int32)                      # category_id | iscrowd
        rows = defaultdict(list)
        for j, g in enumerate(self._gt):
            self._gt_f64[j, :4], self._gt_f64[j, 4] = g["bbox"], g["area"]
            self._gt_i32[j] = g["category_id"], g["iscrowd"]
            rows[g["image_id"]].append(j)
        self._gt_rows = {k: np.asarray(v, dtype=np.int64) for k, v in rows.items()}
        for image_id, r in self._gt_rows.items():
            if len(r) > COCO_GT_CAP:
                raise ValueError(f"NewCOCOEvaluator(device_match=True): image {image_id!r} has {len(r)} ground-truth boxes, "
                                 f"above the device path's cap of {COCO_GT_CAP}; use the host path (SFOD.COCO_EVAL_DEVICE False)")

    def process(self, inputs, outputs):
        if self._device_match and len(outputs) and all("instances" in o and o["instances"].scores.is_cuda for o in outputs):
            return self._process_device(inputs, outputs)
        for inp, out in zip(inputs, outputs):
            pred = {"image_id": inp["image_id"]}
            if "instances" in out:
                pred["instances"] = instances_to_coco_json(out["instances"], inp["image_id"])
            self._predictions.append(pred)

    def _process_device(self, inputs, outputs):
        insts = [o["instances"] for o in outputs]
        ids = [i["image_id"] for i in inputs]
        B, D, G = len(insts), COCO_DET_CAP, COCO_GT_CAP
        nds = [len(oi) for oi in insts]
        for image_id, n in zip(ids, nds):
            if n > D:
                raise ValueError(f"NewCOCOEvaluator(device_match=True): image {image_id!r} has {n} detections, more than {D} "
                                 "(TEST.DETECTIONS_PER_IMAGE); the host path truncates them per category, the device path refuses")
        dev = insts[0].scores.device
        N = sum(nds)
        empty = np.zeros(0, dtype=np.int64)
        grows = [self._gt_rows.get(i, empty) for i in ids]
        # host numbers (tensor shapes, the evaluator's own table) are staged in pinned memory and uploaded without blocking;
        # the detections' values never leave the device: one concatenation and one row scatter per field
        ints = torch.empty(2 * B + 2 * B * G, dtype=torch.int32, pin_memory=True)   # det counts | gt counts | category | iscrowd
        f64 = torch.empty(5 * B * G, dtype=torch.float64, pin_memory=True)          # bbox [B,G,4] | area [B,G]
        rows = torch.empty(N, dtype=torch.int64, pin_memory=True)
        ints_h, f64_h, rows_h = ints.numpy(), f64.numpy(), rows.numpy()
        ints_h[:B], ints_h[B:2 * B] = nds, [len(r) for r in grows]
        cat_h, crowd_h = ints_h[2 * B:2 * B + B * G].reshape(B, G), ints_h[2 * B + B * G:].reshape(B, G)
        box_h, area_h = f64_h[:4 * B * G].reshape(B, G, 4), f64_h[4 * B * G:].reshape(B, G)
        for b, r in enumerate(grows):
            box_h[b, :len(r)], area_h[b, :len(r)] = self._gt_f64[r, :4], self._gt_f64[r, 4]
            cat_h[b, :len(r)], crowd_h[b, :len(r)] = self._gt_i32[r, 0], self._gt_i32[r, 1]
        if N:
            rows_h[:] = np.concatenate([i * D + np.arange(n) for i, n in enumerate(nds)])
        ints, f64, rows = (t.to(dev, non_blocking=True) for t in (ints, f64, rows))

        def scatter(parts, dtype, *tail):
            out = torch.empty(B * D, *tail, dtype=dtype, device=dev)
            if N:
                out.index_copy_(0, rows, torch.cat([p.detach() for p in parts]).to(device=dev, dtype=dtype, non_blocking=True))
            return out.view(B, D, *tail)
        db = scatter([oi.pred_boxes.tensor for oi in insts], torch.float32, 4)      # as the model returned them: no scale
        ds = scatter([oi.scores for oi in insts], torch.float32)
        dc = scatter([oi.pred_classes for oi in insts], torch.int32)
        from . import native
        rank, match, ignore, npig = native.coco_match(
            db, ds, dc, ints[:B], f64[:4 * B * G].view(B, G, 4), f64[4 * B * G:].view(B, G),
            ints[2 * B:2 * B + B * G].view(B, G), ints[2 * B + B * G:].view(B, G), ints[B:2 * B], len(self.class_names),
            IOU_THRS, AREA_RNG)
        self.add_matched(ids, ds, dc, ints[:B], rank, match, ignore, npig)

    def add_matched(self, image_ids, det_scores, det_classes, det_count, rank, match, ignore, npig):
        """Container-level entry: one batch's scores / classes / counts and what ``native.coco_match`` wrote for it (tensors of
        any one device; they stay there until ``evaluate()``)."""
        self._matched.append((list(image_ids), det_count, det_scores, det_classes, rank, match, ignore, npig))

    def _compact(self):
        """this rank's batches -> ``coco_compact`` arrays, through ONE device-to-host copy"""
        if not self._matched:
            K = len(self.class_names)
            z = np.zeros((0, COCO_DET_CAP))
            return coco_compact([], np.zeros(0), z, z, z, z.astype(np.int64), z.astype(np.int64), np.zeros((0, K, len(AREA_RNG))))
        ids = list(itertools.chain(*[m[0] for m in self._matched]))
        fields = [torch.cat([m[j] for m in self._matched]) for j in (5, 6, 4, 2, 3, 7, 1)]   # 8-byte words first: aligned views
        flat = torch.cat([f.contiguous().view(-1).view(torch.uint8) for f in fields]).cpu().numpy()
        out, at = [], 0
        for f, dt in zip(fields, (np.int64, np.int64, np.int32, np.float32, np.int32, np.int32, np.int32)):
            n = f.numel() * f.element_size()
            out.append(flat[at:at + n].view(dt).reshape(tuple(f.shape)))
            at += n
        match, ignore, rank, scores, classes, npig, count = out
        return coco_compact(ids, count, scores, classes, rank, match, ignore, npig)

    def _eval_imgs_from_compact(self, c, coco_eval):
        """``COCOevalBBox._eval_imgs`` (category x area range x image) as ``accumulate()`` reads it, from the compact arrays:
        ``dtMatches`` nonzero where the bit is set, ``dtIgnore``, ``dtScores`` in the category's order, ``gtIgnore`` with one
        zero per ground truth that counts."""
        K, A, T, I0 = len(coco_eval.cat_ids), len(AREA_RNG), len(IOU_THRS), len(coco_eval.img_ids)
        pos = {image_id: i for i, image_id in enumerate(coco_eval.img_ids)}
        known = np.array([i in pos for i in c["image_id"]], dtype=bool)
        ipos = np.array([pos.get(i, 0) for i in c["image_id"]], dtype=np.int64)
        npig = np.zeros((I0, K, A), dtype=np.int64)
        gt_any = np.zeros((I0, K), dtype=bool)
        seen = np.zeros(I0, dtype=bool)
        npig[ipos[known]], seen[ipos[known]] = c["npig"][known], True
        lo, hi = np.array(AREA_RNG, dtype=np.float64).T
        for g in self._gt:                                   # which (image, category) pairs have ground truth at all; the
            i, k = pos.get(g["image_id"]), g["category_id"]  # counts of an image that no rank processed
            if i is None or not 0 <= k < K:
                continue
            gt_any[i, k] = True
            if not seen[i]:
                npig[i, k] += ~(bool(g["iscrowd"]) | (g["area"] < lo) | (g["area"] > hi))
        keep = (c["det_rank"] >= 0) & known[c["det_image"]] if len(c["det_rank"]) else np.zeros(0, dtype=bool)
        di, dk, dr = ipos[c["det_image"][keep]], c["det_class"][keep].astype(np.int64), c["det_rank"][keep]
        order = np.lexsort((dr, dk, di))
        key = (di * K + dk)[order]
        bits = np.arange(A * T, dtype=np.uint64)
        words = lambda w: np.ascontiguousarray((((w[keep][order][:, None] >> bits) & np.uint64(1)) != 0).reshape(-1, A, T).transpose(1, 2, 0))
        dtm, dtig = words(c["det_match"]).astype(np.float64), words(c["det_ignore"])
        scores = c["det_score"][keep][order].astype(np.float64)
        start = np.searchsorted(key, np.arange(I0 * K), side="left").reshape(I0, K)
        end = np.searchsorted(key, np.arange(I0 * K), side="right").reshape(I0, K)
        zeros = np.zeros(int(npig.max()) if npig.size else 0)
        out = [None] * (K * A * I0)
        for k in range(K):
            for i in range(I0):
                s, e = start[i, k], end[i, k]
                if s == e and not gt_any[i, k]:
                    continue
                sc = scores[s:e]
                for a in range(A):
                    out[k * A * I0 + a * I0 + i] = {"dtMatches": dtm[a][:, s:e], "dtScores": sc, "gtIgnore": zeros[:npig[i, k, a]],
                                                    "dtIgnore": dtig[a][:, s:e]}
        return out

    def _evaluate_matched(self):
        t0 = time.perf_counter()
        compact = self._compact()
        t1 = time.perf_counter()
        dist = torch.distributed
        if self._distributed and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            gathered = [None] * dist.get_world_size()
            dist.all_gather_object(gathered, compact)
            if dist.get_rank() != 0:
                return {}
            if any(len(p["image_id"]) for p in gathered):
                compact = coco_compact_merge(gathered)
        if len(compact["image_id"]) == 0:
            logger.warning("[COCOEvaluator] Did not receive valid predictions.")
            return {}
        results = OrderedDict()
        coco_eval = None
        t2 = t3 = time.perf_counter()
        if int(compact["count"].sum()) > 0:
            coco_eval = COCOevalBBox(self._gt, [], range(len(self.class_names)), self._img_ids)
            coco_eval._eval_imgs = self._eval_imgs_from_compact(compact, coco_eval)
            t3 = time.perf_counter()
            coco_eval.accumulate()
            coco_eval.summarize()
        self.coco_eval = coco_eval
        self.timings = {"copy_s": t1 - t0, "rebuild_s": t3 - t2, "accumulate_s": time.perf_counter() - t3}
        results["bbox"] = self._derive_coco_results(coco_eval, "bbox", self.class_names)
        return copy.deepcopy(results)

    def evaluate(self):
        if self._device_match and self._matched and self._predictions:
            raise ValueError("NewCOCOEvaluator(device_match=True): batches of device tensors and of host tensors (or outputs "
                             "without 'instances') were processed in one round; the two paths cannot be mixed")
        if self._device_match and (self._matched or not self._predictions):
            return self._evaluate_matched()
        preds = self._predictions
        if self._distributed and torch.distributed.is_available() and torch.distributed.is_initialized() \
                and torch.distributed.get_world_size() > 1:
            gathered = [None] * torch.distributed.get_world_size()
            torch.distributed.all_gather_object(gathered, preds)
            preds = list(itertools.chain(*gathered))
            if torch.distributed.get_rank() != 0:
                return {}
        if len(preds) == 0:
            logger.warning("[COCOEvaluator] Did not receive valid predictions.")
            return {}
        results = OrderedDict()
        if "instances" in preds[0]:
            coco_results = list(itertools.chain(*[p["instances"] for p in preds]))
            coco_eval = None
            if len(coco_results) > 0:
                coco_eval = COCOevalBBox(self._gt, coco_results, range(len(self.class_names)), self._img_ids)
                coco_eval.evaluate()
                coco_eval.accumulate()
                coco_eval.summarize()
            results["bbox"] = self._derive_coco_results(coco_eval, "bbox", self.class_names)
        return copy.deepcopy(results)

    def _derive_coco_results(self, coco_eval, iou_type, class_names=None):
        """``new_cocoevaluator.py:34-112``: the six standard numbers + per-category AP and AP50."""
        metrics = self.METRICS
        if coco_eval is None:
            logger.warning("No predictions from the model!")
            return {metric: float("nan") for metric in metrics}
        results = {metric: float(coco_eval.stats[idx] * 100 if coco_eval.stats[idx] >= 0 else "nan")
                   for idx, metric in enumerate(metrics)}
        if class_names is None or len(class_names) <= 1:
            return results
        precisions = coco_eval.eval["precision"]           # (iou, recall, cls, area range, max dets)
        assert len(class_names) == precisions.shape[2]
        per_category = []
        for idx, name in enumerate(class_names):
            precision = precisions[:, :, idx, 0, -1]
            p50 = precision[0]
            p50 = p50[p50 > -1]
            ap50 = np.mean(p50) if p50.size else float("nan")
            precision = precision[precision > -1]
            ap = np.mean(precision) if precision.size else float("nan")
            per_category.append((name, float(ap * 100)))
            per_category.append((name + "_AP50", float(ap50 * 100)))
        results.update({"AP-" + name: ap for name, ap in per_category})
        return results


def f1_image_counts(det_boxes, det_scores, det_classes, gt_boxes, gt_classes, sx, sy, height, width, class_number,
                    iou=0.5, top_n=5, score=0.5):
    """The F1Evaluator's rule for ONE image in numpy (the host definition; ``sfod_f1_count`` is the same rule on the
    device) -> [class_number, 3] int64 (TP, FP, FN).
      1. ``detector_postprocess`` to the loader's scale: fp32 multiply by ``float32(sx)`` / ``float32(sy)``, clip to
         [0, width] x [0, height], drop width <= 0 or height <= 0;  2. keep ``score_i >= float32(score)``;
      3. the ``top_n`` highest scores over all classes (equal scores: the later index first; the reference's order among
         them is whatever its unstable sort leaves);  4. detection coordinates truncated toward zero to int32;
      5. "+1" IoU of (ground truth, kept detection) pairs of equal class: ground-truth area in fp32, detection area in
         int32, intersection and quotient in fp64;  6. while the matrix maximum is > ``iou``: its first position in
         row-major order (ground truths by index x detections by descending score) is a match, its row and column are
         zeroed;  7. per class TP = matched ground truths, FP = kept detections not matched, FN = ground truths not matched;
         classes outside [0, class_number) are counted nowhere."""
    K = int(class_number)
    f32 = np.float32
    b = np.asarray(det_boxes, dtype=f32).reshape(-1, 4) * np.array([sx, sy, sx, sy], dtype=f32)
    s = np.asarray(det_scores, dtype=f32).reshape(-1)
    dk = np.asarray(det_classes).reshape(-1).astype(np.int64)
    b[:, 0::2] = np.clip(b[:, 0::2], f32(0), f32(width))
    b[:, 1::2] = np.clip(b[:, 1::2], f32(0), f32(height))
    ok = np.nonzero((b[:, 2] - b[:, 0] > 0) & (b[:, 3] - b[:, 1] > 0) & (s >= f32(score)))[0]
    keep = ok[np.lexsort((-ok, -s[ok]))][: int(top_n)]             # descending score, then descending index
    d = b[keep].astype(np.int32)
    dk = dk[keep]
    g = np.asarray(gt_boxes, dtype=f32).reshape(-1, 4)
    gk = np.asarray(gt_classes).reshape(-1).astype(np.int64)
    gm, dm = np.zeros(len(g), dtype=bool), np.zeros(len(d), dtype=bool)
    if len(g) and len(d):
        ga = (g[:, 2] - g[:, 0] + f32(1)) * (g[:, 3] - g[:, 1] + f32(1))                      # fp32
        da = (d[:, 2] - d[:, 0] + 1) * (d[:, 3] - d[:, 1] + 1)                                # int32
        g64, d64 = g.astype(np.float64), d.astype(np.float64)
        iw = np.maximum(0.0, np.minimum(g64[:, None, 2], d64[None, :, 2]) - np.maximum(g64[:, None, 0], d64[None, :, 0]) + 1)
        ih = np.maximum(0.0, np.minimum(g64[:, None, 3], d64[None, :, 3]) - np.maximum(g64[:, None, 1], d64[None, :, 1]) + 1)
        inter = iw * ih
        m = inter / ((ga.astype(np.float64)[:, None] + da.astype(np.float64)[None, :]) - inter)
        m[gk[:, None] != dk[None, :]] = 0.0
        while True:
            at = int(np.argmax(m))                                 # the first maximum in row-major order
            i, j = divmod(at, len(d))
            if not m[i, j] > float(iou):
                break
            m[i, :] = 0.0
            m[:, j] = 0.0
            gm[i] = dm[j] = True
    out = np.zeros((K, 3), dtype=np.int64)
    gin, din = (gk >= 0) & (gk < K), (dk >= 0) & (dk < K)
    out[:, 0] = np.bincount(gk[gin & gm], minlength=K)
    out[:, 1] = np.bincount(dk[din & ~dm], minlength=K)
    out[:, 2] = np.bincount(gk[gin & ~gm], minlength=K)
    return out


class F1Evaluator:
    """``F1Evaluator(class_number, iou=0.5, top_n=5, score=0.5)`` (``daod/evaluation/f1_evaluator.py``): d2's ``reset`` /
    ``process`` / ``evaluate`` protocol; ``evaluate`` returns ``{"F1 Score": 2pr / (p + r)}`` from the TP / FP / FN summed
    over images and classes (``f1_image_counts`` has the rule).  Device tensors are packed into the fixed-capacity layout
    with torch ops and counted by ``native.f1_count`` into a device accumulator: no host synchronisation before
    ``evaluate()``, which makes the one device-to-host copy.  Host tensors (``MODEL.DEVICE cpu``) run the numpy rule.
    ``counts`` ([class_number, 3] int64: TP, FP, FN per class) holds the table behind the last ``evaluate()``.
    Ranks: the reference scores rank 0's share only (nothing is gathered); here the counts are summed over the ranks
    with one all-reduce, the dict is returned on rank 0 and ``{}`` elsewhere."""

    def __init__(self, class_number, iou=0.5, top_n=5, score=0.5, distributed=True):
        self.class_number, self.iou, self.top_n, self.score = int(class_number), iou, top_n, score
        self._distributed = distributed
        self.reset()

    def reset(self):
        self._host = np.zeros((self.class_number, 3), dtype=np.int64)
        self._dev = None
        self.counts = np.zeros((self.class_number, 3), dtype=np.int64)

    def process(self, inputs, outputs):
        pairs = [(i["instances"], o["instances"]) for i, o in zip(inputs, outputs) if "instances" in o]
        if not pairs:
            return
        pairs = [(gi.materialize() if hasattr(gi, "materialize") else gi, oi) for gi, oi in pairs]
        B, cap = len(pairs), GT_CAP
        for gi, oi in pairs:
            if len(oi) > cap or len(gi) > cap:
                raise ValueError(f"F1Evaluator: more than {cap} detections or ground-truth boxes in one image "
                                 f"({len(oi)}, {len(gi)})")
        dev = pairs[0][1].scores.device
        pin = dev.type == "cuda"
        nds, ngs = [len(oi) for _, oi in pairs], [len(gi) for gi, _ in pairs]
        N, M = sum(nds), sum(ngs)
        # lengths, sizes, scales and the rows each image's entries go to are host numbers (tensor shapes,
        # Instances.image_size): staged in pinned memory and uploaded without blocking.  The detection and ground-truth
        # values never leave the device: one concatenation and one row scatter per field for the whole batch
        ints = torch.empty(4 * B, dtype=torch.int32, pin_memory=pin)          # det counts | gt counts | clip (h, w) x B
        rows = torch.empty(N + M, dtype=torch.int64, pin_memory=pin)          # flat [B * cap] rows: detections | ground truth
        scale = torch.empty(B, 2, dtype=torch.float32, pin_memory=pin)
        ints_h, rows_h, scale_h = ints.numpy(), rows.numpy(), scale.numpy()
        ints_h[:B], ints_h[B:2 * B] = nds, ngs
        ints_h[2 * B:] = [int(v) for gi, _ in pairs for v in gi.image_size]
        rows_h[:N] = np.concatenate([i * cap + np.arange(n) for i, n in enumerate(nds)])
        rows_h[N:] = np.concatenate([i * cap + np.arange(n) for i, n in enumerate(ngs)])
        scale_h[:] = [(gi.image_size[1] / oi.image_size[1], gi.image_size[0] / oi.image_size[0])
                      for gi, oi in pairs]                                    # detector_postprocess(out, *input size)
        ints, rows, scale = (t.to(dev, non_blocking=True) for t in (ints, rows, scale))

        def scatter(parts, idx, dtype, *tail):
            out = torch.empty(B * cap, *tail, dtype=dtype, device=dev)
            if len(idx):
                out.index_copy_(0, idx, torch.cat([p.detach() for p in parts]).to(device=dev, dtype=dtype, non_blocking=True))
            return out.view(B, cap, *tail)
        db = scatter([oi.pred_boxes.tensor for _, oi in pairs], rows[:N], torch.float32, 4)
        ds = scatter([oi.scores for _, oi in pairs], rows[:N], torch.float32)
        dc = scatter([oi.pred_classes for _, oi in pairs], rows[:N], torch.int32)
        gb = scatter([gi.gt_boxes.tensor for gi, _ in pairs], rows[N:], torch.float32, 4)
        gc = scatter([gi.gt_classes for gi, _ in pairs], rows[N:], torch.int32)
        gt = BatchedGT(gb, gc, ints[B:2 * B], [tuple(gi.image_size) for gi, _ in pairs])
        self.process_batched(db, ds, dc, ints[:B], gt, scale, ints[2 * B:].view(B, 2))

    def process_batched(self, det_boxes, det_scores, det_classes, det_count, gt, scale, clip_size):
        """Container-level entry: detections as fixed-capacity arrays ([B,D,4] fp32, [B,D] fp32, [B,D] int32, [B] int32),
        ground truth as a ``BatchedGT``, ``scale`` [B,2] fp32 (sx, sy) and ``clip_size`` [B,2] int32 (h, w)."""
        if det_boxes.is_cuda:
            from . import native
            c = native.f1_count(det_boxes, det_scores, det_classes, det_count, gt.boxes, gt.classes, gt.count, scale,
                                clip_size, self.class_number, self.iou, self.top_n, self.score)
            c = c.sum(dim=0, dtype=torch.int64)
            self._dev = c if self._dev is None else self._dev + c
            return
        db, ds, dc = det_boxes.numpy(), det_scores.numpy(), det_classes.numpy()
        gb, gc = gt.boxes.numpy(), gt.classes.numpy()
        sc, cl = np.asarray(scale, dtype=np.float32), np.asarray(clip_size)
        nd = np.clip(np.asarray(det_count), 0, db.shape[1])
        ng = np.clip(np.asarray(gt.count), 0, gb.shape[1])
        for i in range(db.shape[0]):
            self._host += f1_image_counts(db[i, :nd[i]], ds[i, :nd[i]], dc[i, :nd[i]], gb[i, :ng[i]], gc[i, :ng[i]],
                                          sc[i, 0], sc[i, 1], int(cl[i, 0]), int(cl[i, 1]), self.class_number, self.iou,
                                          self.top_n, self.score)

    def accumulated(self):
        """This rank's [class_number, 3] int64 table so far (copies the device accumulator to the host)."""
        return self._host.copy() if self._dev is None else self._host + self._dev.cpu().numpy()

    def evaluate(self):
        dist = torch.distributed
        if self._distributed and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            on_dev = self._dev is not None and "nccl" in str(dist.get_backend())
            t = torch.from_numpy(self._host.copy())
            t = self._dev + t.to(self._dev.device) if on_dev else (t if self._dev is None else t + self._dev.cpu())
            dist.all_reduce(t)
            self.counts = t.cpu().numpy()
            if dist.get_rank() != 0:
                return {}
        else:
            self.counts = self.accumulated()
        tp, fp, fn = (int(v) for v in self.counts.sum(axis=0))
        precision = 0 if tp + fp == 0 else tp / (tp + fp)
        recall = 0 if tp + fn == 0 else tp / (tp + fn)
        if precision + recall == 0:
            return {"F1 Score": 0}
        return {"F1 Score": 2 * (precision * recall) / (precision + recall)}


class DatasetEvaluators:
    """d2 ``DatasetEvaluators``: ``reset`` / ``process`` go to every evaluator; ``evaluate`` merges their dicts on the main
    process (a key two evaluators both return is an error) and is an empty ``OrderedDict`` elsewhere."""

    def __init__(self, evaluators):
        self._evaluators = list(evaluators)

    def reset(self):
        for e in self._evaluators:
            e.reset()

    def process(self, inputs, outputs):
        for e in self._evaluators:
            e.process(inputs, outputs)

    def evaluate(self):
        dist = torch.distributed
        main = not (dist.is_available() and dist.is_initialized()) or dist.get_rank() == 0
        results = OrderedDict()
        for e in self._evaluators:
            result = e.evaluate()
            if main and result is not None:
                for k, v in result.items():
                    if k in results:
                        raise ValueError("Different evaluators produce results with the same key {}".format(k))
                    results[k] = v
        return results


def inference_on_dataset(model, data_loader, evaluator):
    """d2 ``inference_on_dataset``: eval mode + no_grad, ``evaluator.process`` per batch, ``evaluate`` at the
    end; the model's previous training mode is restored."""
    evaluator.reset()
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for inputs in data_loader:
                outputs = model(inputs)
                evaluator.process(inputs, outputs)
    finally:
        model.train(was_training)
    results = evaluator.evaluate()
    return {} if results is None else results


def print_csv_format(results):
    """d2 ``print_csv_format``: one ``copypaste:`` block per task, first the metric names, then the values."""
    lines = []
    for task, res in results.items():
        if isinstance(res, dict):
            important = [(k, v) for k, v in res.items() if "-" not in k]
            lines.append("copypaste: Task: {}".format(task))
            lines.append("copypaste: " + ",".join(k for k, _ in important))
            lines.append("copypaste: " + ",".join("{0:.4f}".format(v) for _, v in important))
        else:
            lines.append("copypaste: {}={}".format(task, res))
    for ln in lines:
        logger.info(ln)
    return lines
