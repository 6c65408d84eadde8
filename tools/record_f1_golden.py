"""Records tests/golden/f1_ref.npz: the reference's ``F1Evaluator`` (daod/evaluation/f1_evaluator.py, loaded by file
path behind oracle/ref_stub/hook.py) run on the hand cases of tests/helpers/f1_cases.py and on seeded random images, for
the three parameter sets (iou, top_n, score) = (0.5, 5, 0.5), (0.3, 100, 0.05), (0.75, 1, 0.9).

Usage: python tools/record_f1_golden.py <reference checkout> [out.npz]        (CPU only; no test reads the reference)

The stub's ``detector_postprocess`` raises by design, so ``_predictions`` is filled directly with boxes that are already
at the loader's scale, inside the image and non-empty: step 1 of the rule is pinned by tests against this project's own
``detector_postprocess``, steps 2 to 8 against this file.  The stub ``Boxes`` does not iterate row by row as d2's does;
``Rows`` below is the container the evaluator iterates.

Stored: per image K, nd, ng, sizes (h, w) and the concatenated det_boxes / det_scores / det_classes / gt_boxes /
gt_classes; params [3, 3]; counts [3, N, 8, 3] = (TP, FP, FN) of ``evaluate_output`` with class_number = K of the image
(rows >= K are 0); f1 [3] = ``evaluate()["F1 Score"]`` of one evaluator with class_number = 8 over all images.
Kept scores are distinct per image; every value is finite."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PARAMS = [(0.5, 5, 0.5), (0.3, 100, 0.05), (0.75, 1, 0.9)]
N_RANDOM = 200


class Rows:
    def __init__(self, t):
        self.tensor = t

    def __iter__(self):
        return iter(self.tensor)


def random_image(rng, full=False):
    K = int(rng.integers(1, 9))
    nd, ng = (100, 100) if full else (int(rng.integers(0, 101)), int(rng.integers(0, 101)))
    integer = rng.random() < 0.35                       # whole-pixel boxes on a small canvas: equal IoUs do occur
    h, w = (int(rng.integers(40, 90)), int(rng.integers(40, 90))) if integer else (int(rng.integers(200, 700)), int(rng.integers(200, 700)))

    def boxes(n, lo, hi):
        x1, y1 = rng.uniform(0, w - lo - 1, n), rng.uniform(0, h - lo - 1, n)
        return np.stack([x1, y1, x1 + rng.uniform(lo, hi, n), y1 + rng.uniform(lo, hi, n)], 1)
    gb = boxes(ng, 4, min(h, w) / 2)
    gc = np.where(rng.random(ng) < 0.95, rng.integers(0, K, ng), K)
    db = boxes(nd, 4, min(h, w) / 2)
    dc = np.where(rng.random(nd) < 0.95, rng.integers(0, K, nd), K)
    if ng:                                              # a share of the detections: jittered copies of ground-truth boxes
        for i in np.nonzero(rng.random(nd) < 0.6)[0]:
            g = int(rng.integers(0, ng))
            size = np.array([gb[g, 2] - gb[g, 0], gb[g, 3] - gb[g, 1]] * 2)
            db[i] = gb[g] + rng.normal(0, rng.choice([0.02, 0.08, 0.2]), 4) * size
            dc[i] = gc[g] if rng.random() < 0.85 else rng.integers(0, K)
    if integer:
        gb, db = np.round(gb), np.round(db)
    for b in (gb, db):                                  # inside the image, at least one pixel wide and high
        b[:, 0::2] = np.clip(b[:, 0::2], 0, w)
        b[:, 1::2] = np.clip(b[:, 1::2], 0, h)
        b[:, 0] = np.minimum(b[:, 0], w - 1)
        b[:, 1] = np.minimum(b[:, 1], h - 1)
        b[:, 2] = np.maximum(b[:, 2], b[:, 0] + 1)
        b[:, 3] = np.maximum(b[:, 3], b[:, 1] + 1)
    ds = rng.choice(np.arange(500, 10000) if full else np.arange(1, 10000), nd, replace=False) / 10000.0
    return K, db.astype(np.float32), ds.astype(np.float32), dc.astype(np.int32), gb.astype(np.float32), gc.astype(np.int32), (h, w)


def main():
    ref = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "f1_ref.npz")
    from oracle.ref_stub import hook
    hook.install()
    spec = importlib.util.spec_from_file_location("ref_f1_evaluator", os.path.join(ref, "daod", "evaluation", "f1_evaluator.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from helpers import f1_cases

    images = []
    for case in f1_cases.HAND_CASES:
        for dets, gts, size in case["images"]:
            images.append((case["K"], np.array([d[0] for d in dets], np.float32).reshape(-1, 4),
                           np.array([d[1] for d in dets], np.float32), np.array([d[2] for d in dets], np.int32),
                           np.array([g[0] for g in gts], np.float32).reshape(-1, 4), np.array([g[1] for g in gts], np.int32), size))
    rng = np.random.default_rng(20240607)
    images += [random_image(rng, full=i < 2) for i in range(N_RANDOM)]
    for _, db, ds, _, gb, _, (h, w) in images:
        assert np.isfinite(db).all() and np.isfinite(gb).all() and len(set(ds.tolist())) == len(ds)
        for b in (db, gb):
            assert (b[:, 2] - b[:, 0] > 0).all() and (b[:, 3] - b[:, 1] > 0).all() and (b >= 0).all()
            assert (b[:, 0::2] <= w).all() and (b[:, 1::2] <= h).all()

    def prediction(i, img):
        _, db, ds, dc, gb, gc, _ = img
        inst = types.SimpleNamespace(scores=torch.from_numpy(ds), pred_boxes=Rows(torch.from_numpy(db)),
                                     pred_classes=torch.from_numpy(dc).long())
        gt = types.SimpleNamespace(gt_boxes=Rows(torch.from_numpy(gb)), gt_classes=torch.from_numpy(gc).long())
        return {"image_id": i, "input_instances": gt, "instances": inst}

    counts = np.zeros((len(PARAMS), len(images), 8, 3), np.int32)
    f1 = np.zeros(len(PARAMS), np.float64)
    for p, (iou, top_n, score) in enumerate(PARAMS):
        whole = mod.F1Evaluator(8, iou=iou, top_n=top_n, score=score)
        for i, img in enumerate(images):
            res = mod.F1Evaluator(img[0], iou=iou, top_n=top_n, score=score).evaluate_output(prediction(i, img))
            for k, r in enumerate(res):
                counts[p, i, k] = r["true_positive"], r["false_positive"], r["false_negative"]
            whole._predictions.append(prediction(i, img))
        f1[p] = whole.evaluate()["F1 Score"]
    np.savez_compressed(
        out, params=np.array(PARAMS, np.float64), K=np.array([im[0] for im in images], np.int32),
        nd=np.array([len(im[2]) for im in images], np.int32), ng=np.array([len(im[5]) for im in images], np.int32),
        sizes=np.array([im[6] for im in images], np.int32), det_boxes=np.concatenate([im[1] for im in images]),
        det_scores=np.concatenate([im[2] for im in images]), det_classes=np.concatenate([im[3] for im in images]),
        gt_boxes=np.concatenate([im[4] for im in images]), gt_classes=np.concatenate([im[5] for im in images]),
        counts=counts, f1=f1)
    print(out, os.path.getsize(out), "bytes;", len(images), "images; TP/FP/FN per parameter set:",
          counts.sum(axis=(1, 2)).tolist(), "F1:", f1.tolist())


if __name__ == "__main__":
    main()
