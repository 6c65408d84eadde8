"""``sfod_coco_match`` per launch (COCOeval's matching of ``SFOD.COCO_EVAL_DEVICE``) at B images x D detections x G ground
truths, next to the launch floor measured the way tools/bench_tta.py measures it: the same call on one slot, and a one-element
torch op; also with every box in one category (the longest rows the kernel meets at that size).  One JSON line."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def inputs(B, D, G, K, dev, seed=0):
    """D detections = jittered copies of G ground truths (most of them match at the low thresholds), capacity arrays D x G"""
    rng = np.random.RandomState(seed)
    xy = rng.randint(0, 1500, size=(B, G, 2)).astype(np.float64)
    wh = rng.randint(16, 300, size=(B, G, 2)).astype(np.float64)
    gcls = rng.randint(0, K, size=(B, G)).astype(np.int32)
    pick = rng.randint(0, G, size=(B, D))
    b = np.arange(B)[:, None]
    jit = rng.randint(-8, 9, size=(B, D, 4)) / 2.0
    db = np.concatenate([xy[b, pick], xy[b, pick] + wh[b, pick]], axis=2) + jit
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    return (t(db, torch.float32), t(rng.rand(B, D), torch.float32), t(gcls[b, pick], torch.int32),
            torch.full((B,), D, dtype=torch.int32, device=dev), t(np.concatenate([xy, wh], axis=2), torch.float64),
            t(wh[..., 0] * wh[..., 1], torch.float64), t(gcls, torch.int32), t(rng.rand(B, G) < 0.1, torch.int32),
            torch.full((B,), G, dtype=torch.int32, device=dev))


def timed(fn, iters, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return {"device_us": round(e0.elapsed_time(e1) * 1000 / iters, 2), "wall_us": round((time.perf_counter() - t0) * 1e6 / iters, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--gts", type=int, default=100)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--iters", type=int, default=1000)
    args = ap.parse_args()
    sfod = importlib.import_module("simple-sfod_amd")
    native, E = sfod.native, sfod.evaluation
    dev = torch.device("cuda:0")
    x = inputs(args.images, args.dets, args.gts, args.classes, dev)
    x1 = inputs(args.images, args.dets, args.gts, 1, dev)
    one = inputs(1, 1, 1, 1, dev)
    tiny = torch.zeros(1, device=dev)
    run = lambda a, K: native.coco_match(*a, K, E.IOU_THRS, E.AREA_RNG)
    _, match, _, _ = run(x, args.classes)
    res = {
        "shape": {"images": args.images, "detections": args.dets, "ground_truths": args.gts, "classes": args.classes,
                  "matched_at_0.5": int((match & 1).sum())},
        "sfod_coco_match": timed(lambda: run(x, args.classes), args.iters),
        "sfod_coco_match_single_class": timed(lambda: run(x1, 1), args.iters),
        "launch_floor_same_kernel_one_slot": timed(lambda: run(one, 1), args.iters),
        "launch_floor_one_element_torch_op": timed(lambda: tiny.add_(1.0), args.iters),
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
