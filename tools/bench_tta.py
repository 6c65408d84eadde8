"""``sfod_tta_merge`` per launch (TEST.AUG's box merge) at B images x A augmentations x cap detections, next to the same step
-- inverse transforms, concatenation, finite / clip / score filter -> candidates -- composed from torch ops on the device and
done on the host as Detectron2 does it (``.cpu()`` + numpy + upload), and next to the launch-latency floor (the same kernel
on one slot; a one-element torch op).  Device events around ``--iters`` repetitions after a warm-up.  One JSON line."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def inputs(sfod, B, A, cap, dev, seed=0):
    cfg = sfod.config.setup_cfg(None, [])
    cfg.defrost()
    cfg.TEST.AUG.MIN_SIZES = tuple(cfg.TEST.AUG.MIN_SIZES)[: max(A // 2, 1)]
    cfg.TEST.AUG.FLIP = A > 1
    cfg.TEST.DETECTIONS_PER_IMAGE = cap
    opt = sfod.modeling.tta_options.TTAOptions(cfg)
    plan = opt.plan(600, 1200, 1024, 2048)
    assert opt.num_aug == A, (opt.num_aug, A)
    g = torch.Generator().manual_seed(seed)
    hw = torch.tensor([(r[1], r[0]) for r in plan.table], dtype=torch.float32)     # [A, 2] (h_a, w_a)
    xy = torch.rand(B, A, cap, 2, generator=g) * hw.flip(1)[None, :, None, :] * 0.8
    wh = torch.rand(B, A, cap, 2, generator=g) * hw.flip(1)[None, :, None, :] * 0.3 + 1
    boxes = torch.cat([xy, xy + wh], -1)
    scores = torch.rand(B, A, cap, generator=g).sort(dim=-1, descending=True).values
    classes = torch.randint(0, 8, (B, A, cap), generator=g, dtype=torch.int32)
    count = torch.randint(cap // 2, cap + 1, (B, A), generator=g, dtype=torch.int32)
    table = torch.tensor([plan.table] * B, dtype=torch.float32)
    sizes = torch.tensor([plan.native_hw] * B, dtype=torch.int32)
    return [t.to(dev) for t in (boxes, scores, classes, count, table, sizes)]


def torch_composed(boxes, scores, classes, count, table, sizes, thr):
    """the step in torch ops, per image and augmentation as a port of d2's loop would do it (no host read)"""
    B, A, cap = scores.shape
    ob, os_, oc = [], [], []
    slot = torch.arange(cap, device=boxes.device)
    for b in range(B):
        H0, W0 = sizes[b, 0].float(), sizes[b, 1].float()
        for a in range(A):
            t = table[b, a]
            bx = boxes[b, a]
            x = torch.where(t[2] != 0, t[0] - bx[:, 0::2], bx[:, 0::2])
            x = torch.stack([x.min(1).values, x.max(1).values], 1) * t[3] * t[5]
            y = bx[:, 1::2] * t[4] * t[6]
            out = torch.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], 1)
            ok = torch.isfinite(out).all(1) & torch.isfinite(scores[b, a]) & (slot < count[b, a]) & (scores[b, a] > thr)
            out = torch.stack([torch.minimum(out[:, 0].clamp(min=0), W0),
                               torch.minimum(out[:, 1].clamp(min=0), H0), torch.minimum(out[:, 2].clamp(min=0), W0),
                               torch.minimum(out[:, 3].clamp(min=0), H0)], 1)
            ob.append(torch.where(ok[:, None], out, torch.zeros_like(out)))
            os_.append(torch.where(ok, scores[b, a], torch.full_like(scores[b, a], -1.0)))
            oc.append(torch.where(ok, classes[b, a], torch.zeros_like(classes[b, a])))
    n = A * cap
    return torch.cat(ob).view(B, n, 4), torch.cat(os_).view(B, n), torch.cat(oc).view(B, n)


def host_route(boxes, scores, classes, count, table, sizes, thr):
    """d2's: every pass's boxes to the host, numpy apply_box, concatenated tensors back on the device"""
    B, A, cap = scores.shape
    tab, cnt = table.cpu().numpy(), count.cpu().numpy()
    out = []
    for b in range(B):
        bs, ss, cs = [], [], []
        for a in range(A):
            n = int(cnt[b, a])
            bx = boxes[b, a, :n].cpu().numpy()
            t = tab[b, a]
            x = bx[:, 0::2]
            if t[2]:
                x = t[0] - x
            x = np.sort(x, 1) * t[3] * t[5]
            y = bx[:, 1::2] * t[4] * t[6]
            bs.append(torch.from_numpy(np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], 1)).to(boxes.device))
            ss.append(scores[b, a, :n])
            cs.append(classes[b, a, :n])
        out.append((torch.cat(bs), torch.cat(ss), torch.cat(cs)))
    return out


def timed(fn, iters, warmup=5):
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
    ap.add_argument("--augs", type=int, default=18)
    ap.add_argument("--cap", type=int, default=100)
    ap.add_argument("--iters", type=int, default=2000)
    args = ap.parse_args()
    sfod = importlib.import_module("simple-sfod_amd")
    native = sfod.native
    dev = torch.device("cuda:0")
    x = inputs(sfod, args.images, args.augs, args.cap, dev)
    one = inputs(sfod, 1, 1, 1, dev)
    tiny = torch.zeros(1, device=dev)
    thr = 1e-8
    cb, cs, ck, cc = native.tta_merge_candidates(*x, 8, thr)
    tb, ts, tk = torch_composed(*x, thr)
    live = cs >= 0
    agree = bool(torch.equal(cs, ts) and torch.equal(ck, tk) and (cb[live] - tb[live]).abs().max().item() < 1e-2)
    res = {
        "shape": {"images": args.images, "augmentations": args.augs, "cap": args.cap, "candidates_kept": int(cc.sum())},
        "sfod_tta_merge": timed(lambda: native.tta_merge_candidates(*x, 8, thr), args.iters),
        "launch_floor_same_kernel_one_slot": timed(lambda: native.tta_merge_candidates(*one, 8, thr), args.iters),
        "launch_floor_one_element_torch_op": timed(lambda: tiny.add_(1.0), args.iters),
        "torch_ops_on_device": timed(lambda: torch_composed(*x, thr), max(args.iters // 100, 5), warmup=2),
        "host_route_cpu_numpy": timed(lambda: host_route(*x, thr), max(args.iters // 100, 5), warmup=2),
        "whole_merge_chain": timed(lambda: native.tta_merge(*x, 8, thr, 0.5, args.cap), max(args.iters // 10, 5)),
        "torch_composition_agrees": agree,
        "bytes_read_plus_written": int(sum(t.numel() * t.element_size() for t in x) + sum(t.numel() * t.element_size() for t in (cb, cs, ck, cc))),
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
