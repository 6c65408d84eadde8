"""Time the mosaic composition and the step it feeds.  python tools/bench_mosaic.py [--no-step]   (needs the GPU; one JSON line)

Kernel: microseconds per ``sfod_mosaic_u8`` launch for four 3x600x1200 tiles -> 3x1024x2048 (the Cityscapes mosaic) and for
four tiles already at canvas scale (3x1024x2048 each, the base_mosaic_wq_new route), next to the same composition built from
what the project had before -- four ``native.resize_bilinear_u8`` launches, a torch canvas fill, four slice copies and a torch
2x2 mean -- and next to the four resize launches ALONE.  Device events around windows of launches that are enqueued behind
~0.1 s of other device work (so the device, not Python's launch rate, is timed), after a warm-up; the median
of the windows is reported with their spread, the variants alternate inside one process.  The fused result is compared with the
composition's (``torch.equal``) at the timed size before anything is timed.  ``floor_us`` is the bytes the composition must
move (tiles read once, output written once) over the measured copy rate of the chip (6.29 TB/s, float4 copy).

Step: milliseconds per training step of configs/faster_rcnn_VGG_cityscapes_foggy_source_mosaic.yaml at batch 4 in bf16x3
(600x1200 mapped frames -> 1024x2048 mosaics), next to TRAINER base on 1024x2048 frames with MIN_SIZE_TRAIN 0 -- the same
network tensors without the composition -- alternating windows, host clock around work that ends in a synchronise.  The
difference is what the loader fails to hide behind the step.  Reported, not gated."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_RATE = 6.29e12       # bytes / s, measured float4 copy


_blocker = []


def blocker():
    """~0.1 s of device work ahead of a timed window: the host enqueues the whole window while it runs, so the window measures
    the device (kernels and the boundaries between them), not Python's launch rate"""
    if not _blocker:
        _blocker.append(torch.randn(8192, 8192, device="cuda"))
    m = _blocker[0]
    for _ in range(8):
        torch.mm(m, m)


def windows(fn, launches, n_windows):
    out = []
    for _ in range(n_windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        blocker()
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / launches)
    return out


def summary(us):
    return {"us": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}


def kernel_part(native, launches, n_windows):
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    H, W = 1024, 2048
    small = [torch.randint(0, 256, (3, 600, 1200), generator=g, dtype=torch.uint8).to(dev) for _ in range(4)]
    up_hw = [(H, W)] * 4
    rects = [((0, 0, W, H), (0, 0, W, H)), ((W, 0, 2 * W, H), (0, 0, W, H)), ((0, H, W, 2 * H), (0, 0, W, H)),
             ((W, H, 2 * W, 2 * H), (0, 0, W, H))]
    big = [native.resize_bilinear_u8(t, H, W) for t in small]
    out = torch.empty(3, H, W, dtype=torch.uint8, device=dev)
    canvas = torch.empty(3, 2 * H, 2 * W, dtype=torch.uint8, device=dev)

    def paste_and_halve(ups):
        canvas.fill_(114)
        for u, ((lx1, ly1, lx2, ly2), _) in zip(ups, rects):
            canvas[:, ly1:ly2, lx1:lx2] = u
        c = canvas.to(torch.int16)
        return ((c[:, 0::2, 0::2] + c[:, 0::2, 1::2] + c[:, 1::2, 0::2] + c[:, 1::2, 1::2] + 2) >> 2).to(torch.uint8)

    variants = {
        "fused": lambda: native.mosaic_u8(small, up_hw, rects, (H, W), out=out),
        "resizes_alone": lambda: [native.resize_bilinear_u8(t, H, W) for t in small],
        "composed": lambda: paste_and_halve([native.resize_bilinear_u8(t, H, W) for t in small]),
        "fused_canvas_scale": lambda: native.mosaic_u8(big, up_hw, rects, (H, W), out=out),
        "composed_canvas_scale": lambda: paste_and_halve(big),
    }
    want = paste_and_halve(big)
    assert torch.equal(native.mosaic_u8(small, up_hw, rects, (H, W)), want), "fused != composed at the timed size"
    assert torch.equal(native.mosaic_u8(big, up_hw, rects, (H, W)), want), "fused (canvas scale) != composed at the timed size"
    for fn in variants.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(n_windows):                      # alternate: one window of each per round
        for k, fn in variants.items():
            times[k] += windows(fn, launches, 1)
    res = {k: summary(v) for k, v in times.items()}
    res["floor_us"] = round((4 * 3 * 600 * 1200 + 3 * H * W) / COPY_RATE * 1e6, 2)
    res["floor_canvas_scale_us"] = round((4 * 3 * H * W + 3 * H * W) / COPY_RATE * 1e6, 2)
    res["bytes_moved_MB"] = round((4 * 3 * 600 * 1200 + 3 * H * W) / 1e6, 2)
    res["fused_below_resizes_alone"] = res["fused"]["us"] < res["resizes_alone"]["us"]
    res["launches_per_window"], res["windows"] = launches, n_windows
    return res


def step_part(sfod, steps, warmup, n_windows):
    common = ["OUTPUT_DIR", "", "SFOD.COMPUTE_DTYPE", "bf16x3", "SOLVER.IMS_PER_BATCH", "4", "SFOD.SYNTHETIC.NUM_IMAGES", "16",
              "SOLVER.CHECKPOINT_PERIOD", "0", "TEST.EVAL_PERIOD", "0", "SFOD.EVAL_HOOK", "False", "SOLVER.MAX_ITER", "100000"]
    cfgs = {
        "mosaic": sfod.config.setup_cfg(os.path.join(ROOT, "configs", "faster_rcnn_VGG_cityscapes_foggy_source_mosaic.yaml"), common),
        "base_1024x2048": sfod.config.setup_cfg(os.path.join(ROOT, "configs", "faster_rcnn_VGG_cityscapes_foggy_source_mosaic.yaml"),
                                                common + ["TRAINER", "base", "INPUT.MIN_SIZE_TRAIN", "(0,)"]),
    }
    trainers = {}
    for k, cfg in cfgs.items():
        torch.manual_seed(cfg.SEED)
        trainers[k] = sfod.engine.get_trainer_class(cfg)(cfg)

    def run(tr, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            tr.run_step()
            tr.scheduler.step()
            tr.iter += 1
        torch.cuda.synchronize()
        tr.storage.flush()
        return (time.perf_counter() - t0) * 1e3 / n
    for tr in trainers.values():
        run(tr, warmup)
    times = {k: [] for k in trainers}
    for _ in range(n_windows):
        for k, tr in trainers.items():
            times[k].append(run(tr, steps))
    res = {k: {"ms_per_step": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in times.items()}
    res["loader_not_hidden_ms"] = round(res["mosaic"]["ms_per_step"] - res["base_1024x2048"]["ms_per_step"], 2)
    res["batch"], res["steps_per_window"], res["windows"], res["dtype"] = 4, steps, n_windows, "bf16x3"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mosaic.py measures on the GPU; there is none here")
    sfod = importlib.import_module("simple-sfod_amd")
    sfod.native.load()
    res = {"metric": "sfod_mosaic_u8, four 3x600x1200 tiles -> 3x1024x2048", "device": torch.cuda.get_device_name(0),
           "kernel": kernel_part(sfod.native, args.launches, args.windows)}
    if not args.no_step:
        res["step"] = step_part(sfod, args.steps, args.warmup, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
