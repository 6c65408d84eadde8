"""Per-launch times of the Fast R-CNN loss entry point and of the candidates kernel at the hot shapes, per classification mode
(reported, not gated):

  * loss + gradient, R = 4096 rows, K = 8 (bench.py's batch 8 x 512 sampled ROIs): ``sfod_frcnn_loss`` (cross-entropy) and,
    where the library has it, ``sfod_frcnn_loss_cls`` with cross-entropy, focal (gamma 1.5) and sigmoid cross-entropy;
  * candidates, B = 8, P = 1000, K = 8 (the teacher's post-processing): ``sfod_frcnn_candidates`` and ``sfod_frcnn_candidates_cls``
    with softmax and sigmoid probabilities.

A call is a memset, the kernel and (the loss) the partial sum; the figure is device-event time over ``inner`` calls enqueued
back to back, so it is bounded below by the host's enqueue rate -- the kernels' own times come from a kernel trace of this
script.  Copied into ``tools/`` of another checkout it times that checkout's library (one without the ``*_cls`` entry points
reports the existing ones only); three alternating rounds per entry.
    python tools/bench_cls_loss.py [--runs 20] [--inner 200]
"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sfod = importlib.import_module("simple-sfod_amd")
native = sfod.native
DEV = "cuda"
R, K, B, P = 4096, 8, 8, 1000
ROI_W = (10.0, 10.0, 5.0, 5.0)


def timed(fn, runs, inner, warmup=3):
    """-> (median, min) us per call of ``fn()``; ``inner`` calls enqueued back to back between one pair of events"""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / inner * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def loss_calls(lib):
    g = torch.Generator().manual_seed(1)
    ld = 48
    pred = torch.zeros(R, ld)
    pred[:, :K + 1] = torch.randn(R, K + 1, generator=g) * 3
    pred[:, K + 1:5 * K + 1] = torch.randn(R, 4 * K, generator=g) * 0.5
    xy = torch.rand(R, 2, generator=g) * 900
    src = torch.cat([xy, xy + torch.rand(R, 2, generator=g) * 250 + 16], 1)
    rois = torch.cat([torch.zeros(R, 1), src], 1).to(DEV)
    gtb = (src + torch.randn(R, 4, generator=g) * 6).to(DEV)
    cls = torch.randint(0, K + 1, (R,), generator=g)
    cls[torch.rand(R, generator=g) < 0.75] = K                     # three quarters background, like a sampled batch
    cls, pred = cls.int().to(DEV), pred.to(DEV)
    nv = torch.tensor([R], dtype=torch.int32, device=DEV)
    loss, gs = torch.empty(2, device=DEV), torch.tensor([1.0, 1.0], device=DEV)
    d_pred, ws = torch.empty_like(pred), torch.empty(((R + 255) // 256) * 3, device=DEV)      # three per block: the _cls form's modes 1 and 2
    head = (pred, ld, R, K, rois, cls, gtb, nv, loss, gs, d_pred, ws)
    calls = {"sfod_frcnn_loss (cross-entropy)": lambda: native.call("sfod_frcnn_loss", *head)}
    if hasattr(lib, "sfod_frcnn_loss_cls"):
        for label, mode in (("cross-entropy", 0), ("focal gamma 1.5", 1), ("sigmoid cross-entropy", 2)):
            calls[f"sfod_frcnn_loss_cls ({label})"] = (lambda mode=mode: native.call("sfod_frcnn_loss_cls", *head, *ROI_W, 0, 0.0, 0, mode, 1.5))
    return calls


def candidate_calls(lib):
    g = torch.Generator().manual_seed(2)
    ld = 48
    pred = torch.zeros(B * P, ld)
    pred[:, :K + 1] = torch.randn(B * P, K + 1, generator=g) * 3
    pred[:, K + 1:5 * K + 1] = torch.randn(B * P, 4 * K, generator=g) * 0.5
    xy = torch.rand(B, P, 2, generator=g) * torch.tensor([900.0, 400.0])
    props = torch.cat([xy, xy + torch.rand(B, P, 2, generator=g) * 250 + 2], 2).to(DEV)
    pc = torch.full((B,), P, dtype=torch.int32, device=DEV)
    sizes = torch.tensor([(600, 1200)] * B, dtype=torch.int32, device=DEV)
    cb, cs = torch.empty(B, P * K, 4, device=DEV), torch.empty(B, P * K, device=DEV)
    cc = torch.empty(B, dtype=torch.int32, device=DEV)
    head = (pred.to(DEV), ld, B, P, K, props, pc, sizes, 0.05, cb, cs, cc)
    calls = {"sfod_frcnn_candidates (softmax)": lambda: native.call("sfod_frcnn_candidates", *head)}
    if hasattr(lib, "sfod_frcnn_candidates_cls"):
        for label, mode in (("softmax", 0), ("sigmoid", 2)):
            calls[f"sfod_frcnn_candidates_cls ({label})"] = (lambda mode=mode: native.call("sfod_frcnn_candidates_cls", *head, *ROI_W, 0, mode, 1.5))
    return calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cls_loss.py measures on the GPU: no device found")
    lib = native.load()
    res = {"library": native.SO_PATH, "shape": {"loss": {"R": R, "K": K}, "candidates": {"B": B, "P": P, "K": K}}, "runs": a.runs,
           "inner": a.inner}
    for group, calls in (("loss_and_gradient", loss_calls(lib)), ("candidates", candidate_calls(lib))):
        rounds = {k: [] for k in calls}
        for _ in range(a.rounds):          # alternating
            for k, fn in calls.items():
                rounds[k].append(timed(fn, a.runs, a.inner))
        res[group] = {k: {"us_median_rounds": [round(t[0], 2) for t in v], "us_median": round(min(t[0] for t in v), 2),
                          "us_min": round(min(t[1] for t in v), 2)} for k, v in rounds.items()}
    for k, v in res.items():
        print(f"{k:20s} {v}", file=sys.stderr)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
