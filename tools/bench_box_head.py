"""Times of the box-head architecture options at the hot shape (R = 4096 ROIs = 8 frames x 512, 7 x 7, CONV_DIM 256, bf16x3):
the GroupNorm + ReLU launches against the floor of one read and one write of the tensor, the 3x3 convolution's forward, data
gradient and weight gradient (with the kernels the plans pick), and a whole training pass of ``StandardROIHeads`` -- forward
and backward through the loss node -- with the 4conv1fc + GN head against the 2-FC head.  Reported, not gated.
    python tools/bench_box_head.py [--runs 30] [--rois 4096]
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
HBM = 6.29e12          # bytes / s: the measured float4-copy rate of an MI355X (8.0 TB/s on the data sheet)
DEV = "cuda"
YAML = os.path.join(ROOT, "configs", "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free.yaml")


def timed(fn, runs, inner=1, warmup=5):
    """-> (median, min) ms per launch of ``fn()``: ``runs`` samples, each ``inner`` launches enqueued back to back between one
    pair of events (so that a launch of a few tens of microseconds is timed on a busy queue, not behind the host's enqueue)"""
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
        ts.append(a.elapsed_time(b) / inner)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def group_norm(R, P, C, runs):
    g = torch.Generator(device=DEV).manual_seed(1)
    y = torch.randn(R, P, P, C, device=DEV, generator=g) + 0.3
    dz = torch.randn(R, P, P, C, device=DEV, generator=g)
    gamma, beta = torch.randn(C, device=DEV, generator=g), torch.randn(C, device=DEV, generator=g)
    _, _, mean, rstd = native.group_norm_relu_fwd(y, gamma, beta, out_dtype=native.SPLIT_DTYPE)
    n = y.numel()
    out = {}
    for name, fn, nbytes in (
            ("fwd", lambda: native.group_norm_relu_fwd(y, gamma, beta, out_dtype=native.SPLIT_DTYPE), 8 * n),
            ("bwd", lambda: native.group_norm_relu_bwd(dz, y, mean, rstd, gamma, beta, out_dtype=native.SPLIT_DTYPE), 12 * n)):
        med, mn = timed(fn, runs, inner=20)
        floor = nbytes / HBM * 1e3
        out["group_norm_" + name] = {"ms_median": round(med, 4), "ms_min": round(mn, 4), "floor_ms": round(floor, 4),
                                     "median_over_floor": round(med / floor, 2), "bytes": nbytes}
    return out


def conv_layer(R, P, C, runs):
    g = torch.Generator(device=DEV).manual_seed(2)
    dt = native.BF16X3
    x = native.cast(torch.randn(R, P, P, C, device=DEV, generator=g), native.SPLIT_DTYPE)
    dy = native.cast(torch.randn(R, P, P, C, device=DEV, generator=g) * 1e-3, native.SPLIT_DTYPE)
    w = torch.randn(C, C, 3, 3, device=DEV, generator=g) * 0.03
    wp, wr = native.pack_conv_weight(w, C, dt), native.pack_conv_weight(w, C, dt, rot180=True)
    flops = 2.0 * R * P * P * C * C * 9
    out = {"conv_fwd_algo": native.query("sfod_conv_fwd_algo", R, P, P, C, C, 3, dt)}
    for name, fn in (("fwd", lambda: native.conv_fwd(x, wp, None, C, 3)), ("dgrad", lambda: native.conv_fwd(dy, wr, None, C, 3)),
                     ("wgrad", lambda: native.conv_weight_grad(x, dy, w))):
        med, mn = timed(fn, runs, inner=5)
        out["conv3x3_" + name] = {"ms_median": round(med, 4), "ms_min": round(mn, 4), "tflops_median": round(flops / med / 1e9, 1),
                                  "kernel": native.last_conv_kernel()}
    return out


def heads_pass(opts, R, runs):
    """one training pass (label and sample outside the timed region): forward through the loss node and backward"""
    B, per = 8, R // 8
    cfg = sfod.config.setup_cfg(YAML, ["OUTPUT_DIR", "", "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", str(per)] + opts)
    torch.manual_seed(3)
    rh = importlib.import_module("simple-sfod_amd.modeling.roi_heads")
    heads = rh.StandardROIHeads(cfg, {"vgg4": sfod.structures.ShapeSpec(channels=512, stride=16)}).to(DEV).train()
    g = torch.Generator().manual_seed(4)
    Hf, Wf = 37, 75
    feat = torch.randn(B, 512, Hf, Wf, generator=g).to(DEV).requires_grad_(True)
    P = 2 * per
    xy = torch.rand(B, P, 2, generator=g) * torch.tensor([Wf * 16 * 0.7, Hf * 16 * 0.7])
    wh = torch.rand(B, P, 2, generator=g) * torch.tensor([Wf * 16 * 0.3, Hf * 16 * 0.3]) + 8
    boxes = torch.cat([xy, xy + wh], 2)
    S = sfod.structures
    targets = []
    for b in range(B):
        inst = S.Instances((Hf * 16, Wf * 16))
        inst.gt_boxes = S.Boxes(boxes[b, :12].clone())
        inst.gt_classes = torch.randint(0, heads.num_classes, (12,), generator=g)
        targets.append(inst)
    props = sfod.modeling.batched.BatchedProposals(boxes.to(DEV), torch.zeros(B, P, device=DEV),
                                                   torch.full((B,), P, dtype=torch.int32, device=DEV), [(Hf * 16, Wf * 16)] * B)
    gt = sfod.modeling.batched.BatchedGT.from_instances(targets, feat.device)
    samples = heads.label_and_sample_proposals(props, gt)
    params = heads._params()

    def step():
        feat.grad = None
        for p in params:
            p.grad = None
        l_cls, l_box = rh._ROILossFn.apply(heads, feat, samples, *params)
        (l_cls + l_box).backward()
    med, mn = timed(step, runs, warmup=3)
    return {"ms_median": round(med, 3), "ms_min": round(mn, 3), "rois": int(samples["rois"].shape[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--rois", type=int, default=4096)
    a = ap.parse_args()
    native.load()
    if not torch.cuda.is_available():
        raise SystemExit("bench_box_head.py measures on the GPU: no device found")
    H = "MODEL.ROI_BOX_HEAD."
    res = {"shape": {"R": a.rois, "P": 7, "C": 256, "mode": "bf16x3"}, "runs": a.runs,
           "launches_per_sample": {"group_norm": 20, "conv3x3": 5, "head": 1}, "hbm_bytes_per_s": HBM}
    res.update(group_norm(a.rois, 7, 256, a.runs))
    res.update(conv_layer(a.rois, 7, 256, a.runs))
    res["head_4conv1fc_gn"] = heads_pass([H + "NUM_CONV", "4", H + "CONV_DIM", "256", H + "NUM_FC", "1", H + "NORM", "GN"], a.rois,
                                         max(a.runs // 3, 5))
    res["head_2fc"] = heads_pass([], a.rois, max(a.runs // 3, 5))
    for k, v in res.items():
        print(f"{k:20s} {v}", file=sys.stderr)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
