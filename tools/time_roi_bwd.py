"""Time sfod_roi_align_bwd on the student's shapes (SFOD_ROI_BWD_ATOMIC=1 selects the scatter form, pooled <= 8).
--pooled / --sampling-ratio / --aligned: the pooler options; --dtype: the upstream gradient (fp32 in the operand-pair modes);
--hot: only the hot yaml's shape (8 x 37 x 75 x 512, 512 ROIs per image)."""
import argparse
import importlib
import sys
import torch

sys.path.insert(0, ".")
nat = importlib.import_module("simple-sfod_amd.native")

SHAPES = [(8, 37, 75, 512, 512, 160.0), (8, 37, 75, 512, 512, 400.0), (8, 64, 128, 512, 512, 200.0), (8, 37, 75, 1024, 512, 160.0)]


def make_rois(B, H, W, per, size, g, dev):
    R = B * per
    cx = torch.rand(R, generator=g) * W * 16
    cy = torch.rand(R, generator=g) * H * 16
    w = size * (0.3 + 1.4 * torch.rand(R, generator=g))
    h = size * (0.3 + 1.4 * torch.rand(R, generator=g))
    return torch.stack([torch.arange(R).div(per, rounding_mode="floor").float(),
                        (cx - w / 2).clamp(0, W * 16), (cy - h / 2).clamp(0, H * 16),
                        (cx + w / 2).clamp(0, W * 16), (cy + h / 2).clamp(0, H * 16)], 1).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pooled", type=int, default=7)
    ap.add_argument("--sampling-ratio", type=int, default=0)
    ap.add_argument("--aligned", type=int, default=1)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--hot", action="store_true")
    ap.add_argument("--iters", type=int, default=20, help="launches per timed window")
    ap.add_argument("--repeats", type=int, default=1, help="timed windows per shape (each printed: the spread)")
    a = ap.parse_args()
    P = a.pooled
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    for (B, H, W, C, per, size) in (SHAPES[:1] if a.hot else SHAPES):
        R = B * per
        rois = make_rois(B, H, W, per, size, g, dev)
        dout = torch.randn(R, P * P, C, generator=g).to(dev)
        if a.dtype == "bf16":
            dout = dout.to(torch.bfloat16)
        df = torch.zeros(B, H, W, C, device=dev)
        kw = dict(sampling_ratio=a.sampling_ratio, aligned=bool(a.aligned))
        for _ in range(3):
            nat.roi_align_bwd(dout, rois, (B, H, W, C), P, 1 / 16, dfeat=df, **kw)
        torch.cuda.synchronize()
        us = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                nat.roi_align_bwd(dout, rois, (B, H, W, C), P, 1 / 16, dfeat=df, **kw)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1000 / a.iters)
        print("bwd P%d sr%d aligned%d %s B%d %dx%dx%d R%d size~%g: %s us (%d launches per window)" % (
            P, a.sampling_ratio, a.aligned, a.dtype, B, H, W, C, R, size, " ".join("%.1f" % u for u in us), a.iters), flush=True)


if __name__ == "__main__":
    main()
