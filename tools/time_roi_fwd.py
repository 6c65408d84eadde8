"""Time sfod_roi_align_fwd on the hot yaml's shapes (8 x 37 x 75 x 512): the student's 512 and the teacher's 2000 ROIs per
image.  --pooled / --sampling-ratio / --aligned: the pooler options; --dtype: the feature map's (the hot yaml runs bf16x3)."""
import argparse
import importlib
import sys
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
nat = importlib.import_module("simple-sfod_amd.native")
from time_roi_bwd import make_rois  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pooled", type=int, default=7)
    ap.add_argument("--sampling-ratio", type=int, default=0)
    ap.add_argument("--aligned", type=int, default=1)
    ap.add_argument("--dtype", choices=["bf16", "fp32", "bf16x3"], default="bf16x3")
    ap.add_argument("--iters", type=int, default=20, help="launches per timed window")
    ap.add_argument("--repeats", type=int, default=1, help="timed windows per shape (each printed: the spread)")
    a = ap.parse_args()
    P = a.pooled
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    B, H, W, C, size = 8, 37, 75, 512, 160.0
    feat = torch.randn(B, H, W, C, generator=g).to(dev)
    feat = feat.to(torch.bfloat16) if a.dtype == "bf16" else (nat.cast(feat, nat.SPLIT_DTYPE) if a.dtype == "bf16x3" else feat)
    kw = dict(sampling_ratio=a.sampling_ratio, aligned=bool(a.aligned))
    for who, per in (("student", 512), ("teacher", 2000)):
        rois = make_rois(B, H, W, per, size, g, dev)
        for _ in range(3):
            out = nat.roi_align_fwd(feat, rois, P, 1 / 16, **kw)
        torch.cuda.synchronize()
        us = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                out = nat.roi_align_fwd(feat, rois, P, 1 / 16, **kw)
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1000 / a.iters)
        del out
        print("fwd %s P%d sr%d aligned%d %s B%d %dx%dx%d R%d size~%g: %s us (%d launches per window)" % (
            who, P, a.sampling_ratio, a.aligned, a.dtype, B, H, W, C, B * per, size, " ".join("%.1f" % u for u in us), a.iters), flush=True)


if __name__ == "__main__":
    main()
