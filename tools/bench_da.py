"""Times of the DA Faster R-CNN domain-loss kernels at the hot shapes (image-level map 8 x 37 x 75, 8 x 512 ROI rows, pooled 7,
stride 16), reported, not gated:

  * ``sfod_da_bce`` (map, and masked ROI rows) and ``sfod_da_consistency_{fwd,bwd}`` per launch, against their HBM floors from
    the bytes they must move (``bytes`` below: logits read at their padded stride count as 4 bytes each -- the floor is what a
    dense layout would need -- dense gradient arrays as written);
  * the consistency pair against the composition it replaces on the same inputs: torch sigmoid, ``sfod_roi_align_{fwd,bwd}`` on
    the chunk-padded one-channel map, torch mean / L1 -- three alternating runs each, and the two results compared;
  * ``--step``: the step time of configs/faster_rcnn_VGG_cityscapes_foggy_da.yaml at batch 8 + 8 in bf16x3.
    python tools/bench_da.py [--runs 30] [--step]
"""
import argparse
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sfod = importlib.import_module("simple-sfod_amd")
native = sfod.native
HBM = 6.29e12          # bytes / s: the measured float4-copy rate of an MI355X (8.0 TB/s on the data sheet)
DEV = "cuda"
YAML = os.path.join(ROOT, "configs", "faster_rcnn_VGG_cityscapes_foggy_da.yaml")
B, HF, WF, PER, STRIDE, POOLED, LD = 8, 37, 75, 512, 16, 7, 8


def timed(fn, runs, inner=20, warmup=5):
    """-> (median, min) ms per call of ``fn()``; ``inner`` calls enqueued back to back between one pair of events"""
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


def entry(med, mn, nbytes=None):
    out = {"us_median": round(med * 1e3, 2), "us_min": round(mn * 1e3, 2)}
    if nbytes is not None:
        floor = nbytes / HBM * 1e6
        out.update(bytes=nbytes, floor_us=round(floor, 3), median_over_floor=round(med * 1e3 / floor, 1))
    return out


def inputs():
    g = torch.Generator().manual_seed(1)
    R = B * PER
    z_img = torch.zeros(B, HF, WF, LD)
    z_img[..., 0] = torch.randn(B, HF, WF, generator=g)
    z_ins = torch.zeros(R, LD)
    z_ins[:, 0] = torch.randn(R, generator=g)
    W, H = WF * STRIDE, HF * STRIDE
    wh = torch.rand(R, 2, generator=g) ** 2 * torch.tensor([W * 0.6, H * 0.6]) + 16
    xy = torch.rand(R, 2, generator=g) * (torch.tensor([float(W), float(H)]) - wh).clamp_min(0)
    rois = torch.cat([torch.arange(B).repeat_interleave(PER)[:, None].float(), xy, torch.minimum(xy + wh, torch.tensor([float(W), float(H)]))], 1)
    rois[torch.arange(0, R, 9), 0] = -1.0          # a ninth of the rows padding, like a batch whose images have few proposals
    return z_img.to(DEV), z_ins.to(DEV), rois.to(DEV)


def composition(z_img, z_ins, rois, g):
    """what the dedicated pair replaces: sigmoid, ROIAlign of the one-channel map padded to the 8 channels its backward takes
    at least, mean / L1"""
    E = 8
    live = rois[:, 0] >= 0
    n = live.sum().clamp(min=1)

    def fwd():
        prob = torch.zeros(B, HF, WF, E, device=DEV)
        prob[..., 0] = torch.sigmoid(z_img[..., 0])
        pooled = native.roi_align_fwd(prob, rois, POOLED, 1.0 / STRIDE)
        p_img = pooled[:, :, 0].mean(1)
        p_ins = torch.sigmoid(z_ins[:, 0])
        d = (p_img - p_ins) * live
        return d.abs().sum() / n, (prob, p_ins, d)

    def bwd(state):
        prob, p_ins, d = state
        s = torch.sign(d) * (g / n)
        dout = torch.zeros(rois.shape[0], POOLED * POOLED, E, device=DEV)
        dout[:, :, 0] = (s / (POOLED * POOLED))[:, None]
        dprob = native.roi_align_bwd(dout, rois, (B, HF, WF, E), POOLED, 1.0 / STRIDE)
        p = prob[..., 0]
        return dprob[..., 0] * p * (1 - p), -s * p_ins * (1 - p_ins)
    return fwd, bwd


def kernels(runs):
    z_img, z_ins, rois = inputs()
    R, npx = rois.shape[0], B * HF * WF
    gs = torch.tensor([1.3], device=DEV)
    out = {}
    med, mn = timed(lambda: native.da_bce(z_img, 1.0), runs)
    out["da_bce_map_loss"] = entry(med, mn, 4 * npx)
    med, mn = timed(lambda: native.da_bce(z_img, 1.0, grad_scale=gs), runs)
    out["da_bce_map_loss_and_grad"] = entry(med, mn, 4 * npx + 4 * LD * npx)
    med, mn = timed(lambda: native.da_bce(z_ins, 0.0, rois=rois, grad_scale=gs), runs)
    out["da_bce_rows_loss_and_grad"] = entry(med, mn, 4 * R + 20 * R + 4 * LD * R)
    loss, st = native.da_consistency_fwd(z_img, z_ins, rois, POOLED, 1.0 / STRIDE)
    wts = 4 * R * (HF + WF)
    fwd_bytes = 4 * npx + 4 * R + 20 * R + wts + 12 * R
    bwd_bytes = 4 * npx + 4 * R + 20 * R + wts + 4 * R + 4 * LD * (npx + R)
    cfwd, cbwd = composition(z_img, z_ins, rois, gs[0])
    closs, cstate = cfwd()
    dzi, dzn = native.da_consistency_bwd(z_img, z_ins, rois, st, gs)
    cdi, cdn = cbwd(cstate)
    out["dedicated_vs_composition"] = {
        "loss": [loss[0].item(), closs.item()], "dz_img_max_abs_diff": (dzi[..., 0] - cdi).abs().max().item(),
        "dz_img_max_abs": cdi.abs().max().item(), "dz_ins_max_abs_diff": (dzn[:, 0] - cdn).abs().max().item()}
    rounds = {"dedicated_fwd": [], "composition_fwd": [], "dedicated_bwd": [], "composition_bwd": []}
    for _ in range(3):          # alternating
        rounds["dedicated_fwd"].append(timed(lambda: native.da_consistency_fwd(z_img, z_ins, rois, POOLED, 1.0 / STRIDE), runs, inner=5))
        rounds["composition_fwd"].append(timed(cfwd, runs, inner=5))
        rounds["dedicated_bwd"].append(timed(lambda: native.da_consistency_bwd(z_img, z_ins, rois, st, gs), runs, inner=5))
        rounds["composition_bwd"].append(timed(lambda: cbwd(cstate), runs, inner=5))
    for k, v in rounds.items():
        best = min(v, key=lambda t: t[0])
        e = entry(best[0], min(t[1] for t in v), {"dedicated_fwd": fwd_bytes, "dedicated_bwd": bwd_bytes}.get(k))
        e["us_median_rounds"] = [round(t[0] * 1e3, 2) for t in v]
        out["consistency_" + k] = e
    return out


def step_time(steps, warmup):
    cfg = sfod.config.setup_cfg(YAML, ["OUTPUT_DIR", "", "SOLVER.IMS_PER_BATCH", str(B), "SOLVER.IMS_PER_BATCH_TARGET", str(B),
                                       "SFOD.COMPUTE_DTYPE", "bf16x3", "SFOD.SYNTHETIC.NUM_IMAGES", str(2 * B),
                                       "SOLVER.CHECKPOINT_PERIOD", "0"])
    torch.manual_seed(cfg.SEED)
    tr = sfod.engine.get_trainer_class(cfg)(cfg)
    with tr.step_stream():
        for _ in range(warmup):
            tr.run_step()
        torch.cuda.synchronize()
        ts = []
        for _ in range(steps):
            t0 = time.perf_counter()
            tr.run_step()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    rec = tr.storage.flush()
    ts.sort()
    return {"ms_median": round(ts[len(ts) // 2], 2), "ms_min": round(ts[0], 2), "ms_max": round(ts[-1], 2), "steps": steps,
            "mode": "bf16x3", "batch": [B, B], "losses": {k: round(float(v), 5) for k, v in rec.items() if k.startswith("loss")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    native.load()
    if not torch.cuda.is_available():
        raise SystemExit("bench_da.py measures on the GPU: no device found")
    res = {"shape": {"B": B, "Hf": HF, "Wf": WF, "rois": B * PER, "pooled": POOLED, "stride": STRIDE, "ld": LD}, "runs": a.runs,
           "hbm_bytes_per_s": HBM}
    res.update(kernels(a.runs))
    if a.step:
        res["step_da_yaml"] = step_time(a.steps, a.warmup)
    for k, v in res.items():
        print(f"{k:28s} {v}", file=sys.stderr)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
