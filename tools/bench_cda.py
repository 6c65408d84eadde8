"""Times of the conditional DA Faster R-CNN pieces at the yaml's shapes (R = 8 x 512 ROI rows, D = 1024 box features, C = 9
classes) in bf16x3, reported, not gated:

  * ``sfod_cda_condition_fwd`` / ``_bwd`` per launch against their HBM floors (bytes of x written + f read; bytes of dx read +
    df written), and against the composition torch offers on the same inputs (``softmax``, ``bmm``, ``view``, ``native.cast``;
    ``einsum`` for the backward) -- three alternating rounds each, results compared;
  * the instance branch of one domain (condition, DAInsHead forward and backward, contraction) in the form the model runs
    -- fc1 once per direction -- and with fc1 evaluated once per ``DAInsHead`` evaluation, called from here out of the node's
    own pieces (there is no switch in the model), alternating;
  * ``--step``: step time and peak reserved memory of configs/faster_rcnn_VGG_cityscapes_foggy_cda.yaml at batch 8 + 8 in bf16x3
    next to the DA yaml's, alternating.
    python tools/bench_cda.py [--runs 20] [--step]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
sfod = importlib.import_module("simple-sfod_amd")
native = sfod.native
from bench_da import HBM, DEV, timed, entry      # noqa: E402

CONFIGS = os.path.join(ROOT, "configs")
YAMLS = {"cda": os.path.join(CONFIGS, "faster_rcnn_VGG_cityscapes_foggy_cda.yaml"),
         "da": os.path.join(CONFIGS, "faster_rcnn_VGG_cityscapes_foggy_da.yaml")}
B, PER, D, NCLS, LD = 8, 512, 1024, 9, 48
MODE = "bf16x3"


def inputs():
    g = torch.Generator().manual_seed(1)
    R = B * PER
    f = torch.relu(torch.randn(R, D, generator=g))
    scores = torch.zeros(R, LD)
    scores[:, :NCLS] = torch.randn(R, NCLS, generator=g) * 2
    rois = torch.zeros(R, 5)
    rois[:, 0] = torch.arange(B).repeat_interleave(PER).float()
    rois[torch.arange(0, R, 9), 0] = -1.0          # a ninth of the rows padding
    return f.to(DEV), scores.to(DEV), rois.to(DEV)


def best_of(rounds, nbytes=None):
    best = min(rounds, key=lambda t: t[0])
    e = entry(best[0], min(t[1] for t in rounds), nbytes)
    e["us_median_rounds"] = [round(t[0] * 1e3, 2) for t in rounds]
    return e


def kernels(runs):
    f32, scores, rois = inputs()
    R = f32.shape[0]
    pair = native.SPLIT_DTYPE
    f = native.cast(f32, pair)
    live = (rois[:, 0] >= 0).float()[:, None]
    x, _, p, w = native.cda_condition_fwd(f, scores, NCLS, rois, entropy=True, out_dtype=pair)

    def comp_fwd():
        g = torch.softmax(scores[:, :NCLS], dim=1) * live
        return native.cast(torch.bmm(g.unsqueeze(2), f32.unsqueeze(1)).view(R, -1), pair), g
    xc, g = comp_fwd()
    dx = torch.randn(R, NCLS * D, device=DEV)
    df = native.cda_condition_bwd(dx, p, rois)
    comp_bwd = lambda: torch.einsum("rc,rcd->rd", p, dx.view(R, NCLS, D))
    out = {"condition_vs_composition": {
        "x_max_abs_diff": (native.cast(x, torch.float32) - native.cast(xc, torch.float32)).abs().max().item(),
        "p_max_abs_diff": (p - g).abs().max().item(), "df_max_abs_diff": (df - comp_bwd()).abs().max().item(),
        "df_max_abs": df.abs().max().item()}}
    fwd_bytes = 4 * R * NCLS * D + 4 * R * D + 4 * R * NCLS * 2 + 24 * R      # x (pairs: 4 bytes) + f + scores, p + rois, w
    bwd_bytes = 4 * R * NCLS * D + 4 * R * D + 4 * R * NCLS + 20 * R
    rounds = {"condition_fwd": [], "composition_fwd": [], "condition_bwd": [], "composition_bwd": []}
    for _ in range(3):          # alternating
        rounds["condition_fwd"].append(timed(lambda: native.cda_condition_fwd(f, scores, NCLS, rois, entropy=True, out_dtype=pair), runs, inner=5))
        rounds["composition_fwd"].append(timed(comp_fwd, runs, inner=5))
        rounds["condition_bwd"].append(timed(lambda: native.cda_condition_bwd(dx, p, rois), runs, inner=5))
        rounds["composition_bwd"].append(timed(comp_bwd, runs, inner=5))
    for k, v in rounds.items():
        out[k] = best_of(v, {"condition_fwd": fwd_bytes, "condition_bwd": bwd_bytes}.get(k))
    out["condition_fwd"]["composition_over_kernel"] = round(out["composition_fwd"]["us_median"] / out["condition_fwd"]["us_median"], 2)
    out["condition_bwd"]["composition_over_kernel"] = round(out["composition_bwd"]["us_median"] / out["condition_bwd"]["us_median"], 2)
    return out


def instance_branch(runs):
    """one domain's instance branch, forward and backward, out of the node's pieces: fc1 once (the model's form) or twice"""
    M = sfod.modeling.cda_faster_rcnn
    cfg = sfod.config.setup_cfg(YAMLS["cda"], ["OUTPUT_DIR", "", "SFOD.COMPUTE_DTYPE", MODE])
    torch.manual_seed(0)
    head = sfod.modeling.build_model(cfg).DC_ins
    dtype = native.mode_dtype(MODE)
    gdtype = native.grad_dtype_of(dtype)
    dt, gdt = native.dt_of_dtype(dtype), native.dt_of_dtype(gdtype)
    fc1 = sfod.modeling.dann.ins_head_layers(head)[0]
    f32, scores, rois = inputs()
    R = f32.shape[0]
    f = native.cast(f32, dtype)
    g = torch.Generator().manual_seed(2)
    masks = [[(torch.rand(R, 1024, generator=g) >= 0.5).to(torch.uint8).to(DEV) for _ in range(2)] for _ in range(2)]
    dz = torch.zeros(R, 8, device=DEV)
    dz[:, 0] = torch.randn(R, generator=g).to(DEV) / R
    w_n, w_c = 0.1, 0.1

    def branch(two):
        xc, xg, p, w = native.cda_condition_fwd(f, scores, NCLS, rois, entropy=True, out_dtype=dtype, with_grad_operand=True)
        lin = lambda: native.conv_fwd(xc, native.pack_fc_weight(fc1.weight.detach(), dt), fc1.bias.detach(), 1024, 1, act=1)
        r1a = lin()
        r1b = lin() if two else r1a
        ev = [M._ins_tail_logits(head, r1a, masks[0], dtype), M._ins_tail_logits(head, r1b, masks[1], dtype)]
        d1 = [M._ins_tail_backward(head, e, dz, dtype)[0] for e in ev]
        wt = lambda: native.pack_fc_weight(fc1.weight.detach(), gdt, transpose=True)
        if two:
            dw1 = native.conv_wgrad(xg, d1[0], 1024, 1, operand=gdtype) + native.conv_wgrad(xg, d1[1], 1024, 1, operand=gdtype)
            db1 = native.bias_grad(d1[0], 1024) + native.bias_grad(d1[1], 1024)
            dxc = torch.add(native.conv_fwd(d1[0], wt(), None, fc1.in_features, 1) * (-w_n),
                            native.conv_fwd(d1[1], wt(), None, fc1.in_features, 1), alpha=w_c * w_n)
        else:
            par = d1[0] + d1[1]
            dw1, db1 = native.conv_wgrad(xg, par, 1024, 1, operand=gdtype), native.bias_grad(par, 1024)
            dxc = native.conv_fwd(torch.add(d1[0] * (-w_n), d1[1], alpha=w_c * w_n), wt(), None, fc1.in_features, 1)
        return native.cda_condition_bwd(dxc, p, rois), dw1, db1

    a, b = branch(False), branch(True)
    out = {"agreement": {n: ((x - y).norm() / y.norm()).item() for n, x, y in zip(("df", "dw1", "db1"), a, b)}}
    rounds = {"fc1_once": [], "fc1_twice": []}
    for _ in range(3):
        rounds["fc1_once"].append(timed(lambda: branch(False), runs, inner=2, warmup=2))
        rounds["fc1_twice"].append(timed(lambda: branch(True), runs, inner=2, warmup=2))
    out.update({k: best_of(v) for k, v in rounds.items()})
    out["saving_us_per_domain"] = round(out["fc1_twice"]["us_median"] - out["fc1_once"]["us_median"], 1)
    return out


def step_time(which, steps, warmup):
    cfg = sfod.config.setup_cfg(YAMLS[which], ["OUTPUT_DIR", "", "SOLVER.IMS_PER_BATCH", str(B), "SOLVER.IMS_PER_BATCH_TARGET", str(B),
                                               "SFOD.COMPUTE_DTYPE", MODE, "SFOD.SYNTHETIC.NUM_IMAGES", str(2 * B),
                                               "SOLVER.CHECKPOINT_PERIOD", "0"])
    torch.manual_seed(cfg.SEED)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
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
    out = {"ms_median": round(ts[len(ts) // 2], 2), "ms_min": round(ts[0], 2), "ms_max": round(ts[-1], 2), "steps": steps,
           "mode": MODE, "batch": [B, B], "peak_reserved_mb": round(torch.cuda.max_memory_reserved() / 2 ** 20, 1),
           "peak_allocated_mb": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1),
           "losses": {k: round(float(v), 5) for k, v in rec.items() if k.startswith("loss")}}
    del tr
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    native.load()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cda.py measures on the GPU: no device found")
    res = {"shape": {"rois": B * PER, "D": D, "C": NCLS, "score_ld": LD, "mode": MODE}, "runs": a.runs, "hbm_bytes_per_s": HBM}
    res.update(kernels(a.runs))
    res["instance_branch"] = instance_branch(max(a.runs // 2, 3))
    if a.step:
        for rnd in range(2):          # alternating
            for which in ("da", "cda"):
                res[f"step_{which}_yaml_round{rnd}"] = step_time(which, a.steps, a.warmup)
    for k, v in res.items():
        print(f"{k:28s} {v}", file=sys.stderr)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
