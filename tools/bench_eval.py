"""Evaluation-path throughput: eval-mode inference images/s on the synthetic evaluation set
(1024x2048 frames -> ResizeShortestEdge(600) on the device -> backbone -> RPN (TEST top-k 6000 / 1000) -> box head
-> per-class NMS -> detector_postprocess), plus the host-side AP table time.  One JSON line.
``--tta``: the same set behind ``GeneralizedRCNNWithTTA`` (TEST.AUG, d2's default sizes); the line then
also carries the share of the device time spent outside the model passes (resizes, concatenation, the merge chain).
``--coco-device``: SFOD.COCO_EVAL_DEVICE True (COCOeval's matching in ``sfod_coco_match``); combines with ``--evaluators coco,f1``.
The line then also carries the SCORING time -- everything ``inference_on_dataset`` does outside the model call plus
``evaluate()`` -- of ``--scoring-runs`` extra passes in which the device is drained after the model and after ``process``,
for the device path (its kernel, copy, rebuild and ``accumulate`` listed apart) and for this tree's host path fed the same
outputs in the same pass."""
import argparse
import importlib
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--evaluators", default="coco", help="SFOD.EVALUATORS, comma separated: coco | coco,f1")
    ap.add_argument("--tta", action="store_true", help="run behind GeneralizedRCNNWithTTA (TEST.AUG)")
    ap.add_argument("--coco-device", action="store_true", help="SFOD.COCO_EVAL_DEVICE True: COCOeval's matching on the device")
    ap.add_argument("--scoring-runs", type=int, default=3, help="--coco-device: timed scoring passes per path")
    args = ap.parse_args()
    sfod = importlib.import_module("simple-sfod_amd")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = sfod.config.setup_cfg(
        os.path.join(root, "configs", "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free.yaml"),
        ["OUTPUT_DIR", "", "SFOD.COMPUTE_DTYPE", args.dtype, "TEST.IMS_PER_BATCH", str(args.batch), "SFOD.SYNTHETIC.NUM_TEST_IMAGES", str(args.images),
         "DATASETS.TEST", "('synthetic_cityscapes_foggy_val',)", "SFOD.EVALUATORS", repr(tuple(args.evaluators.split(",")))]
        + (["TEST.AUG.ENABLED", "True"] if args.tta else []) + (["SFOD.COCO_EVAL_DEVICE", "True"] if args.coco_device else []))
    torch.manual_seed(0)
    T = sfod.engine.BaseTrainer
    model = T.build_model(cfg)
    with torch.no_grad():        # planted scores so that the per-class NMS and the evaluator see detections
        model.roi_heads.box_predictor.cls_score.weight.mul_(60.0)
    loader = T.build_test_loader(cfg, "synthetic_cityscapes_foggy_val")
    evaluator = T.build_evaluator(cfg, "synthetic_cityscapes_foggy_val", data_loader=loader)
    model.eval()
    passes = []                  # (start, end) events around every model pass under --tta
    if args.tta:
        inner = model.inference

        def timed_inference(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = inner(*a, **k)
            e1.record()
            passes.append((e0, e1))
            return out

        model.inference = timed_inference
        model = sfod.modeling.GeneralizedRCNNWithTTA(cfg, model)
    whole = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    with torch.no_grad():
        for batch in loader:     # warm-up pass
            model(batch)
        torch.cuda.synchronize()
        del passes[:]
        whole[0].record()
        t0 = time.perf_counter()
        n = 0
        for _ in range(args.passes):
            evaluator.reset()
            for batch in loader:
                outs = model(batch)
                evaluator.process(batch, outs)
                n += len(batch)
        whole[1].record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
    coco = getattr(evaluator, "_evaluators", [evaluator])[0]
    n_det = int(sum(int(m[1].sum()) for m in coco._matched)) if args.coco_device else None
    te = time.perf_counter()
    res = evaluator.evaluate()
    t2 = time.perf_counter()
    out = {"metric": "eval-mode inference images/s (incl. postprocess + evaluator.process)",
           "value": round(n / (t1 - t0), 2), "unit": "images/s", "n_gpus": 1, "batch": args.batch,
           "images": n, "ap_table_seconds": round(t2 - te, 3),
           "detections": n_det if args.coco_device else len([d for p in coco._predictions for d in p["instances"]]),
           "AP50": res["bbox"]["AP50"], "dtype": cfg.SFOD.COMPUTE_DTYPE, "data": "synthetic",
           "evaluators": list(cfg.SFOD.EVALUATORS)}
    if args.tta:
        in_passes, total = sum(a.elapsed_time(b) for a, b in passes), whole[0].elapsed_time(whole[1])
        out.update({"tta": True, "tta_min_sizes": list(cfg.TEST.AUG.MIN_SIZES), "tta_flip": bool(cfg.TEST.AUG.FLIP),
                    "model_passes": len(passes), "device_ms_total": round(total, 2), "device_ms_in_model_passes": round(in_passes, 2),
                    "share_outside_model_passes": round(1.0 - in_passes / total, 4)})
    if args.coco_device:
        out.update(scoring(sfod, cfg, args, model, loader, coco, res))
    if "F1 Score" in res:
        out["F1 Score"] = res["F1 Score"]
    print(json.dumps(out))


def scoring(sfod, cfg, args, model, loader, dev_ev, res):
    """``--scoring-runs`` passes over the set with the device drained after the model and after each ``process``: wall seconds
    outside the model call (``process``) plus ``evaluate()``, for the device path and for the host path on the same outputs"""
    E, native = sfod.evaluation, sfod.native
    host_ev = E.NewCOCOEvaluator(dev_ev.dataset_name, loader.dataset.dataset_dicts(cfg), dev_ev.class_names)
    runs = {"device": [], "host": []}
    parts = {"device_process_s": [], "kernel_s": [], "copy_s": [], "rebuild_s": [], "accumulate_s": [], "host_process_s": [],
             "host_evaluate_s": []}
    same = True
    for _ in range(args.scoring_runs):
        dev_ev.reset()
        host_ev.reset()
        timer = native.KernelTimer(watch=("sfod_coco_match",))
        spent = {"device": 0.0, "host": 0.0}
        with torch.no_grad():
            for batch in loader:
                outs = model(batch)
                torch.cuda.synchronize()
                for name, ev in (("device", dev_ev), ("host", host_ev)):
                    native.set_timer(timer if name == "device" else None)
                    t0 = time.perf_counter()
                    ev.process(batch, outs)
                    torch.cuda.synchronize()
                    spent[name] += time.perf_counter() - t0
        native.set_timer(None)
        t0 = time.perf_counter()
        got = dev_ev.evaluate()
        t1 = time.perf_counter()
        want = host_ev.evaluate()
        t2 = time.perf_counter()
        same = same and str(got) == str(want) and str(got["bbox"]) == str(res["bbox"])
        runs["device"].append(spent["device"] + t1 - t0)
        runs["host"].append(spent["host"] + t2 - t1)
        parts["device_process_s"].append(spent["device"])
        parts["kernel_s"].append(sum(v["ms"] for v in timer.summary().values()) / 1e3)
        for k in ("copy_s", "rebuild_s", "accumulate_s"):
            parts[k].append(dev_ev.timings[k])
        parts["host_process_s"].append(spent["host"])
        parts["host_evaluate_s"].append(t2 - t1)
    r4 = lambda v: [round(x, 4) for x in v]
    return {"coco_device": True, "device_equals_host": same, "scoring_seconds_device": r4(runs["device"]),
            "scoring_seconds_host": r4(runs["host"]), "scoring_parts": {k: r4(v) for k, v in parts.items()}}


if __name__ == "__main__":
    main()
