#!/usr/bin/env python
"""Time of TEST.PRECISE_BN's statistics passes at the hot yaml's shapes (B frames per pass at 600 x 1200), beside the same
number of AdaBN-style passes (the momentum path), and of the commit launch.

    python tools/bench_precise_bn.py [--passes 40] [--reps 5] [--batch 8] [--modes momentum precise] [--dtype bf16x3]

Every repetition runs ``--passes`` train-mode forward passes under no_grad (``model.preprocess_image`` + ``model._features``)
over the same pre-drawn batches, between two device synchronisations; the modes alternate inside each repetition.  A tree
without engine/precise_bn.py (the parent of that change) runs ``--modes momentum`` only, so that the two trees can be
alternated by the caller.  Prints one JSON line."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--dtype", default="bf16x3")
    ap.add_argument("--modes", nargs="+", default=["momentum", "precise"], choices=["momentum", "precise"])
    args = ap.parse_args()
    import torch
    sfod = importlib.import_module("simple-sfod_amd")
    sfod.native.load()
    yaml = os.path.join(ROOT, "configs", "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free.yaml")
    cfg = sfod.config.setup_cfg(yaml, ["OUTPUT_DIR", "", "SFOD.COMPUTE_DTYPE", args.dtype, "SOLVER.IMS_PER_BATCH_TARGET",
                                       str(args.batch), "SFOD.SYNTHETIC.NUM_IMAGES", "16"])
    torch.manual_seed(0)
    model = sfod.modeling.build_model(cfg).train()
    loader = iter(sfod.data.TwoCropLoader(cfg, torch.device(cfg.MODEL.DEVICE), labeled=False))
    batches = [next(loader)[1] for _ in range(4)]
    seq = [batches[i % len(batches)] for i in range(args.passes)]

    @torch.no_grad()
    def momentum():
        for b in seq:
            model._features(model.preprocess_image(b))

    def precise():
        sfod.engine.precise_bn.update_bn_stats(model, seq, args.passes)
    fns = {"momentum": momentum, "precise": precise}
    times = {m: [] for m in args.modes}
    for rep in range(args.reps + 1):                      # repetition 0 warms every shape up and is dropped
        for m in args.modes:
            torch.cuda.synchronize()
            t = time.perf_counter()
            fns[m]()
            torch.cuda.synchronize()
            if rep:
                times[m].append(round((time.perf_counter() - t) * 1e3, 3))
    out = {"passes": args.passes, "batch": args.batch, "dtype": args.dtype, "image": list(batches[0][0]["image"].shape),
           "ms_per_repetition": times}
    if "precise" in args.modes:
        native = sfod.native
        bns = sfod.engine.precise_bn.get_bn_modules(model)
        acc, views = native.bn_pop_accumulator([bn.num_features for bn in bns], cfg.MODEL.DEVICE)
        acc[0].fill_(1.0)
        layers, off = [], 0
        for bn in bns:
            layers.append((off, bn.running_mean.clone(), bn.running_var.clone()))
            off += bn.num_features
        rows = torch.tensor([[o, rm.numel(), rm.data_ptr(), rv.data_ptr()] for o, rm, rv in layers], dtype=torch.int64)
        dev_rows = rows.to(acc.device)
        for _ in range(20):
            native.call("sfod_bn_pop_commit", acc, acc.stride(0), dev_rows, rows.data_ptr(), len(layers))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 200
        torch.cuda.synchronize()
        t = time.perf_counter()
        a.record()
        for _ in range(n):
            native.call("sfod_bn_pop_commit", acc, acc.stride(0), dev_rows, rows.data_ptr(), len(layers))
        b.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t) / n * 1e6
        out["commit"] = {"layers": len(layers), "columns": int(acc.shape[1]), "launches": n,
                         "us_per_launch_back_to_back_events": round(a.elapsed_time(b) / n * 1e3, 2),
                         "us_per_call_host_wall": round(wall, 2)}
        t = time.perf_counter()
        native.bn_pop_commit(acc, layers)
        torch.cuda.synchronize()
        out["commit"]["ms_one_call_with_table_upload"] = round((time.perf_counter() - t) * 1e3, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
