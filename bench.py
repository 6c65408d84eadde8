#!/usr/bin/env python
"""Headline benchmark: teacher+student training images/s on synthetic 1024x2048 frames.

One "step" = one pass of the hot path over one batch: teacher forward (train-mode BN / AdaBN
refresh) -> NMS pseudo-labelling -> student forward + backward -> (RCCL grad all-reduce) ->
fused SGD + EMA.  Inputs are resident in HBM before the timed region (the mapper's output:
uint8 CHW tensors, 1024x2048 frames resized to 600x1200 by INPUT.MIN_SIZE_TRAIN=600 of the
named config; ``--res full`` overrides the config to feed 1024x2048 tensors).

``value`` is measured in an arithmetic mode whose parity against the CPU oracle is gated AT THIS FRAME SIZE by
tests/test_gpu_fullsize.py for the config being run: ``bf16x3`` for the VGG16 configs (split-precision products on the
bf16 matrix pipe, about 16 significand bits per operand: losses and boxes within 1e-4, intermediates within 2e-4), ``f16x3``
for ``--model r101`` (the same three-MFMA product with the forward operands as IEEE half pairs, 22 bits each: gated like
fp32) -- on that 101-layer network bf16x3 reaches only ~1e-3 (the test says so), so it is NOT reported as ``value`` there.
Other modes are measured afterwards by child processes and reported in labelled blocks, never as ``value``: faster, less
exact ones under ``reduced_precision_mode``; the tighter parity modes of the same config (VGG16: ``f16x3`` and ``fp32``, the
reference's own arithmetic; r101: ``fp32``) under ``other_parity_modes``.

Contract: ``python bench.py --gpus N --steps K --warmup W``; rank 0 prints ONE JSON line.  N > 1: either started under
``python -m torch.distributed.run`` (RANK / WORLD_SIZE in the environment), or plainly -- then the script starts the N
ranks itself in a child process before touching the GPU (simple-sfod_amd/launch.py).

A plain run does what the headline needs and nothing else: set-up (incl. the planted head's calibration), W warm-up steps,
K timed steps, the outputs of the last timed step if ``--dump-outputs DIR`` is given, the result line.  Everything else
the line can carry is measured only with ``--full``: the roofline / per-kernel segment, the host-enqueue check
(``gpu_fill``), the other precisions and shapes (child processes), the CPU baseline, rocm-smi clock / power samples and,
for N > 1, the exchange block and RCCL's per-rank log.

``--dump-outputs DIR``: what the last timed step computed, as ``DIR/<name>.npy`` (float32, scalars float64): its logged
scalars (losses, pseudo-label statistics), the pseudo labels the teacher handed to the student, and a fixed seeded
sample of the student's parameters and gradient and of the teacher's parameters (+ both BatchNorm statistics).  Inputs
are seeded and every run's step sums its gradients in a fixed order (SFOD.DETERMINISTIC, see build_trainer), so two runs
with the same arguments write bit-identical files and two builds can be compared file by file.
"""
import argparse
import importlib
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# algorithmic forward FLOPs (2 x MACs) per image, SURVEY.md section 8d
FLOPS = {
    "r600": {"trunk": 439.90e9, "rpn": 3.19e9, "box512": 27.42e9, "box2000": 107.12e9},
    "full": {"trunk": 1282.85e9, "rpn": 9.82e9, "box512": 27.42e9, "box2000": 107.12e9},
}
# ResNet-101-C4 (BASELINE config #5): stem + res2 are frozen (FREEZE_AT=2) -> no backward through them
FLOPS_R101 = {
    "r600": {"trunk": 198.14e9, "frozen": 19.2e9 + 3.4e9, "rpn": 54.14e9, "box256": 54.80e9, "box2000": 428.15e9},
    "full": {"trunk": 571.43e9, "frozen": 55.8e9 + 9.9e9, "rpn": 155.63e9, "box256": 54.80e9, "box2000": 428.15e9},
}
YAML = {"vgg": "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free.yaml",
        "r101": "r101_c4_cs_foggy_adaptive_teacher_source_free.yaml",
        "vgg_base": "faster_rcnn_VGG_cityscapes_source_new.yaml"}     # BASELINE config #2 (TRAINER: "base")
# dense MFMA TFLOP/s (MI355X_MICROARCH.md) per ALGORITHMIC flop: bf16x3 issues three bf16 MFMAs per product
# (hi*hi + hi*lo + lo*hi), so its ceiling for the convolution's own 2*M*N*K count is the bf16 peak / 3
PEAK = {"bf16": 2500.0, "fp32": 157.3, "bf16x3": 2500.0 / 3.0, "f16x3": 2500.0 / 3.0}
# the mode test_gpu_fullsize.py gates at the north star's 1e-4 for each model = what `value` is measured in
PARITY_DTYPE = {"vgg": "bf16x3", "r101": "f16x3"}
# further modes that pass the same fullsize gates on the config (reported beside `value`, measured by child processes)
# (fp32 = the reference's own arithmetic: every default line carries one number in it)
OTHER_PARITY = {"vgg": {"bf16x3": ["f16x3", "fp32"], "f16x3": ["fp32"]}, "r101": {"f16x3": ["fp32"]}}
# "planted-label" mode (BASELINE.md section 3 / SURVEY 8d: "teacher box-predictor bias is set so ~10-30 boxes/image pass"):
# seeded random weights give no detection above 0.8, so the class logits are spread by a moderate scale on cls_score's
# weights and the BACKGROUND bias is calibrated at start-up, by bisection over untimed teacher passes on the bench's
# own frames, until the mean number of pseudo labels per image is the target.  The realised count
# and the student's loss_cls_pseudo over warm-up + timed steps are asserted and reported in `config`.
# The head itself lives in the package (simple-sfod_amd/engine/planted.py: SCALE vgg x16 / r101 x4, TARGET 20, RANGE 10-30) so
# that tests/test_gpu_fullsize.py and tests/test_gpu_pseudo_labels.py gate exactly the head this file times.
# the committed PMC captures (profiles/pmc_hbm_traffic_latest.json: VGG16 bf16x3; pmc_hbm_traffic_r101_latest.json: R101 f16x3)
# were taken on exactly these run configurations
PMC_CAPTURE = {"trainer": "source_free", "res": "r600", "batch": 8,
               "files": {"vgg": ("bf16x3", "pmc_hbm_traffic_latest.json"), "r101": ("f16x3", "pmc_hbm_traffic_r101_latest.json")}}


def step_flops(res, model="vgg", trainer="source_free"):
    if trainer == "base":      # source-only step (base.py:93-123): student forward + backward, no teacher
        f = FLOPS[res]
        return 3 * (f["trunk"] + f["rpn"] + f["box512"])
    if model == "r101":
        f = FLOPS_R101[res]
        teacher = f["trunk"] + f["rpn"] + f["box2000"]
        student = f["trunk"] + f["rpn"] + f["box256"]
        return teacher + student + 2 * (student - f["frozen"])
    f = FLOPS[res]
    teacher = f["trunk"] + f["rpn"] + f["box2000"]
    student = f["trunk"] + f["rpn"] + f["box512"]
    return teacher + 3 * student  # student backward = 2 x forward


def physical_cores():
    try:
        ids, phys, core = set(), None, None
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                phys = line.split(":")[1].strip()
            elif line.startswith("core id"):
                core = line.split(":")[1].strip()
            elif not line.strip():
                if phys is not None and core is not None:
                    ids.add((phys, core))
                phys = core = None
        if ids:
            return len(ids)
    except OSError:
        pass
    return max(1, (os.cpu_count() or 2) // 2)


def cpu_baseline(res, planted, model="vgg"):
    """The CPU oracle (kind "port": the PyTorch-CPU restatement of the reference's Detectron2 path -- the reference
    itself cannot run here, Detectron2 is absent) on a bounded sample: ONE image per step, 1 warm-up + 3 timed
    teacher+student steps, one thread per physical core, with the split over the stages."""
    import torch
    from oracle import model as om
    cores = physical_cores()
    torch.set_num_threads(cores)
    cfg = om.Cfg.r101_c4() if model == "r101" else om.Cfg()
    sd_t = om.init_state(cfg, seed=0)
    if planted:      # the GPU run's planted head: same weight scale, the background bias it calibrated
        sd_t["roi_heads.box_predictor.cls_score.weight"] *= planted["cls_score_weight_scale"]
        sd_t["roi_heads.box_predictor.cls_score.bias"][-1] = planted["background_bias"]
    sd_s = om.clone_state(sd_t, requires_grad=True)
    h, w = (600, 1200) if res == "r600" else (1024, 2048)
    g = torch.Generator().manual_seed(42)
    hf, wf = (-(-h // 16), -(-w // 16)) if model == "r101" else (h // 32, w // 32)
    stages = {"teacher_forward": 0.0, "student_forward": 0.0, "student_backward": 0.0, "sgd_ema": 0.0}
    bufs, total, timed = {}, 0.0, 3
    for it in range(1 + timed):
        img = [torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8)]
        rk = [torch.randint(0, 2 ** 31 - 1, (hf * wf * cfg.num_anchors,), generator=g)]
        ok = [torch.randint(0, 2 ** 31 - 1, (2100,), generator=g)]
        t0 = time.perf_counter()
        props, dets = om.teacher_forward(sd_t, img, cfg)
        pl = [om.threshold_bbox(d, cfg.bbox_threshold) for d in dets]
        t1 = time.perf_counter()
        losses = om.student_losses(sd_s, img, [p["gt_boxes"] for p in pl], [p["gt_classes"] for p in pl], rk, ok, cfg)
        t2 = time.perf_counter()
        for v in sd_s.values():
            if getattr(v, "grad", None) is not None:
                v.grad = None
        sum(v for k, v in losses.items() if k != "loss_bpc").backward()
        t3 = time.perf_counter()
        grads = {k: v.grad for k, v in sd_s.items() if getattr(v, "grad", None) is not None}
        om.sgd_step(sd_s, grads, bufs, lr=0.0025 * 0.001)
        om.ema_update(sd_t, {k: v.detach() for k, v in sd_s.items()}, 0.9996)
        t4 = time.perf_counter()
        if it == 0:
            continue            # warm-up (allocator, oneDNN primitive cache)
        for k, d in zip(stages, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            stages[k] += d / timed
        total += (t4 - t0) / timed
    return {"value": round(1.0 / total, 4), "unit": "images/s", "cores": cores, "kind": "port",
            "sample": f"1 warm-up + {timed} timed teacher+student steps on 1 synthetic {h}x{w} image each (oracle/, "
                      f"PyTorch-CPU fp32, {torch.get_num_threads()} threads = physical cores of {os.cpu_count()} logical), "
                      f"{total:.2f} s/step",
            "seconds_per_stage": {k: round(v, 3) for k, v in stages.items()}}


def pmc_traffic(model, *kernel_substrs):
    """HBM bytes per launch of the dominant kernel family from the committed PMC passes (rocprofv3 --pmc
    FETCH_SIZE / WRITE_SIZE in separate runs, gfx950 corrections applied by tools/pmc_summary.py): the
    launch-weighted mean over the family's template instantiations (tile shapes, with / without the BatchNorm-backward
    epilogue), i.e. per launch over the same set of launches as `achieved`.  bench.py cannot collect counters itself."""
    fname = PMC_CAPTURE["files"][model][1]
    path = os.path.join(ROOT, "profiles", fname)
    if not os.path.exists(path):
        return None
    try:
        # the capture is only valid for the kernels it was taken on: tools/pmc_summary.py stamps it with the fingerprint of
        # simple-sfod_amd/csrc + include/ (csrc/build.py::source_fingerprint); a different source tree -> no traffic figure
        meta = json.load(open(path + ".meta")) if os.path.exists(path + ".meta") else {}
        if meta.get("csrc_fingerprint") != csrc_fingerprint():
            return None
        # an entry of kernel_substrs may be a tuple of alternatives (template arguments print differently across builds)
        rows = [r for r in json.load(open(path))
                if all(any(a in r["kernel"] for a in ((k,) if isinstance(k, str) else k)) for k in kernel_substrs)]
        n = sum(r["launches"] for r in rows)
        if n == 0:
            return None
        return {"hbm_read_MB_per_launch": round(sum(r["hbm_read_MB_per_launch"] * r["launches"] for r in rows) / n, 3),
                "hbm_write_MB_per_launch": round(sum(r["hbm_write_MB_per_launch"] * r["launches"] for r in rows) / n, 3),
                "kernels": len(rows), "launches_counted": n, "source": "profiles/" + fname}
    except Exception:
        return None


def csrc_fingerprint():
    spec = importlib.util.spec_from_file_location("sfod_csrc_build", os.path.join(ROOT, "simple-sfod_amd", "csrc", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.source_fingerprint()


def pmc_matches(args):
    return (args.model in PMC_CAPTURE["files"] and args.dtype == PMC_CAPTURE["files"][args.model][0] and
            args.trainer == PMC_CAPTURE["trainer"] and args.res == PMC_CAPTURE["res"] and args.batch == PMC_CAPTURE["batch"]
            and not args.opts)


def _by_path(name, fname):
    """a standard-library-only module of the package, loaded by path (before torch / the package are imported)"""
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "simple-sfod_amd", fname))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _launcher():
    return _by_path("sfod_launch", "launch.py")


def build_trainer(sfod, args, dtype, world, rank, local_rank):
    import torch
    # SFOD.DETERMINISTIC: the same step with every gradient sum in a fixed order (slabs instead of float atomics), so a run
    # with the same arguments computes the same bits every time.  With the atomics two runs differ in the last bits and
    # self-training on its own pseudo labels grows that into other pseudo labels and losses within a hundred steps (the
    # planted-workload check itself can fail on it).  Cost, same box, alternating: 0.4 % of the headline's images/s, 0.7 %
    # for --model r101, 0.9 % for --trainer base (the slab pass over the split partials); ``--opts SFOD.DETERMINISTIC
    # False`` times the atomics, the mode of the figures recorded before this choice.
    opts = ["OUTPUT_DIR", "", "SFOD.COMPUTE_DTYPE", dtype, "SOLVER.CHECKPOINT_PERIOD", "0", "SFOD.DETERMINISTIC", "True",
            "SFOD.SYNTHETIC.NUM_IMAGES", str(max(16, 2 * args.batch)), "MODEL.DEVICE", f"cuda:{local_rank}",
            "TEST.EVAL_PERIOD", "0", "TEST.VAL_LOSS", "False"]
    if args.trainer == "base":
        opts += ["SOLVER.IMS_PER_BATCH", str(args.batch * world)]
    else:
        opts += ["SOLVER.IMS_PER_BATCH_TARGET", str(args.batch * world)]
    if args.no_overlap:
        opts += ["SFOD.OVERLAP_TEACHER", "False"]
        os.environ["SFOD_RESNET_WGRAD_STREAM"] = "0"      # ... and the backward's weight gradients too: ONE stream
        os.environ["SFOD_VGG_WGRAD_STREAM"] = "0"
    if args.res == "full":
        opts += ["INPUT.MIN_SIZE_TRAIN", "(1024,)", "INPUT.MAX_SIZE_TRAIN", "2048"]
    if args.host_frames:
        opts += ["SFOD.SYNTHETIC.HOST_FRAMES", "True"]
    yaml = YAML["vgg_base"] if args.trainer == "base" else YAML[args.model]
    cfg = sfod.config.setup_cfg(os.path.join(ROOT, "configs", yaml), opts + list(args.opts))
    torch.manual_seed(cfg.SEED + rank)
    if args.trainer == "base":
        trainer = sfod.engine.BaseTrainer(cfg)
    else:
        trainer = sfod.engine.SourceFreeAdaptiveTeacherTrainer(cfg)
    return cfg, trainer


class StepLog:
    """per-step device scalars of the run (no host sync until ``summary``): pseudo labels per image, loss_cls_pseudo"""

    def __init__(self):
        self.n_pseudo, self.loss_cls = [], []

    def after_step(self, trainer):
        p = trainer.storage._pending
        if "roi_head/num_pseudo_proposals" in p:
            self.n_pseudo.append(p["roi_head/num_pseudo_proposals"])
        if "loss_cls_pseudo" in p:
            self.loss_cls.append(p["loss_cls_pseudo"])

    def summary(self, first=None):
        """``first``: only the first that many logged steps (the window the workload check is made on)"""
        import torch
        out = {}
        for k, v in (("pseudo_labels_per_image", self.n_pseudo), ("loss_cls_pseudo", self.loss_cls)):
            v = v[:first] if first else v
            if v:
                t = torch.stack([x.detach().float().reshape(()) for x in v]).cpu()
                out[k] = {"mean": round(t.mean().item(), 3), "min": round(t.min().item(), 3), "max": round(t.max().item(), 3),
                          "steps": int(t.numel())}
        return out


STEP_LOG = None
CHECK_WINDOW = 120      # logged steps (warm-up + timed) the planted-workload check covers
DUMP_SAMPLE = 1 << 21   # --dump-outputs: elements sampled from each large flat buffer (8 MB in float32)


def record_pseudo_labels(trainer):
    """Keep the pseudo labels of the latest teacher pass on ``trainer._last_pseudo`` (for --dump-outputs): the trainer's
    own ``_teacher_pass``, its result kept by reference -- no copy, no synchronisation."""
    inner = trainer._teacher_pass

    def teacher_pass(*a, **k):
        trainer._last_pseudo = inner(*a, **k)
        return trainer._last_pseudo
    trainer._teacher_pass = teacher_pass


def dump_outputs(trainer, out_dir):
    """What the last step computed, as ``out_dir/<name>.npy``; call right after the timed steps' final synchronisation,
    before anything else runs on the trainer."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)

    def save(name, t, dtype=np.float32):
        np.save(os.path.join(out_dir, name + ".npy"), t.detach().cpu().double().numpy().astype(dtype))

    # the step's logged device scalars: weighted losses, total_loss, pseudo-label counts, mean teacher confidence
    for k, v in sorted(trainer.storage._pending.items()):
        if isinstance(v, torch.Tensor):
            save(k.replace("/", "."), v.reshape(()), np.float64)
    pseudo = trainer.__dict__.get("_last_pseudo")
    if pseudo is not None:
        count = pseudo.count.long()
        live = torch.arange(pseudo.boxes.shape[1], device=count.device)[None, :] < count[:, None]      # [B, G]
        save("pseudo_count", count)
        save("pseudo_boxes", pseudo.boxes * live[..., None])
        save("pseudo_classes", pseudo.classes * live)
        if pseudo.scores is not None:
            s = pseudo.scores[:, :live.shape[1]]
            save("pseudo_scores", s * live[:, :s.shape[1]])

    def sample(buf, seed):
        """the whole buffer, or DUMP_SAMPLE positions of it drawn by a fixed generator (sorted, the same for every run)"""
        n = buf.numel()
        if n <= DUMP_SAMPLE:
            return buf
        idx = torch.randint(0, n, (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(seed)).sort().values
        return buf[idx.to(buf.device)]

    opt = trainer.optimizer
    save("student_params", sample(opt.flat.param, 0))
    save("student_grad", sample(opt.flat.grad, 0))
    save("student_bn_stats", sample(opt.flat.fbuf, 1))
    teacher = getattr(opt, "teacher", None)
    if teacher is not None:     # same layout as the student's (FusedSGD.attach_teacher): the same positions
        save("teacher_params", sample(teacher.param, 0))
        save("teacher_bn_stats", sample(teacher.fbuf, 1))


def run_steps(trainer, first_iter, n):
    with trainer.step_stream():          # the trainers' own high-priority stream, as in Trainer.train()
        for i in range(n):
            trainer.iter = first_iter + i
            trainer.run_step()
            if STEP_LOG is not None:
                STEP_LOG.after_step(trainer)
            trainer.scheduler.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100, help="timed steps (default: >= 5 s of timed region at N=1)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8, help="images per GPU per step")
    ap.add_argument("--dtype", choices=["bf16x3", "f16x3", "fp32", "bf16"], default=None,
                    help="default: the model's parity-gated mode (vgg: bf16x3, r101: f16x3).  bf16x3: split-precision "
                         "products (3 bf16 MFMAs, ~16-bit operands); fp32: fp32 MFMA; bf16: reduced precision")
    ap.add_argument("--res", choices=["r600", "full"], default="r600")
    ap.add_argument("--model", choices=["vgg", "r101"], default="vgg",
                    help="vgg: the headline VGG16-BN config; r101: r101_c4_..._source_free.yaml (BASELINE config #5)")
    ap.add_argument("--trainer", choices=["source_free", "base"], default="source_free",
                    help="source_free: teacher+student step (BASELINE config #3/#4, the headline); base: source-only "
                         "training step of faster_rcnn_VGG_cityscapes_source_new.yaml (BASELINE config #2)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="skip the reduced-precision (bf16) secondary block")
    ap.add_argument("--no-other-shapes", action="store_true",
                    help="skip the RFULL / one-frame-per-GPU child runs of the default configuration")
    ap.add_argument("--no-smi", action="store_true", help="no rocm-smi clock / power samples beside the run")
    ap.add_argument("--host-frames", action="store_true",
                    help="frames in pinned host memory, uploaded every step on the loader's stream (SFOD.SYNTHETIC.HOST_FRAMES): the "
                         "PCIe-inclusive rate of DESIGN.md section 6 -- never the headline `value`")
    ap.add_argument("--no-planted", action="store_true")
    ap.add_argument("--plant-scale", type=float, default=0.0, help="planted-label mode: scale on cls_score.weight (default: engine/planted.py SCALE)")
    ap.add_argument("--plant-bias", type=float, default=None,
                    help="planted-label mode: use this background bias instead of calibrating it (profiling runs; take it "
                         "from config.planted_labels.background_bias of an unprofiled run of the same configuration)")
    ap.add_argument("--no-kernel-timer", action="store_true")
    ap.add_argument("--opts", nargs="*", default=[], help="extra KEY VALUE config overrides (A/B runs)")
    ap.add_argument("--no-overlap", action="store_true",
                    help="teacher pass on the main stream (SFOD.OVERLAP_TEACHER False)")
    ap.add_argument("--kernel-table", action="store_true", help="stderr: per-shape table of the MFMA kernels (with --full)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: roofline / per-kernel figures, gpu_fill, the other "
                         "precisions and shapes, the CPU baseline, rocm-smi samples, the N > 1 exchange block (the --no-* "
                         "options switch parts of it off)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (losses, pseudo labels, a fixed sample "
                         "of the student / teacher parameters and the student gradient)")
    args = ap.parse_args()
    if args.dtype is None:
        args.dtype = PARITY_DTYPE[args.model]
    if args.kernel_table and not args.full:
        ap.error("--kernel-table needs --full")
    t_start = time.perf_counter()

    def note(msg):      # progress on stderr (the JSON line is the only thing on stdout)
        print(f"[bench +{time.perf_counter() - t_start:6.1f}s] {msg}", file=sys.stderr, flush=True)

    # N > 1 without a launcher: start the N ranks as a child job -- BEFORE torch / HIP are touched in this process
    lm = _launcher()
    if args.gpus > 1 and not lm.under_launcher():
        sys.exit(lm.launch(os.path.abspath(__file__), sys.argv[1:], args.gpus))

    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the launcher started {world} rank(s)")
    # SFOD_BENCH_ONE_GPU=1 (tests/test_gpu_two_rank.py only): the N ranks share cuda:0 and exchange over gloo -- RCCL refuses
    # two ranks on one device -- so that every N > 1 line of this file executes on a one-GPU box.  Such a line says so
    # ("test_hook") and is never a measurement.
    one_gpu = world > 1 and os.environ.get("SFOD_BENCH_ONE_GPU") == "1"
    if one_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    telemetry = _by_path("sfod_telemetry", "telemetry.py")
    rccl_log = None
    if world > 1:
        if one_gpu:
            dist.init_process_group("gloo")
        else:
            # --full: RCCL's INFO lines (INIT / GRAPH / TUNING) of every rank go to a per-rank file: rank 0's is summarised
            # in the line (algorithm / protocol per payload, channels, transports) so that a scaling run explains itself
            if args.full:
                rccl_log = telemetry.rccl_debug_setup(rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    # --full: clocks and package power of every GPU of the node beside the run (rank 0: a host thread running rocm-smi)
    smi = (telemetry.SmiSampler().start() if args.full and rank == 0 and not args.no_smi and not telemetry.under_profiler()
           else None)

    note("torch imported")
    sfod = importlib.import_module("simple-sfod_amd")
    sfod.native.load()
    cfg, trainer = build_trainer(sfod, args, args.dtype, world, rank, local_rank)   # N > 1: the ctor broadcasts rank 0's state

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    note("trainer built")
    planted = None
    global STEP_LOG
    if args.trainer != "base" and not args.no_planted:
        planted = sfod.engine.planted.plant_labels(trainer, args.plant_scale if args.plant_scale else
                                                   sfod.engine.planted.SCALE[args.model], note=note, bias=args.plant_bias)
        if world > 1:       # every rank calibrated on its own shard: take rank 0's bias everywhere (one broadcast, untimed)
            bp = trainer.model.roi_heads.box_predictor
            with torch.no_grad():
                dist.broadcast(bp.cls_score.bias, 0)
                trainer._copy_main_model()
    STEP_LOG = StepLog()
    if args.dump_outputs and args.trainer != "base":
        record_pseudo_labels(trainer)
    run_steps(trainer, 0, args.warmup)
    # --full: per-kernel HIP-event timing is only meaningful when kernels do not share the GPU: with
    # SFOD.OVERLAP_TEACHER the teacher pass runs on a second stream beside the student's forward, so the
    # roofline figures come from a short single-stream segment AFTER the timed region (same model, same
    # shapes, same kernels); without overlap they are measured inside the timed region itself.
    overlapped = bool(cfg.SFOD.OVERLAP_TEACHER) and not args.no_overlap and args.trainer != "base"
    kernel_timer = args.full and not args.no_kernel_timer
    timer = None
    if kernel_timer and not overlapped:
        timer = sfod.native.KernelTimer()
        sfod.native.set_timer(timer)
    sync()
    t0 = time.perf_counter()
    run_steps(trainer, args.warmup, args.steps)
    sync()
    elapsed = time.perf_counter() - t0
    sfod.native.set_timer(None)
    if args.dump_outputs and rank == 0:
        dump_outputs(trainer, args.dump_outputs)
        note(f"outputs of the last timed step written to {args.dump_outputs}")
    step_log, STEP_LOG = STEP_LOG, None        # warm-up + timed steps; the measurement segments below are not logged
    rl_steps, rl_elapsed, rl_segment = args.steps, elapsed, "the timed region"
    if kernel_timer and overlapped:
        rl_steps = max(1, min(5, args.steps))
        trainer.overlap_teacher = False
        bbs = [m.backbone for m in (trainer.model, getattr(trainer, "model_teacher", None)) if m is not None]
        ws_saved = [getattr(b, "wgrad_stream", None) for b in bbs]
        for b in bbs:                       # (ResNet: the backward's weight gradients run on a side stream otherwise)
            if hasattr(b, "wgrad_stream"):
                b.wgrad_stream = False
        run_steps(trainer, args.warmup + args.steps, 1)   # one untimed step to settle the allocator in this mode
        timer = sfod.native.KernelTimer()
        sfod.native.set_timer(timer)
        sync()
        t1 = time.perf_counter()
        run_steps(trainer, args.warmup + args.steps + 1, rl_steps)
        sync()
        rl_elapsed = time.perf_counter() - t1
        sfod.native.set_timer(None)
        trainer.overlap_teacher = None
        for b, w in zip(bbs, ws_saved):
            if w is not None:
                b.wgrad_stream = w
        rl_segment = (f"{rl_steps} single-stream steps after the timed region ({1000.0 * rl_elapsed / rl_steps:.2f} ms/step): "
                      "the timed steps run the teacher on a second stream, where a kernel's event duration includes "
                      "time shared with concurrent kernels")
    # ---- is the GPU waiting for the host?  Un-profiled, on single-stream steps: (a) how long the host needs to ENQUEUE a
    # step (no synchronisation inside) against how long the GPU needs to run it, (b) HIP events around EVERY call into the
    # library: the share of the step's wall time its own launches cover -- the rest is torch's small kernels
    # (tools/profile_torch_ops.py lists them) plus idle gaps.  N = 1 only.
    gpu_fill = None
    if world == 1 and kernel_timer:
        n_id = max(1, min(5, args.steps))
        trainer.overlap_teacher = False
        bbs = [m.backbone for m in (trainer.model, getattr(trainer, "model_teacher", None)) if m is not None]
        ws_saved = [getattr(b, "wgrad_stream", None) for b in bbs]
        for b in bbs:
            if hasattr(b, "wgrad_stream"):
                b.wgrad_stream = False
        run_steps(trainer, args.warmup + args.steps + 20, 1)
        sync()
        in_flight = getattr(trainer, "_max_in_flight", int(cfg.SFOD.MAX_STEPS_IN_FLIGHT))
        trainer._max_in_flight = 0                                     # (the steps-in-flight bound would make the host wait)
        trainer.__dict__.get("_step_events", []).clear()
        th0 = time.perf_counter()
        run_steps(trainer, args.warmup + args.steps + 21, n_id)
        host_ms = (time.perf_counter() - th0) * 1000.0 / n_id          # enqueue only: the queue is drained afterwards
        sync()
        trainer._max_in_flight = in_flight
        allk = sfod.native.KernelTimer(watch=None)
        sfod.native.set_timer(allk)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        e0.record()
        run_steps(trainer, args.warmup + args.steps + 30, n_id)
        e1.record()
        sync()
        sfod.native.set_timer(None)
        span_ms = e0.elapsed_time(e1) / n_id
        summ_all = allk.summary()
        native_ms = sum(v["ms"] for v in summ_all.values()) / n_id
        gpu_fill = {"steps": n_id, "gpu_ms_per_step_single_stream": round(span_ms, 3),
                    "host_enqueue_ms_per_step": round(host_ms, 3),
                    "native_kernel_ms_per_step": round(native_ms, 3),
                    "native_launches_per_step": sum(v["launches"] for v in summ_all.values()) // n_id,
                    "not_in_native_kernels_frac": round(max(0.0, 1.0 - native_ms / span_ms), 4),
                    "note": "HIP events around every call into libsfod_hip.so on single-stream steps (with the events the "
                            "step itself runs a few % slower); what the library's launches do not cover = torch's small "
                            "kernels + idle gaps.  host_enqueue < gpu time: the host runs ahead, the GPU is never waiting "
                            "for a launch"}
        trainer.overlap_teacher = None
        for b, w_ in zip(bbs, ws_saved):
            if w_ is not None:
                b.wgrad_stream = w_
    t_region = (t0, t0 + elapsed)
    if smi is not None:
        smi.stop()
    per_rank = None
    if world > 1:
        mine = torch.tensor([elapsed], device="cuda")
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        every = [e.item() for e in every]
        elapsed = max(every)                                  # the contract's time: MAX over ranks
        ms = [1000.0 * e / args.steps for e in every]
        per_rank = {"ms_per_step": [round(m, 3) for m in ms], "ms_per_step_min": round(min(ms), 3),
                    "ms_per_step_max": round(max(ms), 3), "slowest_rank": ms.index(max(ms))}
    rec = trainer.storage.flush()
    note(f"timed region done: {elapsed:.2f} s")

    # ---- N > 1, --full: what the exchange step costs (the flat-gradient all-reduce alone; the step without any exchange) ----
    comm = None
    if world > 1 and args.full:
        flat = trainer.optimizer.flat
        for _ in range(3):
            dist.all_reduce(flat.grad)
        sync()
        tc = time.perf_counter()
        for _ in range(10):
            dist.all_reduce(flat.grad)
        sync()
        ar_ms = (time.perf_counter() - tc) * 100.0
        # the same steps with the exchange switched off (timing only: the ranks' weights diverge from here on)
        red, trainer._reducer = trainer._reducer, None
        bb = trainer.model.backbone
        hooks = (getattr(bb, "_pre_backward", None), getattr(bb, "_mid_backward", None))
        bb._pre_backward = bb._mid_backward = None
        trainer._reduce_gradients = lambda: None
        nc = max(5, min(20, args.steps))
        run_steps(trainer, args.warmup + args.steps + 10, 2)
        sync()
        tn = time.perf_counter()
        run_steps(trainer, args.warmup + args.steps + 12, nc)
        sync()
        nocomm_ms = (time.perf_counter() - tn) * 1000.0 / nc
        # what each phase exposes: the same steps with only the early (heads) phase, then early + mid (trunk) -- the
        # differences to the exchange-free step and to the full step are the phases' exposed times
        per_phase = {}
        if red is not None:
            trainer._reducer = red
            bb._pre_backward, bb._mid_backward = hooks
            del trainer._reduce_gradients              # back to the class's method
            for tag, ph in (("early", ("early",)), ("early_mid", ("early", "mid"))):
                red.phases = ph
                run_steps(trainer, args.warmup + args.steps + 40, 2)
                sync()
                tp = time.perf_counter()
                run_steps(trainer, args.warmup + args.steps + 42, nc)
                sync()
                per_phase[tag] = (time.perf_counter() - tp) * 1000.0 / nc
            red.phases = ("early", "mid", "final")
        t = torch.tensor([ar_ms, nocomm_ms, per_phase.get("early", 0.0), per_phase.get("early_mid", 0.0)], device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        ar_ms, nocomm_ms, early_ms, early_mid_ms = t.tolist()
        nbytes = flat.grad.numel() * 4
        step_ms = 1000.0 * elapsed / args.steps
        comm = {"collective": "sum all-reduce of the flat fp32 student gradient, 3 phases overlapping the backbone backward "
                              "(engine/trainer.py::GradientReducer)",
                "backend": ("gloo (SFOD_BENCH_ONE_GPU test hook)" if one_gpu else
                            "RCCL " + ".".join(str(v) for v in torch.cuda.nccl.version())),
                "payload_MB": round(nbytes / 1e6, 1), "allreduce_alone_ms": round(ar_ms, 3),
                "allreduce_bus_GBps": round(2.0 * (world - 1) / world * nbytes / (ar_ms * 1e-3) / 1e9, 1),
                "step_without_exchange_ms": round(nocomm_ms, 3),
                "exposed_exchange_ms_per_step": round(max(0.0, step_ms - nocomm_ms), 3),
                "exposed_ms_per_phase": ({"heads_slice_async": round(max(0.0, early_ms - nocomm_ms), 3),
                                          "trunk_slice_async": round(max(0.0, early_mid_ms - early_ms), 3),
                                          "final_slice_blocking": round(max(0.0, step_ms - early_mid_ms), 3),
                                          "slices_MB": [round(4e-6 * (red.hi - red.lo), 1), round(4e-6 * (red.mhi - red.mlo), 1),
                                                        round(4e-6 * red.final_elements(), 2)]}
                                         if red is not None else None),
                "overlap_fraction": round(min(1.0, max(0.0, 1.0 - max(0.0, step_ms - nocomm_ms) / max(ar_ms, 1e-9))), 3)}

    # ---- secondary block: the reduced-precision mode, same shapes, in a CHILD process started now (a second trainer in
    # this process measured 27 % low -- allocator / stream state left by the first one -- so it gets a clean process;
    # starting a child is fine, replacing this process would not be).  N = 1 only; never `value`. ------------------
    secondary = None
    SECONDARY_NOTE = {
        "bf16": "one bf16 MFMA pass per product, bf16 activations: NOT a parity mode (losses within a few % of the oracle, "
                "tests/test_gpu_model.py::test_student_bf16_mode_tracks_the_fp32_oracle)",
        "bf16x3": "split-precision products (3 bf16 MFMAs, ~16-bit operands): NOT a parity mode on this 101-layer network "
                  "(RPN logits 1.7e-3, loss_box_reg 3.7e-4 vs the oracle where fp32 holds 1e-4; tracking gates in "
                  "tests/test_gpu_fullsize.py::test_r101_yaml_teacher_and_student_at_600x1200[bf16x3])",
        "f16x3": "PARITY mode (tighter than the headline's): forward operands as IEEE half pairs (22 bits), gated like fp32 by "
                 "tests/test_gpu_fullsize.py (intermediates within 2e-5 on this config)",
        "fp32": "PARITY mode: exact fp32 FMA chains on v_mfma_f32_32x32x2_f32 (1/16 of the bf16 rate)"}
    faster = {"fp32": ["bf16x3", "bf16"] if args.model == "r101" else ["bf16"], "bf16x3": ["bf16"], "bf16": [],
              "f16x3": ["bf16x3", "bf16"] if args.model == "r101" else ["bf16"]}[args.dtype]
    others = OTHER_PARITY.get(args.model, {}).get(args.dtype, []) if args.trainer != "base" or args.model == "vgg" else []
    other_modes = []
    if args.full and not args.no_secondary and (faster or others) and world == 1:
        import subprocess
        n2 = max(5, min(40, args.steps))
        secondary = []
        for dt2 in list(faster) + list(others):
            # fp32 runs at 1/16 of the matrix rate: fewer steps keep the default run within its few minutes
            n_dt = max(5, n2 // 3) if dt2 == "fp32" else n2
            cmd = [sys.executable, os.path.abspath(__file__), "--dtype", dt2, "--steps", str(n_dt), "--warmup", "3" if dt2 == "fp32" else "5",
                   "--batch", str(args.batch), "--res", args.res, "--model", args.model, "--trainer", args.trainer,
                   "--no-cpu-baseline", "--no-secondary", "--no-kernel-timer", "--no-smi"]
            cmd += (["--no-planted"] if args.no_planted else []) + (["--no-overlap"] if args.no_overlap else [])
            cmd += ["--plant-scale", str(args.plant_scale)] if args.plant_scale else []
            cmd += ["--plant-bias", str(args.plant_bias)] if args.plant_bias is not None else []
            cmd += (["--opts"] + list(args.opts)) if args.opts else []
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=600, check=True)
                d2 = json.loads(r.stdout.decode().strip().splitlines()[-1])
                (other_modes if dt2 in others else secondary).append(
                    {"dtype": dt2, "value": d2["value"], "unit": "images/s", "steps": d2["steps"],
                     "ms_per_step": d2["ms_per_step"],
                     "note": SECONDARY_NOTE[dt2] + "; measured by a child process of this run, reported for reference only"})
            except Exception as e:      # the secondary block must never take the headline down with it
                (other_modes if dt2 in others else secondary).append({"dtype": dt2, "error": repr(e)[:200]})
        if len(secondary) == 1:
            secondary = secondary[0]
        elif not secondary:
            secondary = None
        note("secondary block done")
    # ---- the other shapes BASELINE.md section 3 names for this config (R600 AND RFULL, B = 1 AND B = 8 per GPU), measured by
    # child processes of the --full run like the other modes: 1024x2048 network tensors at B = 8, and the yaml's literal
    # one frame per GPU (IMS_PER_BATCH_TARGET 1, reference yaml :33-46).  Same arithmetic mode, same planted head recipe.
    other_shapes = None
    if (args.full and not args.no_secondary and not args.no_other_shapes and world == 1 and args.res == "r600"
            and args.batch == 8 and args.trainer != "base" and not args.opts):
        import subprocess
        other_shapes = []
        for label, extra in (("one frame per GPU (the yaml's IMS_PER_BATCH_TARGET 1), 600x1200 tensors",
                              ["--batch", "1", "--res", "r600", "--steps", "120", "--warmup", "10"]),
                             ("B = 8 per GPU, 1024x2048 network tensors (INPUT.MIN_SIZE_TRAIN (1024,), MAX 2048)",
                              ["--batch", "8", "--res", "full", "--steps", "12", "--warmup", "3"]),
                             # the PCIe-inclusive rate of the headline configuration
                             ("this line's configuration with the frames in pinned HOST memory, each uploaded over PCIe every step "
                              "(the reference's hand-over: CPU uint8 tensors)",
                              ["--batch", "8", "--res", "r600", "--steps", str(args.steps), "--warmup", "5", "--host-frames"]),
                             )[:3 if args.model == "vgg" else 1]:
            # (--full for the child's clock / power samples: everything else of it is switched off)
            cmd = [sys.executable, os.path.abspath(__file__), "--dtype", args.dtype, "--model", args.model, "--trainer", args.trainer,
                   "--full", "--no-cpu-baseline", "--no-secondary", "--no-kernel-timer"] + extra
            cmd += (["--no-planted"] if args.no_planted else [])
            cmd += ["--plant-scale", str(args.plant_scale)] if args.plant_scale else []
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=600, check=True)
                d2 = json.loads(r.stdout.decode().strip().splitlines()[-1])
                c2 = d2["config"]
                other_shapes.append({"shape": label, "dtype": d2["dtype"], "value": d2["value"], "unit": "images/s",
                                     "batch_per_gpu": c2["batch_per_gpu"], "steps": d2["steps"], "warmup": d2["warmup"],
                                     "ms_per_step": d2["ms_per_step"], "step_tflops_per_gpu": d2["step_tflops_per_gpu"],
                                     "peak_hbm_reserved_GB": c2["peak_hbm_reserved_GB"],
                                     "peak_hbm_allocated_GB": c2["peak_hbm_allocated_GB"],
                                     "pseudo_labels_per_image": c2.get("pseudo_labels_per_image", {}).get("mean"),
                                     "gpu_telemetry": d2.get("gpu_telemetry", {}).get("cards"),
                                     "note": "measured by a child process of this run (same mode, same planted-head recipe); "
                                             "never `value`"})
            except Exception as e:
                other_shapes.append({"shape": label, "error": repr(e)[:200]})
        note("other shapes done")
    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return
    images = args.batch * world * args.steps
    value = images / elapsed
    h, w = (600, 1200) if args.res == "r600" else (1024, 2048)
    sflops = step_flops(args.res, args.model, args.trainer)
    yaml = YAML["vgg_base"] if args.trainer == "base" else YAML[args.model]
    what = ("source-only training step (student fwd/bwd + SGD)" if args.trainer == "base" else
            "teacher+student (teacher fwd + NMS pseudo-labels + student fwd/bwd + SGD + EMA)")
    out = {
        "metric": "teacher+student train images/s on 1024x2048 synthetic" if args.trainer != "base"
                  else "source-only train images/s on 1024x2048 synthetic (BASELINE config #2)",
        "value": round(value, 3), "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(1000.0 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "dtype_note": {
            "bf16x3": ("split precision: operands as (hi, lo) bf16 pairs (~16 significand bits each), hi*hi + hi*lo + lo*hi on "
                       "v_mfma_f32_16x16x32_bf16 / 32x32x16_bf16 with fp32 accumulation; fp32 activations / statistics / losses.  Gated at "
                       "600x1200 by tests/test_gpu_fullsize.py: " +
                       ("losses and decoded boxes within 1e-4 of the CPU oracle, intermediates (RPN logits / deltas, box "
                        "scores / deltas) within 2e-4 (measured 6e-5 .. 1e-4), every discrete decision bit-exact"
                        if args.model == "vgg" else
                        "on this 101-layer network only ~1e-3 (tracking gates) -- f16x3 and fp32 are this config's parity modes")),
            "fp32": "v_mfma_f32_32x32x2_f32 (exact fp32 FMA chains); losses and decoded boxes within 1e-4 of the CPU oracle at "
                    "600x1200 (tests/test_gpu_fullsize.py), intermediates within 3x the reference arithmetic's own fp32-vs-fp64 "
                    "error on the network",
            "f16x3": "split precision with IEEE half pairs in the FORWARD products (22-bit operands, weights under a per-tensor "
                     "power-of-two scale; v_mfma_f32_32x32x16_f16 x 3, fp32 accumulation) and bf16 pairs in the backward "
                     "products; gated like fp32 at 600x1200 by tests/test_gpu_fullsize.py on both yamls (losses / boxes 1e-4, "
                     "intermediates 2e-5 or 3x the reference arithmetic's own fp32-vs-fp64 error), discrete steps bit-exact",
            "bf16": "reduced precision, not a parity mode"}[args.dtype],
        "timed_region_s": round(elapsed, 3),
        "config": {
            "workload": f"{yaml}: {'VGG16-BN' if args.model == 'vgg' or args.trainer == 'base' else 'ResNet-101-C4'} {what}, "
                        "synthetic 1024x2048 8-class "
                        f"frames -> {h}x{w} network tensors ({'INPUT.MIN_SIZE_TRAIN=600 of the config' if args.res == 'r600' else 'MIN_SIZE_TRAIN overridden to 1024'})",
            "batch_per_gpu": args.batch, "global_batch": args.batch * world, "parallelism": f"dp{world}",
            "ema": bool(cfg.SFOD.EMA.ENABLED) and args.trainer != "base", "teacher_on_second_stream": overlapped,
            "input_pipeline": (("uint8 1024x2048 frames in PINNED HOST memory, each uploaded over PCIe on the loader's stream every "
                                "step (--host-frames: the PCIe-inclusive rate, not the headline)"
                                if args.host_frames and args.res == "r600" else "uint8 1024x2048 frames resident in HBM") +
                               "; ResizeShortestEdge (Pillow-exact bilinear) + "
                               "RandomFlip on the device every step, prefetched one batch ahead on a loader stream"
                               if bool(cfg.SFOD.SYNTHETIC.DEVICE_RESIZE) else
                               "frames resized once at start-up (Pillow), RandomFlip on the device every step"), "elide_zero_weight_branches": bool(cfg.SFOD.ELIDE_DEAD_BRANCHES),
            "planted_labels": planted if planted is not None else False,
            **(step_log.summary() if step_log is not None and args.trainer != "base" else {}),
            "max_steps_in_flight": int(cfg.SFOD.MAX_STEPS_IN_FLIGHT), "deterministic": bool(cfg.SFOD.DETERMINISTIC),
            "algorithmic_tflop_per_image": round(sflops / 1e12, 3),
            # torch's caching allocator on this rank (the library allocates nothing itself): what the step holds of the 288 GB
            "peak_hbm_reserved_GB": round(torch.cuda.max_memory_reserved() / 1e9, 1),
            "peak_hbm_allocated_GB": round(torch.cuda.max_memory_allocated() / 1e9, 1),
        },
        "step_tflops_per_gpu": round(sflops * value / world / 1e12, 2),
        "losses": {k: round(v, 5) for k, v in rec.items() if k.startswith("loss") or k.startswith("roi_head")},
    }
    if planted is not None:
        # the student is trained on 10-30 pseudo labels per image with an O(1) classification loss --
        # a bench line whose workload is not that is not printed.  The check is made on the first CHECK_WINDOW logged steps
        # (warm-up + timed; the default run and the driver's short runs lie inside it entirely): that is what the planted
        # head is calibrated for.  Over hundreds of further steps the count is training dynamics (the student learns the
        # labels, the EMA teacher follows: reduced-precision bf16 drifts to ~9 per image by step 300, bf16x3 reaches zero
        # around step 1000: the confirmation-bias collapse of self-training from random weights) -- reported for the whole
        # run in ``config`` beside the window's figures.
        win = step_log.summary(first=CHECK_WINDOW)
        pl, lc = win.get("pseudo_labels_per_image"), win.get("loss_cls_pseudo")
        assert pl is not None and sfod.engine.planted.RANGE[0] <= pl["mean"] <= sfod.engine.planted.RANGE[1], f"pseudo labels per image {pl}"
        assert lc is not None and 0.0 < lc["max"] < 5.0, f"loss_cls_pseudo {lc}"
        out["config"]["workload_check"] = {"window_steps": pl["steps"], "pseudo_labels_per_image": pl, "loss_cls_pseudo": lc,
                                           "rule": f"mean count in {list(sfod.engine.planted.RANGE)}, max loss < 5 over the first "
                                                   f"{CHECK_WINDOW} logged steps (the whole run's figures are beside it in "
                                                   "config: self-training on random weights loses its pseudo labels after "
                                                   "several hundred steps -- 1500 steps: mean 4.7, none at the end; the "
                                                   "step's kernels and shapes do not depend on the count)"}
    if gpu_fill is not None:
        out["gpu_fill"] = gpu_fill
    if comm is not None:
        comm["rccl"] = telemetry.rccl_summary(rccl_log)       # None under the gloo test hook / when the log is elsewhere
        out["exchange"] = comm
    if per_rank is not None:
        out["per_rank"] = per_rank
    if smi is not None:
        tel = smi.summary(*t_region)
        if tel is not None:
            out["gpu_telemetry"] = {"during": "the timed region", "source": "rocm-smi --showpower --showclocks, sampled "
                                    f"every {smi.interval} s by a host thread of rank 0", "cards": tel}
    if one_gpu:
        out["test_hook"] = "SFOD_BENCH_ONE_GPU: all ranks on cuda:0 over gloo -- exercises the N > 1 code path, not a measurement"
    if secondary is not None:
        out["reduced_precision_mode"] = secondary
    if other_modes:
        out["other_parity_modes"] = other_modes
    if other_shapes:
        out["other_shapes"] = other_shapes
    if timer is not None:
        summ = timer.summary()
        if args.kernel_table:
            agg = {}
            for name, flops, a, b in timer.records:
                d = agg.setdefault((name, round(flops / 1e9, 2)), [0, 0.0])
                d[0] += 1
                d[1] += a.elapsed_time(b)
            for (name, gf), (n, ms) in sorted(agg.items(), key=lambda kv: -kv[1][1]):
                print(f"{name:18s} {gf:10.2f} GF/launch  x{n:4d}  {ms / n:8.3f} ms  {gf / (ms / n):8.1f} TF/s  "
                      f"{100 * ms / (1000 * rl_elapsed):5.1f}% of step", file=sys.stderr)
        # the dominant kernel family = the one with the larger share of the step (VGG16: the halo-patch 3x3 kernel;
        # ResNet-101-C4: the generic GEMM behind its 1x1 convolutions and the box head's linear layers)
        cands = [k_ for k_ in ("sfod_conv_fwd:patch3x3", "sfod_conv_fwd:gemm") if k_ in summ]
        key = max(cands, key=lambda k_: summ[k_]["ms"]) if cands else "sfod_conv_fwd:gemm"
        k = summ.get(key, {"ms": 0.0, "flops": 0.0, "launches": 0})
        ach = k["flops"] / (k["ms"] * 1e-3) / 1e12 if k["ms"] > 0 else 0.0
        kname = ("k_conv3x3_patch / k_conv3x3_m16 (halo-patch MFMA conv3x3 fwd + dgrad; operand pairs: the 256 x 128 shape on "
                 "v_mfma_f32_16x16x32, the 64-channel shape on 32x32x16)" if key.endswith("patch3x3")
                 else "k_conv_fwd (MFMA implicit GEMM)")
        out["roofline"] = {
            "kernel": kname,
            "bound": "mfma", "achieved": round(ach, 2), "peak": PEAK[args.dtype], "unit": "TFLOP/s",
            "frac": round(ach / PEAK[args.dtype], 4),
            # bf16x3: `frac` is matrix-pipe utilisation (3 MFMAs per algorithmic product, peak = 2500 / 3); per ALGORITHMIC
            # FLOP the same measurement is this fraction of the dense bf16 peak -- useful work, not pipe occupancy
            "frac_of_bf16_peak_algorithmic": round(ach / PEAK["bf16"], 4),
            # HBM bytes per launch from the committed PMC passes of THIS mode's kernel (tools/pmc_hbm_run.sh); null otherwise
            # only when THIS run is the configuration the counters were captured on (else null)
            "traffic": ((pmc_traffic(args.model, ("k_conv3x3_patch<", "k_conv3x3_m16<"),
                                     {"bf16x3": ("float, true", "float, 1,", "m16<8, 4, 1,", "m16<4, 8, 1,"),
                                      "f16x3": ("float, 2,", "m16<8, 4, 2,", "m16<4, 8, 2,"),
                                      "bf16": ("__bf16, false", "__bf16, 0,")}.get(args.dtype, "-"))
                         if key.endswith("patch3x3") else
                         pmc_traffic(args.model, "k_conv_fwd<", {"bf16x3": (", 1, 64>", ", 1, 128>"), "f16x3": (", 2, 64>", ", 2, 128>")}.get(args.dtype, "-")))
                        if pmc_matches(args) else None),
            # what the traffic figure says, in words (DESIGN.md section 6 / profiles/HISTORY.md round 3): writes = algorithmic; the
            # halo-patch kernel READS ~2x its algorithmic bytes -- the two 64-byte halves of a 128-byte line are fetched a K-body
            # apart and the line leaves L2 in between (real double fetching, sized at ~8 W; not fixed)
            "traffic_note": ("reads ~2x algorithmic (both halves of a line fetched a K-body apart); writes = algorithmic"
                             if key.endswith("patch3x3") else "see DESIGN.md section 6"),
            "launches_per_step": k["launches"] // max(rl_steps, 1),
            "avg_launch_ms": round(k["ms"] / max(k["launches"], 1), 4),
            "algorithmic_gflop_per_launch": round(k["flops"] / max(k["launches"], 1) / 1e9, 3),
            "share_of_step_time": round(k["ms"] / (1000.0 * rl_elapsed), 4),
            "measured_over": rl_segment,
        }
        g = summ.get("sfod_conv_fwd:gemm")
        if g and g["ms"] > 0 and key.endswith("patch3x3"):
            out["roofline_gemm"] = {"kernel": "k_conv_fwd (generic implicit GEMM: 1x1 / linear / first layer)",
                                    "achieved": round(g["flops"] / (g["ms"] * 1e-3) / 1e12, 2), "peak": PEAK[args.dtype],
                                    "unit": "TFLOP/s", "frac": round(g["flops"] / (g["ms"] * 1e-3) / 1e12 / PEAK[args.dtype], 4),
                                    "share_of_step_time": round(g["ms"] / (1000.0 * rl_elapsed), 4)}
        p3 = summ.get("sfod_conv_fwd:patch3x3")
        if p3 and p3["ms"] > 0 and key.endswith("gemm"):
            out["roofline_patch3x3"] = {"kernel": "k_conv3x3_patch (halo-patch MFMA conv3x3 fwd + dgrad)",
                                        "achieved": round(p3["flops"] / (p3["ms"] * 1e-3) / 1e12, 2), "peak": PEAK[args.dtype],
                                        "unit": "TFLOP/s",
                                        "frac": round(p3["flops"] / (p3["ms"] * 1e-3) / 1e12 / PEAK[args.dtype], 4),
                                        "share_of_step_time": round(p3["ms"] / (1000.0 * rl_elapsed), 4)}
        wk = {k2: sum(summ[n][k2] for n in ("sfod_conv_wgrad", "sfod_conv_wgrad_oihw") if n in summ)
              for k2 in ("launches", "ms", "flops")}
        if wk["ms"] > 0:
            out["roofline_wgrad"] = {"kernel": "k_conv_wgrad", "achieved": round(wk["flops"] / (wk["ms"] * 1e-3) / 1e12, 2),
                                     "peak": PEAK[args.dtype], "unit": "TFLOP/s",
                                     "frac": round(wk["flops"] / (wk["ms"] * 1e-3) / 1e12 / PEAK[args.dtype], 4),
                                     "share_of_step_time": round(wk["ms"] / (1000.0 * rl_elapsed), 4)}
    if args.full and world == 1 and not args.no_cpu_baseline and args.trainer != "base":
        note("cpu baseline ...")
        out["cpu_baseline"] = cpu_baseline(args.res, planted, args.model)
    note("done")
    print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
