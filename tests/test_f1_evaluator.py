"""F1Evaluator on the host (no GPU): the numpy rule against the reference's recorded counts (tests/golden/f1_ref.npz, written by
tools/record_f1_golden.py), the hand cases of tests/helpers/f1_cases.py, the ``process`` protocol against ``detector_postprocess``,
``DatasetEvaluators``, ``SFOD.EVALUATORS`` through ``BaseTrainer.test``, two gloo ranks, and the C entry point's refusals."""
import importlib
import multiprocessing as mp
import os
import sys
import threading

import numpy as np
import pytest
import torch
import torch.distributed as dist

from helpers import f1_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOT = os.path.join(ROOT, "configs", "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free.yaml")
GOLDEN = os.path.join(ROOT, "tests", "golden", "f1_ref.npz")
SMALL = ["MODEL.DEVICE", "cpu", "SFOD.SYNTHETIC.HEIGHT", "64", "SFOD.SYNTHETIC.WIDTH", "128", "INPUT.MIN_SIZE_TEST", "32",
         "DATASETS.TEST", "('synthetic_cityscapes_foggy_val',)"]


def _batched(sfod, ev, a):
    t = {k: torch.from_numpy(v) for k, v in a.items()}
    ev.process_batched(t["det_boxes"], t["det_scores"], t["det_classes"], t["det_count"],
                       sfod.modeling.batched.BatchedGT(t["gt_boxes"], t["gt_classes"], t["gt_count"], None), t["scale"], t["clip_size"])


@pytest.fixture(scope="module")
def fixture():
    z = np.load(GOLDEN)
    return z, C.fixture_images(z)


def test_fixture_holds_what_the_recorder_promises(fixture):
    z, imgs = fixture
    assert z["params"].tolist() == [[0.5, 5, 0.5], [0.3, 100, 0.05], [0.75, 1, 0.9]]
    assert len(imgs) >= 200 and os.path.getsize(GOLDEN) < 512 * 1024
    assert set(z["K"].tolist()) == set(range(1, 9)) and min(z["nd"]) == 0 and min(z["ng"]) == 0
    assert any(n == 100 and g == 100 for n, g in zip(z["nd"], z["ng"]))
    for _, db, ds, _, gb, _, _ in imgs:
        assert len(set(ds.tolist())) == len(ds) and np.isfinite(db).all() and np.isfinite(gb).all()
    assert (z["counts"].sum(axis=(1, 2)) > 0).all()           # every parameter set has TP, FP and FN


@pytest.mark.parametrize("p", [0, 1, 2])
def test_host_rule_equals_the_reference_per_image_and_in_total(sfod, fixture, p):
    z, imgs = fixture
    iou, top_n, score = z["params"][p]
    whole = sfod.evaluation.F1Evaluator(8, iou, int(top_n), score)
    for i, img in enumerate(imgs):
        ev = sfod.evaluation.F1Evaluator(img[0], iou, int(top_n), score)
        before = ev.accumulated()
        _batched(sfod, ev, C.pack_arrays([img], max(len(img[2]), 1), max(len(img[5]), 1)))
        assert (ev.accumulated() - before == z["counts"][p, i, :img[0]]).all(), (p, i)
    for i in range(0, len(imgs), 16):
        _batched(sfod, whole, C.pack_arrays(imgs[i:i + 16]))
    res = whole.evaluate()
    assert list(res) == ["F1 Score"] and isinstance(res["F1 Score"], float) and res["F1 Score"] == float(z["f1"][p])
    assert whole.counts.shape == (8, 3) and whole.counts.dtype == np.int64


@pytest.mark.parametrize("case", C.HAND_CASES, ids=[c["name"] for c in C.HAND_CASES])
def test_hand_cases(sfod, case):
    for poison in (False, True):                     # padding beyond the counts, filled with boxes that would match
        ev = sfod.evaluation.F1Evaluator(case["K"], *case["params"])
        _batched(sfod, ev, C.pack(case["images"], 7, 5, poison=poison))
        assert ev.accumulated().tolist() == case["counts"], poison


def test_evaluate_arithmetic_and_reset(sfod):
    ev = sfod.evaluation.F1Evaluator(2)
    assert (ev.class_number, ev.iou, ev.top_n, ev.score) == (2, 0.5, 5, 0.5)
    assert ev.evaluate() == {"F1 Score": 0}                                 # nothing seen: p + r == 0
    ev._host += np.array([[3, 1, 0], [0, 0, 2]])                            # TP 3, FP 1, FN 2: p = 3/4, r = 3/5
    assert ev.evaluate() == {"F1 Score": 2 * (0.75 * 0.6) / (0.75 + 0.6)}
    assert ev.counts.tolist() == [[3, 1, 0], [0, 0, 2]]
    ev.reset()
    assert ev.evaluate() == {"F1 Score": 0} and not ev.counts.any()


def _echo_outputs(sfod, batch, factor_of=lambda d: d["width"] / d["image"].shape[2]):
    """detections = the ground truth with a few of them shifted, at the frame's native size (as the model returns them)"""
    S = sfod.structures
    outs = []
    for d in batch:
        inst = S.Instances((d["height"], d["width"]))
        boxes = d["instances"].gt_boxes.tensor.clone()
        boxes[::3, 0] += 3.3                                               # some IoUs fall below 1, some below 0.5
        boxes[1::3, 2] -= 0.45 * (boxes[1::3, 2] - boxes[1::3, 0])
        inst.pred_boxes = S.Boxes(boxes * factor_of(d))
        inst.scores = torch.linspace(0.95, 0.35, len(boxes))
        inst.pred_classes = d["instances"].gt_classes
        outs.append({"instances": inst})
    return outs


def test_process_equals_detector_postprocess_then_process_batched_at_scale_one(sfod):
    """dicts with Instances at a native size different from the input size: ``process`` (scale and clip inside the rule) against
    the project's ``detector_postprocess`` to the input size followed by ``process_batched`` at scale 1"""
    cfg = sfod.config.setup_cfg(HOT, SMALL + ["SFOD.SYNTHETIC.NUM_TEST_IMAGES", "6", "TEST.IMS_PER_BATCH", "3",
                                              "SFOD.SYNTHETIC.BOXES_PER_IMAGE", "7", "SFOD.SYNTHETIC.HEIGHT", "70",
                                              "SFOD.SYNTHETIC.WIDTH", "150"])     # 32 x 69 frames: scales that round in fp32
    loader = sfod.data.TestLoader(cfg, torch.device("cpu"))
    post = importlib.import_module("simple-sfod_amd.modeling.meta_arch").detector_postprocess
    a, b = sfod.evaluation.F1Evaluator(8, 0.5, 4, 0.5), sfod.evaluation.F1Evaluator(8, 0.5, 4, 0.5)
    for batch in loader:
        outs = _echo_outputs(sfod, batch)
        for d, o in zip(batch, outs):                # one box partly outside and one wholly outside the frame: clipped / dropped
            o["instances"].pred_boxes.tensor[0, 2] = d["width"] + 40.0
            o["instances"].pred_boxes.tensor[-1] = torch.tensor([d["width"] + 5.0, 0.0, d["width"] + 50.0, 20.0])
        assert all(o["instances"].image_size != d["instances"].image_size for d, o in zip(batch, outs))
        a.process(batch, outs)
        imgs = []
        for d, o in zip(batch, outs):
            r = post(o["instances"], *d["instances"].image_size)
            assert len(r) == len(o["instances"]) - 1
            imgs.append((8, r.pred_boxes.tensor.numpy(), r.scores.numpy(), r.pred_classes.numpy(),
                         d["instances"].gt_boxes.tensor.numpy(), d["instances"].gt_classes.numpy(), d["instances"].image_size))
        _batched(sfod, b, C.pack_arrays(imgs))
    assert (a.accumulated() == b.accumulated()).all()
    assert a.accumulated()[:, 0].sum() > 0 and a.accumulated()[:, 1].sum() > 0 and a.accumulated()[:, 2].sum() > 0
    with pytest.raises(ValueError, match="more than 100"):
        S = sfod.structures
        big = S.Instances((10, 10))
        big.pred_boxes, big.scores, big.pred_classes = S.Boxes(torch.zeros(101, 4)), torch.zeros(101), torch.zeros(101, dtype=torch.long)
        a.process([batch[0]], [{"instances": big}])


def test_dataset_evaluators_merge_and_refuse_a_duplicate_key(sfod):
    class Fixed:
        def __init__(self, res):
            self.res, self.calls = res, []

        def reset(self):
            self.calls.append("reset")

        def process(self, inputs, outputs):
            self.calls.append(("process", inputs, outputs))

        def evaluate(self):
            return self.res
    x, y, n = Fixed({"bbox": {"AP": 1.0}}), Fixed({"F1 Score": 0.5}), Fixed(None)
    ev = sfod.evaluation.DatasetEvaluators([x, y, n])
    ev.reset()
    ev.process([1], [2])
    assert x.calls == y.calls == n.calls == ["reset", ("process", [1], [2])]
    res = ev.evaluate()
    assert list(res.items()) == [("bbox", {"AP": 1.0}), ("F1 Score", 0.5)]
    with pytest.raises(ValueError, match="same key"):
        sfod.evaluation.DatasetEvaluators([x, Fixed({"bbox": {}})]).evaluate()


class _Echo(torch.nn.Module):
    def __init__(self, sfod):
        super().__init__()
        self.sfod = sfod

    def forward(self, batched_inputs):
        return _echo_outputs(self.sfod, batched_inputs)


def test_sfod_evaluators_key(sfod):
    E, T = sfod.evaluation, sfod.engine.BaseTrainer
    opts = SMALL + ["SFOD.SYNTHETIC.NUM_TEST_IMAGES", "4", "TEST.IMS_PER_BATCH", "3", "SFOD.SYNTHETIC.BOXES_PER_IMAGE", "5"]
    cfg = sfod.config.setup_cfg(HOT, opts)
    assert tuple(cfg.SFOD.EVALUATORS) == ("coco",)
    assert type(T.build_evaluator(cfg, "synthetic_cityscapes_foggy_val")) is E.NewCOCOEvaluator
    res = T.test(cfg, _Echo(sfod))
    assert list(res) == ["bbox"]
    cfg2 = sfod.config.setup_cfg(HOT, opts + ["SFOD.EVALUATORS", "('coco', 'f1')"])
    both = T.build_evaluator(cfg2, "synthetic_cityscapes_foggy_val")
    assert type(both) is E.DatasetEvaluators and [type(e) for e in both._evaluators] == [E.NewCOCOEvaluator, E.F1Evaluator]
    assert both._evaluators[1].class_number == cfg2.MODEL.ROI_HEADS.NUM_CLASSES
    res2 = T.test(cfg2, _Echo(sfod))
    assert list(res2) == ["bbox", "F1 Score"] and str(res2["bbox"]) == str(res["bbox"]) and 0 < res2["F1 Score"] < 1
    lines = E.print_csv_format(res2)                 # a scalar entry prints as one line
    assert lines[-1] == "copypaste: F1 Score={}".format(res2["F1 Score"])
    only = T.build_evaluator(sfod.config.setup_cfg(HOT, opts + ["SFOD.EVALUATORS", "('f1',)"]), "synthetic_cityscapes_foggy_val")
    assert type(only) is E.F1Evaluator
    for bad in ("('coco', 'dece')", "()", "('f1', 'f1')"):
        with pytest.raises(ValueError, match=r"SFOD\.EVALUATORS"):
            T.build_evaluator(sfod.config.setup_cfg(HOT, opts + ["SFOD.EVALUATORS", bad]), "synthetic_cityscapes_foggy_val")


def _rank_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sfod = importlib.import_module("simple-sfod_amd")
    cfg = sfod.config.setup_cfg(HOT, SMALL + ["SFOD.SYNTHETIC.NUM_TEST_IMAGES", "5", "TEST.IMS_PER_BATCH", "2",
                                              "SFOD.SYNTHETIC.BOXES_PER_IMAGE", "6", "SFOD.EVALUATORS", "('coco', 'f1')"])
    res = sfod.engine.BaseTrainer.test(cfg, _Echo(sfod))
    q.put((rank, {k: v for k, v in res.items() if k != "bbox"}, "bbox" in res))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_sum_their_counts_on_rank0(sfod):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35500 + os.getpid() % 2000
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        rank, r, has_bbox = q.get(timeout=300)
        res[rank] = (r, has_bbox)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert res[1] == ({}, False)                                   # only the main process gets results
    cfg = sfod.config.setup_cfg(HOT, SMALL + ["SFOD.SYNTHETIC.NUM_TEST_IMAGES", "5", "TEST.IMS_PER_BATCH", "2",
                                              "SFOD.SYNTHETIC.BOXES_PER_IMAGE", "6"])
    ev = sfod.evaluation.F1Evaluator(cfg.MODEL.ROI_HEADS.NUM_CLASSES)
    shares = []
    for rank in range(world):                                      # the whole set in one process; each rank's share on its own
        part = sfod.evaluation.F1Evaluator(cfg.MODEL.ROI_HEADS.NUM_CLASSES)
        for batch in sfod.data.TestLoader(cfg, torch.device("cpu"), rank, world):
            outs = _echo_outputs(sfod, batch)
            ev.process(batch, outs)
            part.process(batch, outs)
        shares.append(part.accumulated())
    whole = ev.evaluate()["F1 Score"]
    assert res[0] == ({"F1 Score": whole}, True) and 0 < whole < 1
    assert (shares[0] + shares[1] == ev.counts).all() and shares[1].sum() > 0     # rank 1's share is part of the total


def test_entry_point_refuses_broken_arguments_without_a_gpu(sfod):
    import ctypes
    lib = sfod.native.load()
    proto = sfod.native.parse_header()["sfod_f1_count"]
    assert proto[1][13] is ctypes.c_double and proto[1][15] is ctypes.c_float and len(proto[1]) == 18
    failures = []

    def body():      # sfod_last_error is per thread: the messages provoked here stay out of the other tests' thread
        try:
            buf = ctypes.create_string_buffer(1 << 12)
            P = (ctypes.addressof(buf) + 63) // 64 * 64
            names = ["det_boxes", "det_scores", "det_classes", "det_count", "gt_boxes", "gt_classes", "gt_count", "scale", "clip_size",
                     "B", "D", "G", "K", "iou", "top_n", "score", "counts", "stream"]
            valid = [P] * 9 + [2, 100, 100, 8, 0.5, 5, 0.5, P, None]
            for key, val in (("K", 0), ("K", 33), ("top_n", 0), ("top_n", 101), ("D", 101), ("G", 101), ("B", -1), ("D", -4),
                             ("iou", -0.1), ("iou", float("nan")), ("iou", float("inf")), ("score", float("nan")),
                             ("det_boxes", None), ("gt_count", None), ("counts", None)):
                a = list(valid)
                a[names.index(key)] = val
                assert lib.sfod_f1_count(*a) == -1000 and lib.sfod_last_error(), (key, val)
            a = list(valid)
            a[names.index("D")], a[names.index("top_n")] = 4, 5                  # top_n > D
            assert lib.sfod_f1_count(*a) == -1000 and b"top_n" in lib.sfod_last_error()
            a = list(valid)
            a[names.index("B")] = 0                                              # an empty batch is a valid call: nothing is launched
            assert lib.sfod_f1_count(*a) == 0
        except BaseException as e:      # noqa: BLE001 -- handed to the test's thread
            failures.append(e)
    before = lib.sfod_last_error()
    th = threading.Thread(target=body)
    th.start()
    th.join()
    if failures:
        raise failures[0]
    assert lib.sfod_last_error() == before
