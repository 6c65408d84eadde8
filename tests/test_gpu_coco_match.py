"""``sfod_coco_match`` on the device: integer for integer against the numpy producer (tests/helpers/coco_match_definitions.py,
which tests/test_coco_match_host.py ties to ``COCOevalBBox.evaluate()``) on every case of tests/helpers/coco_match_cases.py;
``NewCOCOEvaluator(device_match=True)`` on CUDA instances against the host evaluator; ``Trainer.test`` with
``SFOD.COCO_EVAL_DEVICE`` on and off; no synchronisation inside ``process``.  Everything compared is an integer or a float
made of integers on the host: the gate is equality."""
import os

import numpy as np
import pytest
import torch

from helpers import coco_match_cases as C
from helpers import coco_match_definitions as Def

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOT = os.path.join(ROOT, "configs", "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free.yaml")
CASES = C.all_cases()
SENTINEL = -0x0123456789ABCDF           # in every byte lane of the four outputs something no result holds


def _run(native, arrs, K, sentinel=True):
    t = {k: torch.from_numpy(v).to(DEV) for k, v in arrs.items()}
    B, D = arrs["det_scores"].shape
    out = None
    if sentinel:
        out = (torch.full((B, D), -77, dtype=torch.int32, device=DEV), torch.full((B, D), SENTINEL, dtype=torch.int64, device=DEV),
               torch.full((B, D), SENTINEL, dtype=torch.int64, device=DEV),
               torch.full((B, K, len(C.AREA_RNG)), -77, dtype=torch.int32, device=DEV))
    got = native.coco_match(t["det_boxes"], t["det_scores"], t["det_classes"], t["det_count"], t["gt_boxes"], t["gt_area"],
                            t["gt_classes"], t["gt_iscrowd"], t["gt_count"], K, C.IOU_THRS, C.AREA_RNG, out=out)
    rank, match, ignore, npig = (g.cpu().numpy() for g in got)
    return rank, match.view(np.uint64), ignore.view(np.uint64), npig


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_kernel_equals_the_producer_on_every_case(native, case):
    for poison in (True, False):                         # padding beyond the counts that would match, then zeros
        arrs = C.pack(case["images"], C.D_CAP, case.get("G"), poison=poison)
        want = Def.coco_match(arrs, case["K"], C.IOU_THRS, C.AREA_RNG)
        got = _run(native, arrs, case["K"])
        for name, g, w in zip(("rank", "match", "ignore", "npig"), got, want):
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (case["name"], poison, name, np.argwhere(g != w)[:8].tolist())


def test_a_batch_of_different_images_and_two_launches(native):
    images = C.random_images(21, 4, 5, max_det=100, max_gt=40)
    arrs = C.pack(images, C.D_CAP, C.G_CAP)
    want = Def.coco_match(arrs, 5, C.IOU_THRS, C.AREA_RNG)
    first, second = _run(native, arrs, 5), _run(native, arrs, 5, sentinel=False)
    for g, h, w in zip(first, second, want):
        assert np.array_equal(g, w) and np.array_equal(h, w)
    assert want[1].any() and want[2].any()


@pytest.fixture(scope="module")
def random_set(sfod):
    images = C.random_images(13, 16, 4)
    dicts = C.to_dataset_dicts(images)
    names = ["c0", "c1", "c2", "c3"]
    host = sfod.evaluation.NewCOCOEvaluator("random", dicts, names, distributed=False)
    host.process(*C.instances(sfod, images, "cpu"))
    return images, dicts, names, host.evaluate()


def test_evaluator_on_cuda_instances_equals_the_host_evaluator_without_a_synchronisation(sfod, native, random_set):
    images, dicts, names, want = random_set
    dev = sfod.evaluation.NewCOCOEvaluator("random", dicts, names, distributed=False, device_match=True)
    batches = [C.instances(sfod, images[i:i + 4], DEV, first_id=i) for i in range(0, 16, 4)]
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")          # raises a Python error at a synchronising call; faults nothing
    try:
        for inputs, outputs in batches:
            dev.process(inputs, outputs)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert dev._predictions == [] and len(dev._matched) == 4 and all(t.is_cuda for m in dev._matched for t in m[1:])
    got = dev.evaluate()
    assert str(got) == str(want) and got["bbox"]["AP"] > 0 and got["bbox"]["AP50"] > got["bbox"]["AP75"] > 0
    assert set(dev.timings) == {"copy_s", "rebuild_s", "accumulate_s"}
    dev.reset()
    assert dev._matched == [] and dev.evaluate() == {}


def test_process_makes_no_cpu_call_and_refuses_more_than_100_detections(sfod, native, random_set, monkeypatch):
    images, dicts, names, _ = random_set
    dev = sfod.evaluation.NewCOCOEvaluator("random", dicts, names, distributed=False, device_match=True)
    inputs, outputs = C.instances(sfod, images[:4], DEV)
    calls = []
    cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: calls.append(self.shape) or cpu(self, *a, **k))
    dev.process(inputs, outputs)
    assert calls == []
    dev.evaluate()
    assert len(calls) == 1                                # the one copy of the concatenated outputs
    monkeypatch.undo()
    S = sfod.structures
    big = S.Instances((10, 10))
    big.pred_boxes, big.scores = S.Boxes(torch.zeros(101, 4, device=DEV)), torch.zeros(101, device=DEV)
    big.pred_classes = torch.zeros(101, dtype=torch.long, device=DEV)
    with pytest.raises(ValueError, match=r"TEST\.DETECTIONS_PER_IMAGE"):
        dev.process(inputs[:1], [{"instances": big}])
    host_inputs, host_outputs = C.instances(sfod, images[:2], "cpu")          # host tensors: the host path, unchanged
    dev.reset()
    dev.process(host_inputs, host_outputs)
    assert len(dev._predictions) == 2 and dev._matched == []


def test_trainer_test_gives_equal_results_with_the_key_on_and_off(sfod, native):
    T = sfod.engine.BaseTrainer
    opts = ["OUTPUT_DIR", "", "MODEL.DEVICE", DEV, "SFOD.SYNTHETIC.HEIGHT", "256", "SFOD.SYNTHETIC.WIDTH", "384", "INPUT.MIN_SIZE_TEST", "192",
            "DATASETS.TEST", "('synthetic_cityscapes_foggy_val',)", "SFOD.SYNTHETIC.NUM_TEST_IMAGES", "5", "TEST.IMS_PER_BATCH", "2",
            "SFOD.SYNTHETIC.BOXES_PER_IMAGE", "6"]
    cfg = sfod.config.setup_cfg(HOT, opts)
    torch.manual_seed(0)
    model = T.build_model(cfg)
    with torch.no_grad():        # planted scores so that the per-class NMS and the evaluators see detections
        model.roi_heads.box_predictor.cls_score.weight.mul_(60.0)
    off = T.test(cfg, model)
    on = T.test(sfod.config.setup_cfg(HOT, opts + ["SFOD.COCO_EVAL_DEVICE", "True"]), model)
    assert list(on) == ["bbox"] and str(on) == str(off) and "nan" not in str(off["bbox"]["AP"])
    both = opts + ["SFOD.EVALUATORS", "('coco', 'f1')"]
    off2 = T.test(sfod.config.setup_cfg(HOT, both), model)
    on2 = T.test(sfod.config.setup_cfg(HOT, both + ["SFOD.COCO_EVAL_DEVICE", "True"]), model)
    assert list(on2) == ["bbox", "F1 Score"] and str(on2) == str(off2) and str(on2["bbox"]) == str(off["bbox"])
    assert on2["F1 Score"] == off2["F1 Score"]


class _Echo(torch.nn.Module):
    """detections = the ground truth at the frame's native size, every third box shifted"""

    def __init__(self, sfod):
        super().__init__()
        self.sfod = sfod

    def forward(self, batched_inputs):
        S = self.sfod.structures
        outs = []
        for d in batched_inputs:
            inst = S.Instances((d["height"], d["width"]))
            boxes = d["instances"].gt_boxes.tensor.clone() * (d["width"] / d["image"].shape[2])
            boxes[::3, 0] += 3.3
            inst.pred_boxes = S.Boxes(boxes)
            inst.scores = torch.linspace(0.95, 0.35, len(boxes), device=boxes.device)
            inst.pred_classes = d["instances"].gt_classes
            outs.append({"instances": inst})
        return outs


def test_trainer_test_with_matching_detections_gives_equal_results_with_the_key_on_and_off(sfod, native):
    """the trained-from-nothing head above need not hit a single ground truth; here every detection lies on one"""
    T = sfod.engine.BaseTrainer
    opts = ["OUTPUT_DIR", "", "MODEL.DEVICE", DEV, "SFOD.SYNTHETIC.HEIGHT", "256", "SFOD.SYNTHETIC.WIDTH", "384", "INPUT.MIN_SIZE_TEST", "192",
            "DATASETS.TEST", "('synthetic_cityscapes_foggy_val',)", "SFOD.SYNTHETIC.NUM_TEST_IMAGES", "5", "TEST.IMS_PER_BATCH", "2",
            "SFOD.SYNTHETIC.BOXES_PER_IMAGE", "6", "SFOD.EVALUATORS", "('coco', 'f1')"]
    model = _Echo(sfod)
    off = T.test(sfod.config.setup_cfg(HOT, opts), model)
    on = T.test(sfod.config.setup_cfg(HOT, opts + ["SFOD.COCO_EVAL_DEVICE", "True"]), model)
    assert list(on) == ["bbox", "F1 Score"] and str(on) == str(off)
    assert on["bbox"]["AP50"] > 50 and on["bbox"]["AP"] > 0 and on["F1 Score"] > 0
