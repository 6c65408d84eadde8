"""``TEST.AUG`` on the device: ``sfod_tta_merge`` + the merge chain against the numpy restatement of Detectron2's rule
(tests/helpers/tta_definitions.py) on built inputs that hold every edge (tests/helpers/tta_cases.py), and
``GeneralizedRCNNWithTTA`` end to end against that definition fed by ``model.inference`` on the same one-size passes.  The merge
reorders, rescales and selects: every comparison is bit equality of boxes and scores and equality of classes and counts."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import tta_cases as C
from helpers import tta_definitions as D
from helpers.detection_cases import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HOT_YAML = os.path.join(os.path.dirname(GOLDEN), "..", "configs", "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free.yaml")
DA_YAML = os.path.join(os.path.dirname(HOT_YAML), "faster_rcnn_VGG_cityscapes_foggy_da.yaml")
MIN_SIZES, MAX_SIZE = (48, 64, 80), 120


# ---- the kernel and its chain on built inputs ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    return {c["name"]: (c, C.expected(c)) for c in C.cases()}


def _run(native, case):
    t = {k: torch.from_numpy(case[k]).to(DEV) for k in ("det_boxes", "det_scores", "det_classes", "det_count", "table", "sizes")}
    out = native.tta_merge(t["det_boxes"], t["det_scores"], t["det_classes"], t["det_count"], t["table"], t["sizes"], case["K"],
                           D.SCORE_THRESH, case["nms_thresh"], case["topk"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", ["edges", "ratios"])
def test_merge_kernel_and_chain_equal_the_definition(native, built, name):
    case, exp = built[name]
    got = _run(native, case)
    n = case["A"] * case["cap"]
    assert got["cand_scores"].shape == (case["B"], n) and got["det_scores"].shape == (case["B"], case["topk"])
    for b in range(case["B"]):
        cb, cs, ck, cn = C.expected_candidates(case, b)
        assert int(got["cand_count"][b]) == cn == exp[b][3], (name, b)
        assert (bits(got["cand_scores"][b]) == bits(cs)).all() and (got["cand_classes"][b] == ck).all(), (name, b)
        assert (bits(got["cand_boxes"][b]) == bits(cb)).all(), (name, b)
        eb, es, ek, _ = exp[b]
        m = int(got["det_count"][b])
        assert m == len(es), (name, b, m, len(es))
        assert (got["det_classes"][b, :m] == ek).all(), (name, b)
        assert (bits(got["det_scores"][b, :m]) == bits(es)).all() and (bits(got["det_boxes"][b, :m]) == bits(eb)).all(), (name, b)
        assert not got["det_boxes"][b, m:].any() and not got["det_scores"][b, m:].any()           # the unused tail: zeros
    if name == "edges":
        assert int(got["det_count"][0]) == 100 and int(got["det_count"][1]) == 0 and int(got["cand_count"][1]) == 0


def test_merge_twice_gives_the_same_bits_and_dead_slots_are_never_read(native, built):
    case, _ = built["edges"]
    first = _run(native, case)
    other = dict(case)
    dead = np.arange(case["cap"])[None, None, :] >= case["det_count"][:, :, None]
    for k, fill in (("det_boxes", np.float32(-7e30)), ("det_scores", np.float32(3.0)), ("det_classes", np.int32(2))):
        other[k] = case[k].copy()
        other[k][dead] = fill                                        # other poison beyond det_count: nothing may change
    second = _run(native, other)
    for k in first:
        assert first[k].tobytes() == second[k].tobytes(), k


# ---- the module end to end ------------------------------------------------------------------------------------------------------
def _cfg(sfod, dtype, yaml=HOT_YAML, opts=()):
    return sfod.config.setup_cfg(yaml, [
        "OUTPUT_DIR", "", "SFOD.COMPUTE_DTYPE", dtype, "SFOD.SYNTHETIC.HEIGHT", "96", "SFOD.SYNTHETIC.WIDTH", "160",
        "SFOD.SYNTHETIC.NUM_TEST_IMAGES", "3", "SFOD.SYNTHETIC.BOXES_PER_IMAGE", "4", "INPUT.MIN_SIZE_TEST", "64", "TEST.IMS_PER_BATCH", "2",
        "DATASETS.TEST", "('synthetic_cityscapes_foggy_val',)", "TEST.AUG.MIN_SIZES", repr(MIN_SIZES), "TEST.AUG.MAX_SIZE", str(MAX_SIZE),
        "MODEL.DEVICE", DEV] + list(opts))


def _model(sfod, cfg, seed=17):
    torch.manual_seed(seed)
    model = sfod.modeling.build_model(cfg)
    with torch.no_grad():     # planted scores: detections clear the thresholds with distinct scores
        model.roi_heads.box_predictor.cls_score.weight.mul_(60.0)
        model.roi_heads.box_predictor.bbox_pred.weight.mul_(20.0)
        for name, buf in model.named_buffers():
            if name.endswith("running_mean"):
                buf.normal_(0.0, 0.05)
            if name.endswith("running_var"):
                buf.uniform_(0.5, 1.5)
    return model.eval()


def _definition(model, batch, K, nms_thresh, topk):
    """the rule of tests/helpers/tta_definitions.py with Pillow's augmented tensors and ``model.inference`` on the same one-size
    passes (one MIN_SIZES entry of one image: the plain tensor and its mirrored twin)"""
    out = []
    for inp in batch:
        h, w = (int(v) for v in inp["image"].shape[1:])
        augs = D.augmentations(h, w, inp["height"], inp["width"], MIN_SIZES, MAX_SIZE, True)
        img = inp["image"].cpu().numpy()
        passes = []
        for i in range(0, len(augs), 2):
            pair = [{"image": torch.from_numpy(D.augmented_image(img, a)).to(DEV), "height": a["size"][0], "width": a["size"][1]}
                    for a in augs[i:i + 2]]
            for r in model.inference(pair, do_postprocess=False):
                passes.append((r.pred_boxes.tensor.cpu().numpy(), r.scores.cpu().numpy(), r.pred_classes.cpu().numpy()))
        out.append((D.tta_image(passes, augs, (inp["height"], inp["width"]), K, nms_thresh, topk), passes, augs))
    return out


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_module_equals_the_definition_on_the_same_passes(sfod, native, dtype):
    cfg = _cfg(sfod, dtype)
    model = _model(sfod, cfg)
    tta = sfod.modeling.GeneralizedRCNNWithTTA(cfg, model)
    assert not tta.training and (tta.options.num_aug, tta.max_det) == (6, 100)
    loader = sfod.engine.BaseTrainer.build_test_loader(cfg, "synthetic_cityscapes_foggy_val")
    batches = list(loader)
    assert [len(b) for b in batches] == [2, 1] and tuple(batches[0][0]["image"].shape[1:]) == (64, 107)
    K, nms_thresh = cfg.MODEL.ROI_HEADS.NUM_CLASSES, cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST
    ndet = nflip = 0
    for batch in batches:
        outs = tta(batch)
        ref = _definition(model, batch, K, nms_thresh, 100)
        merged = tta.merged(batch)
        cand_s = merged.d["cand_scores"].view(len(batch), 6, 100).cpu().numpy()
        cand_b = merged.d["cand_boxes"].view(len(batch), 6, 100, 4).cpu().numpy()
        for b, (inp, o, (want, passes, augs)) in enumerate(zip(batch, outs, ref)):
            inst = o["instances"]
            assert list(o) == ["instances"] and inst.image_size == (inp["height"], inp["width"]) == (96, 160)
            assert sorted(inst.get_fields()) == ["pred_boxes", "pred_classes", "scores"] and inst.pred_classes.dtype == torch.int64
            gb, gs, gk = inst.pred_boxes.tensor.cpu().numpy(), inst.scores.cpu().numpy(), inst.pred_classes.cpu().numpy()
            assert len(gs) == len(want[1]) and (gk == want[2]).all(), (dtype, len(gs), len(want[1]))
            assert (bits(gs) == bits(want[1])).all() and (bits(gb) == bits(want[0])).all()
            assert (gb[:, 0::2] <= 160).all() and (gb[:, 1::2] <= 96).all() and (gb >= 0).all()
            # the hand-over: the plain and the mirrored pass of one size are each taken back by their own table row
            for a, (p, aug) in enumerate(zip(passes, augs)):
                n = len(p[1])
                inv = D.inverse_boxes(p[0], aug)
                inv[:, 0::2], inv[:, 1::2] = np.clip(inv[:, 0::2], 0, 160), np.clip(inv[:, 1::2], 0, 96)
                assert (bits(cand_s[b, a, :n]) == bits(p[1])).all() and (cand_s[b, a, n:] == -1).all()
                assert (bits(cand_b[b, a, :n]) == bits(inv)).all()
                nflip += n if aug["flip"] else 0
            ndet += len(gs)
        # the augmented tensors themselves: Pillow's, mirrored in the same launch
        plan = tta.plan_of(batch[0])
        for i, size in enumerate(plan.sizes):
            for f, t in enumerate(tta.augmented_inputs(batch[0], plan, i)):
                want_img = D.augmented_image(batch[0]["image"].cpu().numpy(), {"size": size, "flip": bool(f)})
                assert (t["height"], t["width"]) == size and np.array_equal(t["image"].cpu().numpy(), want_img)
    assert ndet > 10 and nflip > 10


def test_nothing_between_the_first_resize_and_the_instances_copies_to_the_host(sfod, native):
    cfg = _cfg(sfod, "fp32")
    model = _model(sfod, cfg)
    tta = sfod.modeling.GeneralizedRCNNWithTTA(cfg, model)
    batch = next(iter(sfod.engine.BaseTrainer.build_test_loader(cfg, "synthetic_cityscapes_foggy_val")))
    first = tta.merged(batch)                        # fills the caches of host constants (tables, sizes, resize coefficients)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")          # raises a Python error at a synchronising call; faults nothing
    try:
        second = tta.merged(batch)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert second.image_sizes == [(96, 160), (96, 160)] and second.d["det_boxes"].is_cuda
    for k in ("det_boxes", "det_scores", "det_classes", "det_count"):
        assert torch.equal(first.d[k], second.d[k]), k
    assert int(second.d["det_count"].sum()) > 0
    model.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        tta(batch)


def _same_results(a, b):
    assert list(a.keys()) == list(b.keys())
    for k in a:
        if isinstance(a[k], dict):
            _same_results(a[k], b[k])
        else:
            assert (np.isnan(a[k]) and np.isnan(b[k])) or a[k] == b[k], (k, a[k], b[k])


def test_trainer_test_is_untouched_when_disabled_and_test_with_tta_suffixes_its_keys(sfod, native, monkeypatch):
    T = sfod.engine.BaseTrainer
    cfg = _cfg(sfod, "fp32", opts=["SFOD.EVALUATORS", "('coco', 'f1')"])
    assert cfg.TEST.AUG.ENABLED is False
    model = _model(sfod, cfg)
    # what Trainer.test is: the evaluators fed by the plain eval-mode forward, batch by batch
    loader = T.build_test_loader(cfg, "synthetic_cityscapes_foggy_val")
    ev = T.build_evaluator(cfg, "synthetic_cityscapes_foggy_val", data_loader=loader)
    ev.reset()
    with torch.no_grad():
        for batch in loader:
            ev.process(batch, model(batch))
    want = ev.evaluate()

    def forbidden(*a, **k):
        raise AssertionError("TEST.AUG.ENABLED False must construct and call nothing of the augmentation")

    with monkeypatch.context() as mp:
        mp.setattr(sfod.modeling.tta.GeneralizedRCNNWithTTA, "__init__", forbidden)
        mp.setattr(sfod.modeling.tta_options.TTAOptions, "__init__", forbidden)
        mp.setattr(native, "tta_merge", forbidden)
        plain = T.test(cfg, model)
    assert list(plain.keys()) == ["bbox", "F1 Score"] and not model.training
    _same_results(plain, want)
    res = T.test_with_TTA(cfg, model)
    assert list(res.keys()) == ["bbox_TTA", "F1 Score_TTA"] and list(res["bbox_TTA"].keys()) == list(plain["bbox"].keys())
    assert not model.training                                   # the wrapper hands the model back in the mode it came in
    # ... and those are the evaluators' results on the wrapper's outputs
    ev.reset()
    tta = sfod.modeling.GeneralizedRCNNWithTTA(cfg, model)
    for batch in loader:
        ev.process(batch, tta(batch))
    _same_results(res, {k + "_TTA": v for k, v in ev.evaluate().items()})
    model.train()
    assert T.test_with_TTA(cfg, model).keys() == res.keys() and model.training       # inference_on_dataset's eval / restore


def test_the_da_meta_architecture_runs_behind_the_wrapper(sfod, native):
    """every meta-architecture whose eval path is ``inference``: DAFasterRCNN's ROI heads hand over the same containers"""
    cfg = _cfg(sfod, "fp32", yaml=DA_YAML)
    model = _model(sfod, cfg)
    assert type(model).__name__ == "DAFasterRCNN"
    tta = sfod.modeling.GeneralizedRCNNWithTTA(cfg, model)
    batch = next(iter(sfod.engine.BaseTrainer.build_test_loader(cfg, "synthetic_cityscapes_foggy_val")))
    outs = tta(batch)
    ref = _definition(model, batch, cfg.MODEL.ROI_HEADS.NUM_CLASSES, cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST, 100)
    for o, (want, _, _) in zip(outs, ref):
        inst = o["instances"]
        assert len(inst) == len(want[1]) and (inst.pred_classes.cpu().numpy() == want[2]).all()
        assert (bits(inst.scores.cpu().numpy()) == bits(want[1])).all()
        assert (bits(inst.pred_boxes.tensor.cpu().numpy()) == bits(want[0])).all()
