"""TRAINER "da" (DA Faster R-CNN) without a device: registries, trainer dispatch, the validation of modeling/da_options.py,
state-dict names, the loss definitions of tests/helpers/da_definitions.py against the reference's recorded values
(tests/golden/da_ref.npz, written by tools/record_da_golden.py from the reference's own code) and the loader's bucket rule.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import da_cases as C
from helpers import da_definitions as D

CONFIGS = os.path.join(os.path.dirname(GOLDEN), "..", "configs")
DA_YAML = os.path.join(CONFIGS, "faster_rcnn_VGG_cityscapes_foggy_da.yaml")
HOT_YAML = os.path.join(CONFIGS, "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free.yaml")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "da_ref.npz"), allow_pickle=False)


def cfg_of(sfod, *opts):
    return sfod.config.setup_cfg(DA_YAML, ["OUTPUT_DIR", ""] + list(opts))


def test_registries_resolve_the_da_names(sfod):
    r = sfod.registry
    m = sfod.modeling.da_faster_rcnn
    assert r.META_ARCH_REGISTRY.get("DAFasterRCNN") is m.DAFasterRCNN
    assert r.PROPOSAL_GENERATOR_REGISTRY.get("DARPN") is m.DARPN
    assert r.ROI_HEADS_REGISTRY.get("DAStandardROIHeads") is m.DAStandardROIHeads
    assert issubclass(m.DARPN, sfod.modeling.rpn.RPN) and issubclass(m.DAStandardROIHeads, sfod.modeling.roi_heads.StandardROIHeads)


def test_trainer_dispatch(sfod):
    assert sfod.engine.get_trainer_class(cfg_of(sfod)) is sfod.engine.DATrainer
    assert issubclass(sfod.engine.DATrainer, sfod.engine.BaseTrainer)
    with pytest.raises(ValueError, match="MODEL.META_ARCHITECTURE"):
        sfod.engine.get_trainer_class(sfod.config.setup_cfg(HOT_YAML, ["TRAINER", "da"]))


@pytest.mark.parametrize("opts, key", [
    (["MODEL.META_ARCHITECTURE", "GeneralizedRCNN"], "MODEL.META_ARCHITECTURE"),
    (["MODEL.ROI_HEADS.NAME", "StandardROIHeads"], "MODEL.ROI_HEADS.NAME"),
    (["DA_FASTER.LEVELS", "['vgg3', 'vgg4']"], "DA_FASTER.LEVELS"),
    (["DA_FASTER.LEVELS", "[]"], "DA_FASTER.LEVELS"),
    (["DA_FASTER.LEVELS", "['vgg3']"], "DA_FASTER.LEVELS"),                  # not the feature the ROI heads pool
    (["DA_FASTER.ENTROPY_CONDITIONING", "True"], "DA_FASTER.ENTROPY_CONDITIONING"),
    (["DA_FASTER.DC_IMG_GRL_WEIGHT", "-0.1"], "DA_FASTER.DC_IMG_GRL_WEIGHT"),
    (["DA_FASTER.DC_INS_GRL_WEIGHT", "1e999"], "DA_FASTER.DC_INS_GRL_WEIGHT"),
    (["DA_FASTER.DC_CONSISTENCY_WEIGHT", "-1e999"], "DA_FASTER.DC_CONSISTENCY_WEIGHT"),
    (["MODEL.ROI_BOX_HEAD.NUM_FC", "0", "MODEL.ROI_BOX_HEAD.NUM_CONV", "1"], "MODEL.ROI_BOX_HEAD.NUM_FC"),
])
def test_validation_names_the_key(sfod, opts, key):
    from importlib import import_module
    O = import_module("simple-sfod_amd.modeling.da_options")
    cfg = cfg_of(sfod, *opts)
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        O.validate_da_trainer_cfg(cfg)
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        sfod.engine.get_trainer_class(cfg)


def test_levels_must_be_a_backbone_feature_and_the_model_checks_on_construction(sfod):
    from importlib import import_module
    O = import_module("simple-sfod_amd.modeling.da_options")
    with pytest.raises(ValueError, match=r"DA_FASTER\.LEVELS"):
        O.da_options(cfg_of(sfod), backbone_features={"vgg0", "vgg1"})
    o = O.da_options(cfg_of(sfod), backbone_features={"vgg4"})
    assert (o.level, o.img_weight, o.ins_weight, o.consistency_weight) == ("vgg4", 0.01, 0.1, 0.1)
    with pytest.raises(ValueError, match=r"DA_FASTER\.ENTROPY_CONDITIONING"):
        sfod.registry.META_ARCH_REGISTRY.get("DAFasterRCNN")(cfg_of(sfod, "DA_FASTER.ENTROPY_CONDITIONING", "True"))


def test_state_dict_keys_are_the_references(sfod):
    torch.manual_seed(0)
    model = sfod.registry.META_ARCH_REGISTRY.get("DAFasterRCNN")(cfg_of(sfod))
    keys = set(model.state_dict())
    want = {f"DC_img.DC_img_conv{k}_level_vgg4.{p}" for k in (1, 2) for p in ("weight", "bias")} | \
           {f"DC_ins.da_ins_fc{k}_level_vgg4.{p}" for k in (1, 2, 3) for p in ("weight", "bias")}
    assert want <= keys and {k for k in keys if k.startswith("DC_")} == want
    sd = model.state_dict()
    assert tuple(sd["DC_img.DC_img_conv1_level_vgg4.weight"].shape) == (512, 512, 1, 1)
    assert tuple(sd["DC_img.DC_img_conv2_level_vgg4.weight"].shape) == (1, 512, 1, 1)
    assert tuple(sd["DC_ins.da_ins_fc1_level_vgg4.weight"].shape) == (1024, 1024)
    assert float(sd["DC_img.DC_img_conv1_level_vgg4.bias"].abs().max()) == 0.0
    assert 0.0005 < float(sd["DC_img.DC_img_conv1_level_vgg4.weight"].std()) < 0.002          # normal(std=0.001)
    for k in ("roi_heads.box_head.fc1.weight", "proposal_generator.rpn_head.conv.weight", "backbone.vgg0.0.weight"):
        assert k in keys


# ---- the definitions against the recorded reference values -------------------------------------------------------------------
def check_recorded(fx, key, t, rel=1e-12):
    t = t.detach().double().reshape(-1)
    if key in fx.files:
        ref = torch.from_numpy(fx[key]).reshape(-1)
        assert ref.numel() == t.numel(), key
        scale = max(float(ref.abs().max()), 1e-300)
        assert float((t - ref).abs().max()) <= rel * scale, (key, float((t - ref).abs().max()), scale)
        return
    ref = torch.from_numpy(fx[key + "@probe"])
    norm = float(fx[key + "@norm"])
    got = t[C.probe_indices(t.numel())]
    assert float((got - ref).abs().max()) <= rel * max(float(ref.abs().max()), norm / t.numel() ** 0.5), key
    assert abs(float(t.norm()) - norm) <= 1e-10 * norm, key
    assert abs(float(t.sum()) - float(fx[key + "@sum"])) <= 1e-9 * max(norm, 1e-300), key


def leaf(t):
    return t.clone().requires_grad_(True)


def test_head_definitions_equal_the_recorded_reference(fx):
    sc = C.small_case()
    feat, w = leaf(sc["feat"]), {k: leaf(v) for k, v in sc["w_img"].items()}
    y = D.img_head(feat, w)
    check_recorded(fx, "img_head/out", y)
    names = ["feat"] + ["w_img/" + k for k in w]
    for n, g in zip(names, torch.autograd.grad(y.sum(), [feat] + list(w.values()))):
        check_recorded(fx, "img_head/g/" + n, g)
    for mode in ("eval", "train"):
        bf, w = leaf(sc["box_features"]), {k: leaf(v) for k, v in sc["w_ins"].items()}
        y = D.ins_head(bf, w, sc["masks"][0] if mode == "train" else None)
        check_recorded(fx, f"ins_head/{mode}/out", y)
        names = ["box_features"] + ["w_ins/" + k for k in w]
        for n, g in zip(names, torch.autograd.grad(y.sum(), [bf] + list(w.values()))):
            check_recorded(fx, f"ins_head/{mode}/g/" + n, g)


@pytest.mark.parametrize("run", C.SMALL_RUNS, ids=lambda r: "w{}-l{}-p{}-{}".format(*r))
def test_loss_definitions_equal_the_recorded_reference(fx, run):
    k, label, pi, mode = run
    sc = C.small_case()
    feat, bf = leaf(sc["feat"]), leaf(sc["box_features"])
    w_img, w_ins = {n: leaf(v) for n, v in sc["w_img"].items()}, {n: leaf(v) for n, v in sc["w_ins"].items()}
    res = D.evaluate_losses(feat, bf, sc["rois"], w_img, w_ins, C.WEIGHT_SETS[k], label, C.POOLERS[pi],
                            sc["masks"] if mode == "train" else None, pool="oracle")
    prefix = f"small/w{k}/l{label}/p{pi}/{mode}"
    seen = 0
    for which, (value, grads) in res.items():
        ref = float(fx[f"{prefix}/{which}/value"])
        assert abs(value.item() - ref) <= 1e-12 * abs(ref), (which, value.item(), ref)
        recorded = {f.split("/g/", 1)[1].split("@")[0] for f in fx.files if f.startswith(f"{prefix}/{which}/g/")}
        assert recorded == set(grads), (which, recorded ^ set(grads))
        for n, g in grads.items():
            check_recorded(fx, f"{prefix}/{which}/g/{n}", g)
            seen += 1
    assert seen >= 20


def test_the_two_pooling_forms_agree_to_fp32_rounding():
    """``pool="oracle"`` carries the fp32 rounding of the C ROIAlign, ``pool="matrices"`` is float64 throughout: the same
    number up to a few fp32 ulps of a probability, for both pooler settings and every ROI shape of the case."""
    sc = C.small_case()
    z = D.img_head(sc["feat"], sc["w_img"])
    live = sc["rois"][sc["rois"][:, 0] >= 0].double()
    for pooled, sr, aligned in C.POOLERS:
        a = D.pooled_mean(torch.sigmoid(z), live, pooled, 1.0 / C.STRIDE, sr, aligned, pool="oracle")
        b = D.pooled_mean(torch.sigmoid(z), live, pooled, 1.0 / C.STRIDE, sr, aligned, pool="matrices")
        assert float((a - b).abs().max()) < 16 * 2.0 ** -24
        assert float(b.abs().max()) > 0.1
    assert float(D.pooled_mean(torch.sigmoid(z), live[4:5], 7, 1.0 / C.STRIDE, 0, True).abs().max()) == 0.0      # x2 == x1


def test_empty_domain_gives_zero_not_nan():
    z = torch.zeros(2, 5, 7, dtype=torch.float64)
    rois = torch.tensor([[-1.0, 0, 0, 0, 0]] * 3, dtype=torch.float64)
    loss, _, d = D.consistency(z, torch.zeros(3, dtype=torch.float64), rois, 7, 1.0 / 32)
    assert loss.item() == 0.0 and d.numel() == 0
    assert D.bce(torch.zeros(3), 1.0, live=torch.zeros(3, dtype=torch.bool))[0].item() == 0.0


# ---- the loader ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [0, 1])
def test_bucket_rule_yields_the_recorded_sequence(sfod, fx, ci):
    from importlib import import_module
    S = import_module("simple-sfod_amd.data.synthetic")
    mk = lambda wide, base: [{"width": 1200 if w else 600, "height": 600 if w else 1200, "image_id": base + i}
                             for i, w in enumerate(wide.tolist())]
    lab, unl = mk(fx[f"bucket/{ci}/wide_label"], 0), mk(fx[f"bucket/{ci}/wide_unlabel"], 1000)
    batches = list(S.semisup_batches(iter(lab), iter(unl), 2, 3))
    assert len(batches) == len(fx[f"bucket/{ci}/label_ids"]) > 5
    np.testing.assert_array_equal(np.array([[d["image_id"] for d in a] for a, _ in batches]), fx[f"bucket/{ci}/label_ids"])
    np.testing.assert_array_equal(np.array([[d["image_id"] for d in b] for _, b in batches]), fx[f"bucket/{ci}/unlabel_ids"])
    for a, b in batches:      # one aspect class per list
        assert len({d["width"] > d["height"] for d in a}) == 1 and len({d["width"] > d["height"] for d in b}) == 1


def test_loader_refuses_what_the_reference_refuses(sfod):
    from importlib import import_module
    S = import_module("simple-sfod_amd.data.synthetic")
    with pytest.raises(NotImplementedError, match="ASPECT_RATIO_GROUPING"):
        S.DALoader(cfg_of(sfod, "DATALOADER.ASPECT_RATIO_GROUPING", "False"), "cpu")
    with pytest.raises(AssertionError, match="Total target batch size"):
        S.DALoader(cfg_of(sfod, "SOLVER.IMS_PER_BATCH", "2", "SOLVER.IMS_PER_BATCH_TARGET", "3"), "cpu", 0, 2)


def test_loader_yields_source_and_target_lists_of_the_configured_sizes(sfod):
    from importlib import import_module
    S = import_module("simple-sfod_amd.data.synthetic")
    cfg = cfg_of(sfod, "SOLVER.IMS_PER_BATCH", "2", "SOLVER.IMS_PER_BATCH_TARGET", "3", "SFOD.SYNTHETIC.HEIGHT", "64",
                 "SFOD.SYNTHETIC.WIDTH", "96", "SFOD.SYNTHETIC.NUM_IMAGES", "6", "INPUT.MIN_SIZE_TRAIN", "(64,)")
    src, tgt = next(iter(S.DALoader(cfg, "cpu")))
    assert len(src) == 2 and len(tgt) == 3
    assert all("instances" in d and d["image"].dtype == torch.uint8 for d in src)
    ids = lambda lst: [d["file_name"] for d in lst]
    assert set(ids(src)) != set(ids(tgt)) or cfg.DATASETS.TRAIN != cfg.DATASETS.TRAIN_TARGET
