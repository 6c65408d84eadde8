"""Classification-loss options without a device: known answers of tests/helpers/cls_loss_definitions.py, the validation of
modeling/cls_loss_options.py (every refusal names its key; defaults give no options object), the refusals of the ``*_cls``
entry points before any launch, and the focal yaml."""
import ctypes
import importlib
import math
import os
import re
import threading

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from helpers import cls_loss_definitions as D

CONFIGS = os.path.join(ROOT, "configs")
HOT_YAML = os.path.join(CONFIGS, "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free.yaml")
FOCAL_YAML = os.path.join(CONFIGS, "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free_focal.yaml")
DA_YAML = os.path.join(CONFIGS, "faster_rcnn_VGG_cityscapes_foggy_da.yaml")
CDA_YAML = os.path.join(CONFIGS, "faster_rcnn_VGG_cityscapes_foggy_cda.yaml")


def _opts():
    return importlib.import_module("simple-sfod_amd.modeling.cls_loss_options")


def _cfg(sfod, *opts, yaml=HOT_YAML):
    return sfod.config.setup_cfg(yaml, ["OUTPUT_DIR", ""] + list(opts))


# ---- definitions -----------------------------------------------------------------------------------------------------------
def test_focal_known_answer_and_gamma_zero_is_cross_entropy():
    z = torch.zeros(1, 2, dtype=torch.float64)
    c = torch.tensor([0])
    loss, s = D.cls_loss(z, c, "focal", gamma=2.0)
    assert abs(loss.item() - 0.25 * math.log(2.0)) < 1e-15 and abs(s.item() - loss.item()) < 1e-18      # p = 1/2: (1/2)^2 ln 2
    g = torch.Generator().manual_seed(0)
    z = torch.randn(40, 9, generator=g, dtype=torch.float64) * 3
    c = torch.randint(0, 9, (40,), generator=g)
    c[33:] = -1                                                         # padding rows take no part
    ce = F.cross_entropy(z[:33], c[:33], reduction="sum") / 33
    assert torch.equal(D.cls_loss(z, c, "focal", gamma=0.0)[0], D.cls_loss(z, c, "ce")[0])
    assert abs(D.cls_loss(z, c, "ce")[0].item() - ce.item()) < 1e-14
    # gamma > 0 down-weights every row: 0 < focal < CE
    assert 0 < D.cls_loss(z, c, "focal", gamma=1.5)[0].item() < ce.item()
    _, _, g0 = D.evaluate(z, c, "focal", 0.0, 1.0, torch.float64)
    _, _, gc = D.evaluate(z, c, "ce", 0.0, 1.0, torch.float64)
    assert torch.equal(g0, gc) and (g0[33:] == 0).all()


def test_sigmoid_known_answers():
    g = torch.Generator().manual_seed(1)
    K = 5
    z = torch.randn(3, K + 1, generator=g, dtype=torch.float64) * 2
    bg = torch.full((3,), K)
    # a background row has the all-zero target: sum softplus(z[:K]); the background column takes no part
    want = F.softplus(z[:, :K]).sum() / 3
    assert abs(D.cls_loss(z, bg, "sigmoid")[0].item() - want.item()) < 1e-14
    z2 = z.clone()
    z2[:, K] += 100.0
    assert torch.equal(D.cls_loss(z2, bg, "sigmoid")[0], D.cls_loss(z, bg, "sigmoid")[0])
    # a foreground row: softplus(-z_c) + the other foreground columns' softplus(z_j)
    c = torch.tensor([2, 0, 4])
    want = sum(F.softplus(-z[i, c[i]]) + F.softplus(z[i, :K]).sum() - F.softplus(z[i, c[i]]) for i in range(3)) / 3
    assert abs(D.cls_loss(z, c, "sigmoid")[0].item() - want.item()) < 1e-14
    _, _, grad = D.evaluate(z, c, "sigmoid", 0.0, 1.0, torch.float64)
    assert (grad[:, K] == 0).all() and (grad[:, :K] != 0).all()
    assert torch.equal(D.probs(z, True), torch.sigmoid(z)) and torch.allclose(D.probs(z, False).sum(1), torch.ones(3, dtype=torch.float64))


def test_gate_uses_the_floor_alone_where_fp32_is_not_finite():
    ref = torch.tensor([1.0, 2.0], dtype=torch.float64)
    assert D.gate(ref, torch.tensor([1.0, float("nan")]), 2.0)[0] == 4.0 * 2.0 ** -24 * 2.0
    assert D.gate(ref, torch.tensor([1.0, 2.5]), 2.0) == (2.0, 0.5)
    assert D.gate(ref, ref.float(), 2.0)[0] == 4.0 * 2.0 ** -24 * 2.0


# ---- validation ------------------------------------------------------------------------------------------------------------
def test_defaults_give_no_options_object(sfod):
    O = _opts()
    for yaml in (HOT_YAML, DA_YAML, CDA_YAML):
        cfg = _cfg(sfod, yaml=yaml)
        assert cfg.MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE is False and cfg.MODEL.ROI_BOX_HEAD.USE_FED_LOSS is False
        assert cfg.SFOD.FOCAL_LOSS_GAMMA == 1.5
        assert O.native_cls_loss(cfg) is None
        o = O.cls_loss_options(cfg)
        assert o.is_default() and o.mode == 0 and o.kind == "CrossEntropy" and not o.sigmoid
    # a changed gamma alone changes nothing that runs
    assert O.native_cls_loss(_cfg(sfod, "SFOD.FOCAL_LOSS_GAMMA", "2.0")) is None
    bp = sfod.modeling.roi_heads.FastRCNNOutputLayers(_cfg(sfod), sfod.structures.ShapeSpec(channels=64))
    assert bp._cls_loss is None


def test_built_options(sfod):
    O = _opts()
    o = O.native_cls_loss(_cfg(sfod, "MODEL.ROI_HEADS.LOSS", "FocalLoss"))
    assert (o.kind, o.gamma, o.sigmoid, o.mode) == ("FocalLoss", 1.5, False, 1)
    o = O.native_cls_loss(_cfg(sfod, "MODEL.ROI_HEADS.LOSS", "FocalLoss", "SFOD.FOCAL_LOSS_GAMMA", "0.5"))
    assert (o.gamma, o.mode) == (0.5, 1)
    assert O.native_cls_loss(_cfg(sfod, "MODEL.ROI_HEADS.LOSS", "FocalLoss", "SFOD.FOCAL_LOSS_GAMMA", "0")).gamma == 0.0
    o = O.native_cls_loss(_cfg(sfod, "MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE", "True"))
    assert (o.kind, o.sigmoid, o.mode) == ("CrossEntropy", True, 2)
    # sigmoid CE under TRAINER "da" with DAFasterRCNN (its yaml has no MODEL.ROI_HEADS.LOSS key: cross-entropy)
    o = O.native_cls_loss(_cfg(sfod, "MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE", "True", yaml=DA_YAML))
    assert o.mode == 2
    # the two teacher-student ROI heads build their predictor with the focal loss
    R = sfod.modeling.roi_heads
    cfg = _cfg(sfod, "MODEL.ROI_HEADS.LOSS", "FocalLoss", "SFOD.FOCAL_LOSS_GAMMA", "2.0")
    shape = {"vgg4": sfod.structures.ShapeSpec(channels=512, stride=16)}
    for cls, layers in ((R.SourceFreeAdaptiveTeacherStandardROIHeads, R.SourceFreeFastRCNNOutputLayers),
                        (R.AdaptiveTeacherStandardROIHeads, R.FastRCNNOutputLayers)):
        bp = cls(cfg, shape).box_predictor
        assert type(bp) is layers and (bp._cls_loss.mode, bp._cls_loss.gamma) == (1, 2.0)


def test_options_value_refuses_with_a_value_error(sfod):
    N = sfod.native
    with pytest.raises(ValueError, match="kind"):
        N.ClsLossOptions("Hinge", 1.5, False)
    with pytest.raises(ValueError, match="sigmoid"):
        N.ClsLossOptions("FocalLoss", 1.5, True)


REFUSALS = [
    (HOT_YAML, ["MODEL.ROI_HEADS.LOSS", "Hinge"], r"MODEL\.ROI_HEADS\.LOSS"),
    (HOT_YAML, ["MODEL.ROI_HEADS.LOSS", "FocalLoss", "MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE", "True"],
     r"MODEL\.ROI_HEADS\.LOSS.*MODEL\.ROI_BOX_HEAD\.USE_SIGMOID_CE"),
    (HOT_YAML, ["MODEL.ROI_BOX_HEAD.USE_FED_LOSS", "True"], r"MODEL\.ROI_BOX_HEAD\.USE_FED_LOSS"),
    (HOT_YAML, ["SFOD.FOCAL_LOSS_GAMMA", "-0.5"], r"SFOD\.FOCAL_LOSS_GAMMA"),
    (HOT_YAML, ["SFOD.FOCAL_LOSS_GAMMA", "float('inf')"], r"SFOD\.FOCAL_LOSS_GAMMA"),
    (HOT_YAML, ["SFOD.FOCAL_LOSS_GAMMA", "float('nan')"], r"SFOD\.FOCAL_LOSS_GAMMA"),
    (HOT_YAML, ["MODEL.RPN.LOSS", "FocalLoss"], r"MODEL\.RPN\.LOSS"),
    (HOT_YAML, ["MODEL.ROI_HEADS.LOSS", "FocalLoss", "MODEL.ROI_HEADS.NAME", "StandardROIHeads"], r"MODEL\.ROI_HEADS\.LOSS"),
    (HOT_YAML, ["MODEL.ROI_HEADS.LOSS", "FocalLoss", "MODEL.ROI_HEADS.NAME", "DAStandardROIHeads"], r"MODEL\.ROI_HEADS\.LOSS"),
    (HOT_YAML, ["MODEL.ROI_HEADS.LOSS", "FocalLoss", "MODEL.ROI_HEADS.NAME", "CDAStandardROIHeads"], r"MODEL\.ROI_HEADS\.LOSS"),
    (CDA_YAML, ["MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE", "True"], r"MODEL\.ROI_BOX_HEAD\.USE_SIGMOID_CE"),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_every_refusal_names_its_key(sfod, case):
    yaml, opts, pattern = REFUSALS[case]
    O = _opts()
    opts = list(opts)
    special = {"float('inf')": float("inf"), "float('nan')": float("nan")}
    plain = [o for o in opts if o not in special]
    cfg = _cfg(sfod, *plain, yaml=yaml) if len(plain) == len(opts) else None
    if cfg is None:      # a non-finite gamma cannot be written on a command line: set it on the node
        cfg = _cfg(sfod, yaml=yaml)
        cfg.defrost()
        cfg.SFOD.FOCAL_LOSS_GAMMA = special[opts[1]]
        cfg.freeze()
    with pytest.raises(ValueError, match=pattern):
        O.cls_loss_options(cfg)
    with pytest.raises(ValueError, match=pattern):
        O.native_cls_loss(cfg)


def test_roi_heads_classes_refuse_what_their_reference_class_does_not_read(sfod):
    """the class that is being built decides, not MODEL.ROI_HEADS.NAME: the hot yaml's cfg with "FocalLoss" builds the two
    teacher-student heads and is refused by the three others; the predictor built on its own follows the cfg's name"""
    R = sfod.modeling.roi_heads
    cfg = _cfg(sfod, "MODEL.ROI_HEADS.LOSS", "FocalLoss")
    shape = {"vgg4": sfod.structures.ShapeSpec(channels=512, stride=16)}
    for cls in (R.StandardROIHeads, R.DAStandardROIHeads, R.CDAStandardROIHeads):
        with pytest.raises(ValueError, match=r"MODEL\.ROI_HEADS\.LOSS"):
            cls(cfg, shape)
    bad = _cfg(sfod, "MODEL.ROI_HEADS.LOSS", "Hinge")
    for cls in (R.SourceFreeAdaptiveTeacherStandardROIHeads, R.AdaptiveTeacherStandardROIHeads):
        with pytest.raises(ValueError, match=r"MODEL\.ROI_HEADS\.LOSS"):
            cls(bad, shape)
    assert R.FastRCNNOutputLayers(cfg, sfod.structures.ShapeSpec(channels=64))._cls_loss.mode == 1


def test_focal_yaml_is_the_hot_yaml_plus_the_loss(sfod):
    a, b = _cfg(sfod), _cfg(sfod, yaml=FOCAL_YAML)
    assert b.MODEL.ROI_HEADS.LOSS == "FocalLoss" and a.MODEL.ROI_HEADS.LOSS == "CrossEntropy"
    assert _opts().native_cls_loss(b).mode == 1 and _opts().native_cls_loss(b).gamma == 1.5
    b.defrost()
    b.MODEL.ROI_HEADS.LOSS = "CrossEntropy"
    b.OUTPUT_DIR = a.OUTPUT_DIR
    assert b.dump() == a.dump()


# ---- the entry points refuse before any launch -----------------------------------------------------------------------------
def _param_names(sfod, name):
    src = open(sfod.native.HEADER).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
    return [re.sub(r"[\*\s]", " ", a).split()[-1] for a in m.group(1).split(",")]


def _refusals(sfod, lib, protos):
    buf = ctypes.create_string_buffer(1 << 12)
    P = (ctypes.addressof(buf) + 63) // 64 * 64
    nan, inf = float("nan"), float("inf")
    modes = [("cls_mode", v) for v in (-1, 3, 17)]
    gammas = [("gamma", v) for v in (-1e-3, nan, inf, -inf)]

    def refused(name, valid, mutations):
        assert name in protos
        names = _param_names(sfod, name)
        assert len(names) == len(valid) == len(protos[name][1]), (name, names)
        fn = getattr(lib, name)
        for key, val in mutations:
            a = list(valid)
            a[names.index(key)] = val
            assert fn(*a) == -1000 and lib.sfod_last_error(), (name, key, val)

    # (pred, ld, R, K, rois, gt_cls, gt_box, n_valid, loss, grad_scale, d_pred, ws, wx, wy, ww, wh, loss_type, beta,
    #  cls_agnostic, cls_mode, gamma, stream)
    v = [P, 48, 300, 8, P, P, P, P, P, None, None, P, 10.0, 10.0, 5.0, 5.0, 0, 0.5, 0, 1, 1.5, None]
    refused("sfod_frcnn_loss_cls", v, modes + gammas + [("ld", 40),
                                               ("K", 0), ("K", 4097), ("R", -1), ("wx", 0.0), ("loss_type", 2), ("beta", nan),
                                               ("pred", None), ("rois", None), ("gt_cls", None), ("gt_box", None),
                                               ("n_valid", None), ("loss", None), ("ws", None), ("grad_scale", P)])
    v[1], v[18] = 16, 1                                  # class-agnostic: K + 5 = 13 columns fit 16, not 12
    refused("sfod_frcnn_loss_cls", v, [("ld", 12), ("cls_agnostic", 0)])
    # (pred, ld, B, P, K, props, prop_count, image_sizes, score_thresh, cand_boxes, cand_scores, cand_count, wx, wy, ww, wh,
    #  cls_agnostic, cls_mode, gamma, stream)
    v = [P, 48, 2, 100, 8, P, P, P, 0.05, P, P, P, 10.0, 10.0, 5.0, 5.0, 0, 2, 1.5, None]
    refused("sfod_frcnn_candidates_cls", v, modes + gammas + [("ld", 40), ("K", 33), ("P", -1), ("wh", nan), ("pred", None), ("props", None),
                                                     ("prop_count", None), ("image_sizes", None), ("cand_boxes", None),
                                                     ("cand_scores", None), ("cand_count", None)])
    # (scores, ld, R, K, cls_mode, gamma, probs, stream)
    v = [P, 16, 100, 8, 2, 1.5, P, None]
    refused("sfod_predict_probs_cls", v, modes + gammas + [("ld", 8), ("K", 0), ("K", 33), ("R", -2), ("scores", None), ("probs", None)])
    # (pred, ld, R, K, rois, roi_cls, B, image_sizes, gt_boxes, gt_classes, gt_count, G, iou_thresh, loss, ws, wx, wy, ww, wh,
    #  cls_agnostic, cls_mode, gamma, stream)
    v = [P, 48, 100, 8, P, P, 2, P, P, P, P, 16, 0.5, P, P, 10.0, 10.0, 5.0, 5.0, 0, 2, 1.5, None]
    refused("sfod_bpc_loss_cls", v, modes + gammas + [("ld", 40), ("K", 0), ("K", 33), ("R", -5), ("ww", -1.0), ("pred", None), ("rois", None),
                                             ("roi_cls", None), ("image_sizes", None), ("gt_boxes", None), ("gt_classes", None),
                                             ("gt_count", None), ("loss", None), ("ws", None)])


def test_cls_entry_points_refuse_broken_arguments_before_any_launch(sfod):
    """From a valid argument list ONE argument is broken at a time: an unknown mode, gamma < 0 or non-finite, K / ld that do not
    fit the layout, a NULL operand -> SFOD_EBADARG with a message, so nothing was launched (no GPU needed)."""
    lib = sfod.native.load()
    protos = sfod.native.parse_header()
    failures = []
    before = lib.sfod_last_error()

    def body():      # sfod_last_error is per thread: the messages provoked here stay out of the other tests' thread
        try:
            _refusals(sfod, lib, protos)
        except BaseException as e:      # noqa: BLE001 -- handed to the test's thread
            failures.append(e)
    th = threading.Thread(target=body)
    th.start()
    th.join()
    if failures:
        raise failures[0]
    assert lib.sfod_last_error() == before
