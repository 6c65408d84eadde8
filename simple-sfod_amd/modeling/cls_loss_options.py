"""Classification-loss options of the Fast R-CNN head, read from the config (no device needed).

``MODEL.ROI_HEADS.LOSS`` ("CrossEntropy" / "FocalLoss"), ``SFOD.FOCAL_LOSS_GAMMA`` and ``MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE``
become a ``native.ClsLossOptions`` (what the ``sfod_*_cls`` kernels take by value); whatever is not built raises a
``ValueError`` that names the key.  The definitions -- Unbiased Teacher's ``FastRCNNFocalLoss`` (the branch the reference's
three ROI-heads files carry commented out, e.g. source_free_adaptive_teacher_roi_heads.py:19,56-57) and Detectron2's
``FastRCNNOutputLayers`` with its sigmoid cross-entropy -- are restated in include/sfod_hip.h (sfod_frcnn_loss_cls) and, in torch
ops, in tests/helpers/cls_loss_definitions.py.
"""
import math

from .. import native

ROI_LOSSES = tuple(sorted(native.CLS_LOSS_KINDS))
# the ROI heads whose ``_init_box_head`` reads MODEL.ROI_HEADS.LOSS in the reference; the others build FastRCNNOutputLayers
# whatever the key says
FOCAL_ROI_HEADS = ("SourceFreeAdaptiveTeacherStandardROIHeads", "AdaptiveTeacherStandardROIHeads")
SOFTMAX_ONLY_META_ARCH = ("CDAFasterRCNN",)      # its class conditioning is defined on softmax probabilities


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


def _get(cfg, dotted, default):
    """a key that only some trainers' config blocks declare (MODEL.ROI_HEADS.LOSS: the semi-supervised ones)"""
    node = cfg
    for part in dotted.split("."):
        if part not in node:
            return default
        node = node[part]
    return node


def cls_loss_options(cfg, roi_heads_name=None):
    """-> ``native.ClsLossOptions``; ``roi_heads_name`` (default MODEL.ROI_HEADS.NAME): the class that is being built"""
    kind = _get(cfg, "MODEL.ROI_HEADS.LOSS", "CrossEntropy")
    if kind not in ROI_LOSSES:
        raise ValueError(f"MODEL.ROI_HEADS.LOSS must be one of {list(ROI_LOSSES)}, got {kind!r}")
    rpn = _get(cfg, "MODEL.RPN.LOSS", "CrossEntropy")
    if rpn != "CrossEntropy":
        raise ValueError(f"MODEL.RPN.LOSS must be 'CrossEntropy' (the reference has no other RPN loss), got {rpn!r}")
    sigmoid = cfg.MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE
    if not isinstance(sigmoid, bool):
        raise ValueError(f"MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE must be True or False, got {sigmoid!r}")
    fed = cfg.MODEL.ROI_BOX_HEAD.USE_FED_LOSS
    if fed is not False:
        raise ValueError(f"MODEL.ROI_BOX_HEAD.USE_FED_LOSS must be False (the federated loss needs dataset class "
                         f"frequencies: not built), got {fed!r}")
    gamma = cfg.SFOD.FOCAL_LOSS_GAMMA
    if not _number(gamma) or gamma < 0:
        raise ValueError(f"SFOD.FOCAL_LOSS_GAMMA must be a finite number >= 0, got {gamma!r}")
    if kind == "FocalLoss" and sigmoid:
        raise ValueError("MODEL.ROI_HEADS.LOSS 'FocalLoss' and MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE True exclude each other "
                         "(the focal loss is defined on the softmax cross-entropy)")
    name = roi_heads_name if roi_heads_name is not None else cfg.MODEL.ROI_HEADS.NAME
    if kind == "FocalLoss" and name not in FOCAL_ROI_HEADS:
        raise ValueError(f"MODEL.ROI_HEADS.LOSS 'FocalLoss' is read by {list(FOCAL_ROI_HEADS)} only; MODEL.ROI_HEADS.NAME "
                         f"{name!r} trains with 'CrossEntropy'")
    if sigmoid and cfg.MODEL.META_ARCHITECTURE in SOFTMAX_ONLY_META_ARCH:
        raise ValueError(f"MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE True: MODEL.META_ARCHITECTURE {cfg.MODEL.META_ARCHITECTURE!r} "
                         "conditions on softmax class probabilities")
    return native.ClsLossOptions(kind, gamma, sigmoid)


def native_cls_loss(cfg, roi_heads_name=None):
    """what the native calls take: None = today's entry points (every key at its default)"""
    o = cls_loss_options(cfg, roi_heads_name)
    return None if o.is_default() else o
