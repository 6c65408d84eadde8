"""Box-regression options of the two detection heads, read from the config (no device needed).

``MODEL.RPN.{BBOX_REG_LOSS_TYPE, SMOOTH_L1_BETA, BBOX_REG_WEIGHTS}`` and
``MODEL.ROI_BOX_HEAD.{BBOX_REG_LOSS_TYPE, SMOOTH_L1_BETA, BBOX_REG_WEIGHTS, CLS_AGNOSTIC_BBOX_REG, BBOX_REG_LOSS_WEIGHT}``
become a ``native.BoxRegOptions`` (what the ``sfod_*_opt`` kernels take by value); whatever is not built raises a
``ValueError`` that names the key and the accepted values.  Detectron2's definitions (``_dense_box_regression_loss``,
``FastRCNNOutputLayers.box_reg_loss``, fvcore ``smooth_l1_loss`` / ``giou_loss``) are restated in include/sfod_hip.h.
"""
import math

from .. import native

RPN_DEFAULT_WEIGHTS = (1.0, 1.0, 1.0, 1.0)
ROI_DEFAULT_WEIGHTS = (10.0, 10.0, 5.0, 5.0)
LOSS_TYPES = tuple(sorted(native.BOX_REG_LOSS_TYPES))      # d2 also knows "diou" / "ciou": not built


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


def box_reg_options(node, prefix, cls_agnostic=False):
    """``node``: cfg.MODEL.RPN or cfg.MODEL.ROI_BOX_HEAD; ``prefix``: its dotted name, for the messages."""
    loss_type = node.BBOX_REG_LOSS_TYPE
    if loss_type not in LOSS_TYPES:
        raise ValueError(f"{prefix}.BBOX_REG_LOSS_TYPE must be one of {list(LOSS_TYPES)}, got {loss_type!r}")
    beta = node.SMOOTH_L1_BETA
    if not _number(beta) or beta < 0:
        raise ValueError(f"{prefix}.SMOOTH_L1_BETA must be a finite number >= 0, got {beta!r}")
    weights = node.BBOX_REG_WEIGHTS
    if not isinstance(weights, (tuple, list)) or len(weights) != 4 or not all(_number(w) and w > 0 for w in weights):
        raise ValueError(f"{prefix}.BBOX_REG_WEIGHTS must be four finite numbers > 0 (wx, wy, ww, wh), got {weights!r}")
    if not isinstance(cls_agnostic, bool):
        raise ValueError(f"{prefix}.CLS_AGNOSTIC_BBOX_REG must be True or False, got {cls_agnostic!r}")
    return native.BoxRegOptions(weights, loss_type, beta, cls_agnostic)


def rpn_box_reg_options(cfg):
    return box_reg_options(cfg.MODEL.RPN, "MODEL.RPN")


def roi_box_reg_options(cfg):
    """-> (BoxRegOptions, loss_box_reg weight) of the Fast R-CNN output layers"""
    h = cfg.MODEL.ROI_BOX_HEAD
    opts = box_reg_options(h, "MODEL.ROI_BOX_HEAD", h.CLS_AGNOSTIC_BBOX_REG)
    w = h.BBOX_REG_LOSS_WEIGHT
    if not _number(w) or w < 0:
        raise ValueError(f"MODEL.ROI_BOX_HEAD.BBOX_REG_LOSS_WEIGHT must be a finite number >= 0, got {w!r}")
    return opts, float(w)


def validate_box_reg_cfg(cfg):
    """Both heads' options, checked without building a module (setup_cfg calls it)."""
    rpn_box_reg_options(cfg)
    roi_box_reg_options(cfg)
