"""Proposal and matcher options, read from the config (no device needed).

``MODEL.ANCHOR_GENERATOR.OFFSET``, ``MODEL.RPN.BOUNDARY_THRESH``, ``MODEL.PROPOSAL_GENERATOR.MIN_SIZE`` and
``MODEL.ROI_HEADS.{IOU_THRESHOLDS, IOU_LABELS}`` become what the ``sfod_rpn_decode_shift`` / ``sfod_anchor_match_opt`` /
``sfod_rpn_loss_shift`` / ``sfod_rpn_gather_topk_opt`` / ``sfod_roi_match_opt`` entry points take by value; whatever is not
built -- another anchor generator or RPN head, extra RPN convolutions, a matcher of another shape -- raises a ``ValueError``
that names the key and the accepted values.  Detectron2's definitions (``_create_grid_offsets``, ``Boxes.inside_box``,
``Boxes.nonempty``, ``Matcher`` + ``_sample_proposals``) are restated in include/sfod_hip.h.
"""
import math


def _number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


class ProposalOptions:
    """``offset`` (anchor grid shift in strides), ``boundary_thresh`` (-1.0: off), ``min_size`` of the RPN."""
    __slots__ = ("offset", "boundary_thresh", "min_size")

    def __init__(self, offset=0.0, boundary_thresh=-1.0, min_size=0.0):
        self.offset, self.boundary_thresh, self.min_size = float(offset), float(boundary_thresh), float(min_size)

    def is_default(self):
        return self.offset == 0.0 and self.boundary_thresh < 0 and self.min_size == 0.0

    def shift(self, stride):
        """what the kernels add to ``x * stride``: the double product, rounded to float32 once at the call"""
        return self.offset * stride

    def __repr__(self):
        return f"ProposalOptions(offset={self.offset}, boundary_thresh={self.boundary_thresh}, min_size={self.min_size})"


def proposal_options(cfg):
    m = cfg.MODEL
    name = m.ANCHOR_GENERATOR.NAME
    if name != "DefaultAnchorGenerator":
        raise ValueError(f"MODEL.ANCHOR_GENERATOR.NAME must be 'DefaultAnchorGenerator' (rotated anchors are not built), got {name!r}")
    head = m.RPN.HEAD_NAME
    if head != "StandardRPNHead":
        raise ValueError(f"MODEL.RPN.HEAD_NAME must be 'StandardRPNHead', got {head!r}")
    conv_dims = m.RPN.CONV_DIMS
    if not isinstance(conv_dims, (tuple, list)) or list(conv_dims) != [-1]:
        raise ValueError(f"MODEL.RPN.CONV_DIMS must be [-1] (one 3x3 convolution of the input's width), got {conv_dims!r}")
    offset = m.ANCHOR_GENERATOR.OFFSET
    if not _number(offset) or not 0.0 <= offset < 1.0:
        raise ValueError(f"MODEL.ANCHOR_GENERATOR.OFFSET must be a number in [0, 1), got {offset!r}")
    bt = m.RPN.BOUNDARY_THRESH
    if not _number(bt) or not (bt == -1 or bt >= 0):
        raise ValueError(f"MODEL.RPN.BOUNDARY_THRESH must be -1 (off) or a finite number >= 0, got {bt!r}")
    ms = m.PROPOSAL_GENERATOR.MIN_SIZE
    if not _number(ms) or ms < 0:
        raise ValueError(f"MODEL.PROPOSAL_GENERATOR.MIN_SIZE must be a finite number >= 0, got {ms!r}")
    return ProposalOptions(offset, bt, ms)


def roi_iou_band(cfg):
    """MODEL.ROI_HEADS.IOU_THRESHOLDS / IOU_LABELS -> (lo, hi): ``[t]`` / ``[0, 1]`` gives (t, t), the one-threshold matcher;
    ``[lo, hi]`` / ``[0, -1, 1]`` gives the band whose ROIs are ignored (class -1, never sampled)."""
    r = cfg.MODEL.ROI_HEADS
    thr, lab = r.IOU_THRESHOLDS, r.IOU_LABELS
    ok = isinstance(thr, (tuple, list)) and isinstance(lab, (tuple, list)) and all(_number(t) for t in thr)
    if ok and len(thr) == 1 and list(lab) == [0, 1]:
        return float(thr[0]), float(thr[0])
    if ok and len(thr) == 2 and list(lab) == [0, -1, 1] and thr[0] <= thr[1]:
        return float(thr[0]), float(thr[1])
    raise ValueError("MODEL.ROI_HEADS.IOU_THRESHOLDS / MODEL.ROI_HEADS.IOU_LABELS must be [t] / [0, 1] or [lo, hi] / [0, -1, 1] "
                     f"with lo <= hi, got {thr!r} / {lab!r}")


def validate_proposal_cfg(cfg):
    """Every key above, checked without building a module."""
    proposal_options(cfg)
    roi_iou_band(cfg)
