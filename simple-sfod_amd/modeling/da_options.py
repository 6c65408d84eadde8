"""Options of ``TRAINER "da"`` / ``DAFasterRCNN`` (DA Faster R-CNN, Chen et al. 2018) and its conditional variant
``CDAFasterRCNN``, read from the config (no device needed).

``DA_FASTER.{DC_IMG_GRL_WEIGHT, DC_INS_GRL_WEIGHT, DC_CONSISTENCY_WEIGHT, LEVELS, ENTROPY_CONDITIONING}`` mean what they mean
in the reference's ``DAFasterRCNN`` (daod/modeling/meta_arch/da_faster_rcnn.py): the image-level and the instance-level
domain classifier see the features through gradient-scalar layers of ``-DC_IMG_GRL_WEIGHT`` / ``-DC_INS_GRL_WEIGHT``, the
consistency term through ``DC_CONSISTENCY_WEIGHT`` times those.  Built: ONE level, which is the feature the ROI heads pool
(there is no FPN here).  With one level

  * ``assign_boxes_to_levels`` is all zeros: every ROI goes through the one ``DAInsHead`` branch, and
  * the ``F.interpolate(size=(H, W), mode="bilinear", align_corners=True)`` of ``image_dc_loss``, which resizes every level's
    logit map to the first level's size, is the identity.

``CDAFasterRCNN`` (daod/modeling/meta_arch/cda_faster_rcnn.py, with ``CDAStandardROIHeads``) reads the same keys and
``ENTROPY_CONDITIONING``: its instance-level classifier sees the outer product of the box features and the detached class
probabilities, each ROI weighted by ``1 + exp(-entropy)`` of its prediction when the key is True.

Whatever is not built raises a ``ValueError`` that names the key.
"""
import math

from .box_head_options import box_head_options

WEIGHT_KEYS = ("DC_IMG_GRL_WEIGHT", "DC_INS_GRL_WEIGHT", "DC_CONSISTENCY_WEIGHT")
ARCH_HEADS = {"DAFasterRCNN": "DAStandardROIHeads", "CDAFasterRCNN": "CDAStandardROIHeads"}      # what TRAINER "da" builds


class DAOptions:
    """``level``: the one feature both domain classifiers read; the three weights as python floats; ``conditional``: the
    CDA architecture (class-conditioned instance-level classifier), ``entropy_conditioning``: its per-ROI entropy weights."""
    __slots__ = ("level", "img_weight", "ins_weight", "consistency_weight", "conditional", "entropy_conditioning")

    def __init__(self, level, img_weight, ins_weight, consistency_weight, conditional=False, entropy_conditioning=False):
        self.level = level
        self.img_weight, self.ins_weight, self.consistency_weight = float(img_weight), float(ins_weight), float(consistency_weight)
        self.conditional, self.entropy_conditioning = bool(conditional), bool(entropy_conditioning)

    def __repr__(self):
        return (f"DAOptions(level={self.level!r}, img_weight={self.img_weight}, ins_weight={self.ins_weight}, "
                f"consistency_weight={self.consistency_weight}, conditional={self.conditional}, "
                f"entropy_conditioning={self.entropy_conditioning})")


def validate_da_trainer_cfg(cfg):
    """``TRAINER "da"`` feeds ``(source, target)`` tuples: only ``DAFasterRCNN`` and ``CDAFasterRCNN`` take them."""
    arch = cfg.MODEL.META_ARCHITECTURE
    if arch not in ARCH_HEADS:
        raise ValueError(f"MODEL.META_ARCHITECTURE must be 'DAFasterRCNN' or 'CDAFasterRCNN' under TRAINER 'da' (its loader "
                         f"yields (source, target) batches), got {arch!r}")
    return da_options(cfg)


def da_options(cfg, backbone_features=None):
    """``backbone_features``: names of the features the built backbone produces (None: not checked here)."""
    d = cfg.DA_FASTER
    heads = cfg.MODEL.ROI_HEADS.NAME
    conditional = cfg.MODEL.META_ARCHITECTURE == "CDAFasterRCNN"
    if conditional and heads != "CDAStandardROIHeads":
        raise ValueError(f"MODEL.ROI_HEADS.NAME must be 'CDAStandardROIHeads' under CDAFasterRCNN (it returns the box features "
                         f"and the class logits, and samples unlabeled proposals), got {heads!r}")
    if not conditional and heads != "DAStandardROIHeads":
        raise ValueError(f"MODEL.ROI_HEADS.NAME must be 'DAStandardROIHeads' under DAFasterRCNN (it returns the box features and "
                         f"samples unlabeled proposals), got {heads!r}")
    levels = d.LEVELS
    if not isinstance(levels, (list, tuple)) or len(levels) != 1 or not isinstance(levels[0], str):
        raise ValueError(f"DA_FASTER.LEVELS must name exactly one feature (no FPN is built), got {levels!r}")
    pooled = list(cfg.MODEL.ROI_HEADS.IN_FEATURES)
    if levels[0] != pooled[0]:
        raise ValueError(f"DA_FASTER.LEVELS must be the feature the ROI heads pool, MODEL.ROI_HEADS.IN_FEATURES[0] = "
                         f"{pooled[0]!r}, got {list(levels)!r}")
    if backbone_features is not None and levels[0] not in backbone_features:
        raise ValueError(f"DA_FASTER.LEVELS must name a feature the backbone produces ({sorted(backbone_features)}), got "
                         f"{list(levels)!r}")
    entropy = d.ENTROPY_CONDITIONING
    if conditional:
        if not isinstance(entropy, bool):
            raise ValueError(f"DA_FASTER.ENTROPY_CONDITIONING must be True or False, got {entropy!r}")
    elif entropy:
        raise ValueError("DA_FASTER.ENTROPY_CONDITIONING must be False (only the CDA architecture reads it, which is not built), "
                         "got True")
    vals = []
    for key in WEIGHT_KEYS:
        v = d[key]
        if not isinstance(v, (int, float)) or isinstance(v, bool) or not math.isfinite(v) or v < 0:
            raise ValueError(f"DA_FASTER.{key} must be a finite number >= 0, got {v!r}")
        vals.append(v)
    if cfg.MODEL.ROI_BOX_HEAD.NAME == "FastRCNNConvFCHead" and box_head_options(cfg).num_fc == 0:
        raise ValueError("MODEL.ROI_BOX_HEAD.NUM_FC must be >= 1 under DAFasterRCNN: DAInsHead takes the box head's FC "
                         "features, got NUM_FC 0")
    return DAOptions(levels[0], *vals, conditional=conditional, entropy_conditioning=conditional and entropy)
