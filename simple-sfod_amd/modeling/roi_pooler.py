"""ROI pooler options of the box head, read from the config (no device needed).

``MODEL.ROI_BOX_HEAD.{POOLER_TYPE, POOLER_SAMPLING_RATIO, POOLER_RESOLUTION}`` become what the ``sfod_roi_align_*_opt``
kernels take by value: ``aligned`` (Detectron2's ``ROIAlignV2`` is torchvision ``roi_align(aligned=True)``, ``ROIAlign`` is
``aligned=False``), the sampling ratio (0: the adaptive grid) and the pooled size.  Whatever is not built raises a
``ValueError`` that names the key and the accepted values.  ``ROIPool`` is not built: no named config sets it, and a
deterministic argmax backward is a piece of work of its own.  The definition is restated in include/sfod_hip.h.
"""
POOLER_TYPES = {"ROIAlign": False, "ROIAlignV2": True}      # -> aligned
MAX_RESOLUTION = 16          # ROI_MAXP_FWD of csrc/roi_align.hip
MAX_SAMPLING_RATIO = 16      # ROI_MAX_SAMPLING


def _integer(v):
    return isinstance(v, int) and not isinstance(v, bool)


def roi_pooler_options(resolution, sampling_ratio, pooler_type, prefix="MODEL.ROI_BOX_HEAD"):
    """-> (resolution, sampling_ratio, aligned), checked; ``prefix``: the dotted name of the config node, for the messages."""
    if pooler_type not in POOLER_TYPES:
        raise ValueError(f"{prefix}.POOLER_TYPE must be one of {sorted(POOLER_TYPES)}, got {pooler_type!r}")
    if not _integer(sampling_ratio) or not 0 <= sampling_ratio <= MAX_SAMPLING_RATIO:
        raise ValueError(f"{prefix}.POOLER_SAMPLING_RATIO must be an integer in [0, {MAX_SAMPLING_RATIO}] (0: the adaptive "
                         f"grid), got {sampling_ratio!r}")
    if not _integer(resolution) or not 1 <= resolution <= MAX_RESOLUTION:
        raise ValueError(f"{prefix}.POOLER_RESOLUTION must be an integer in [1, {MAX_RESOLUTION}], got {resolution!r}")
    return resolution, sampling_ratio, POOLER_TYPES[pooler_type]


def validate_roi_pooler_cfg(cfg):
    """The box head's pooler keys, checked without building a module."""
    h = cfg.MODEL.ROI_BOX_HEAD
    return roi_pooler_options(h.POOLER_RESOLUTION, h.POOLER_SAMPLING_RATIO, h.POOLER_TYPE)
