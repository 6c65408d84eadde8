"""Architecture options of the box head, read from the config (no device needed).

``MODEL.ROI_BOX_HEAD.{NUM_CONV, CONV_DIM, NUM_FC, FC_DIM, NORM}`` mean what they mean in Detectron2's ``FastRCNNConvFCHead``:
NUM_CONV 3x3 convolutions of CONV_DIM channels (pad 1, ``bias = not norm``, the norm at ``conv{k}.norm``, ReLU), the result
flattened in (C, H, W) order, then NUM_FC linear layers of FC_DIM with ReLU.  Built: counts in [0, 4] with at least one
layer, widths that are positive multiples of 8 (the 8-channel groups of the pair storage; with NUM_CONV > 0 CONV_DIM is
8 x a power of two up to 1024, the input widths of the 3x3 convolution kernels -- a limit to lift by padding a layer's output), NORM "" or "GN" =
``torch.nn.GroupNorm(32, CONV_DIM)`` with eps 1e-5 (Detectron2's ``get_norm``; CONV_DIM then a multiple of 32).  Whatever is
not built raises a ``ValueError`` that names the key and the accepted values.  BatchNorm variants are not built on purpose:
the ROI tensors carry all-zero padding rows, which would enter a batch statistic; GroupNorm is per ROI.  The kernels'
definition is restated in include/sfod_hip.h (sfod_group_norm_relu_fwd / _bwd).
"""
NORMS = ("", "GN")
MAX_LAYERS = 4
GN_GROUPS = 32
GN_EPS = 1e-5


def _integer(v):
    return isinstance(v, int) and not isinstance(v, bool)


class BoxHeadOptions:
    """``num_conv`` x conv3x3(``conv_dim``) [+ GroupNorm] + ReLU, then ``num_fc`` x linear(``fc_dim``) + ReLU."""
    __slots__ = ("num_conv", "conv_dim", "num_fc", "fc_dim", "norm")

    def __init__(self, num_conv=0, conv_dim=256, num_fc=2, fc_dim=1024, norm=""):
        self.num_conv, self.conv_dim, self.num_fc, self.fc_dim, self.norm = num_conv, conv_dim, num_fc, fc_dim, norm

    def is_default(self):
        """the named yamls' head: two linear layers, nothing else (``StandardROIHeads`` keeps its own pass for it)"""
        return self.num_conv == 0 and self.num_fc == 2

    def __repr__(self):
        return (f"BoxHeadOptions(num_conv={self.num_conv}, conv_dim={self.conv_dim}, num_fc={self.num_fc}, "
                f"fc_dim={self.fc_dim}, norm={self.norm!r})")


def box_head_options(cfg, prefix="MODEL.ROI_BOX_HEAD"):
    h = cfg.MODEL.ROI_BOX_HEAD
    num_conv, num_fc, conv_dim, fc_dim, norm = h.NUM_CONV, h.NUM_FC, h.CONV_DIM, h.FC_DIM, h.NORM
    for key, v in (("NUM_CONV", num_conv), ("NUM_FC", num_fc)):
        if not _integer(v) or not 0 <= v <= MAX_LAYERS:
            raise ValueError(f"{prefix}.{key} must be an integer in [0, {MAX_LAYERS}], got {v!r}")
    if num_conv + num_fc < 1:
        raise ValueError(f"{prefix}.NUM_CONV + {prefix}.NUM_FC must be at least 1 (a box head has a layer), got "
                         f"{num_conv} + {num_fc}")
    for key, v in (("CONV_DIM", conv_dim), ("FC_DIM", fc_dim)):
        if not _integer(v) or v <= 0 or v % 8:
            raise ValueError(f"{prefix}.{key} must be a positive multiple of 8 (the 8-channel groups of the operand "
                             f"storage), got {v!r}")
    if norm not in NORMS:
        raise ValueError(f"{prefix}.NORM must be one of {list(NORMS)} (\"GN\": GroupNorm(32, CONV_DIM), eps 1e-5; the "
                         f"BatchNorm variants and LN are not built: padding ROIs would enter a batch statistic), got {norm!r}")
    if norm == "GN" and num_conv > 0 and conv_dim % GN_GROUPS:
        raise ValueError(f"{prefix}.CONV_DIM must be a multiple of {GN_GROUPS} under {prefix}.NORM \"GN\" (GroupNorm with "
                         f"{GN_GROUPS} groups), got {conv_dim!r}")
    if num_conv > 0 and (conv_dim // 8) & (conv_dim // 8 - 1):
        raise ValueError(f"{prefix}.CONV_DIM must be 8 x a power of two (8, 16, 32, ..., 1024: what the 3x3 convolution kernels "
                         f"take as an input width), got {conv_dim!r}")
    if num_conv > 0 and conv_dim > 1024:
        raise ValueError(f"{prefix}.CONV_DIM must be at most 1024 (the GroupNorm kernels' channel limit), got {conv_dim!r}")
    return BoxHeadOptions(num_conv, conv_dim, num_fc, fc_dim, norm)


def validate_box_head_cfg(cfg):
    """The five keys, and what the instance-level domain branch needs of them, checked without building a module."""
    opts = box_head_options(cfg)
    check_instance_branch(cfg, opts)
    return opts


def check_instance_branch(cfg, opts):
    """The instance-level domain discriminator (``DAInsHead``) reads the box head's flat FC features: a head without an FC
    layer cannot feed it."""
    ins_dc = bool(cfg.SEMISUPNET.INS_DC) if "SEMISUPNET" in cfg else False
    instance = bool(cfg.DOMAIN_CLASSIFIER.INSTANCE) if "DOMAIN_CLASSIFIER" in cfg and "INSTANCE" in cfg.DOMAIN_CLASSIFIER else False
    if opts.num_fc == 0 and (ins_dc or instance):
        raise ValueError("MODEL.ROI_BOX_HEAD.NUM_FC must be >= 1 when the instance-level domain branch can run "
                         f"(SEMISUPNET.INS_DC {ins_dc}, DOMAIN_CLASSIFIER.INSTANCE {instance}): DAInsHead takes the box "
                         "head's FC features, got NUM_FC 0")
