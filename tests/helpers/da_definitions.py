"""The domain losses of DA Faster R-CNN as plain torch definitions (``DAFasterRCNN.image_dc_loss`` / ``instance_dc_loss`` /
``consistency_loss`` and the two heads, daod/modeling/meta_arch/da_faster_rcnn.py:228-272, daod/modeling/dann/dann.py:54-155),
usable in float64 and float32; gradients by autograd.  One level: ``assign_boxes_to_levels`` is all zeros and the
``F.interpolate(align_corners=True)`` of ``image_dc_loss`` is the identity, so neither appears.

The one-channel ROIAlign of the consistency loss comes in two forms:

  ``pool="oracle"``    ``oracle.roi_align`` (the plain-C fp32 restatement of torchvision's kernel), then ``avg_pool2d``: what
                       tools/record_da_golden.py serves the reference as ``roi_heads.box_pooler``.  Its values are fp32
                       whatever the surrounding dtype; tests/test_da_host.py pins these definitions to the recorded
                       reference values through it (1e-12 relative in float64).
  ``pool="matrices"``  the interpolation weights of tests/helpers/roi_pooler_definitions.py (coordinates in fp32 as
                       torchvision writes them, weights summed in float64), contracted in the definition's own dtype: a true
                       float64 value, the reference of the GPU tests' error gates.

Weights are dicts ``{"conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias"}`` (image head) and ``{"fc1.weight", ..,
"fc3.bias"}`` (instance head).  Only tests/ and tools/record_da_golden.py import this module.
"""
import torch
import torch.nn.functional as F

from helpers import roi_pooler_definitions as RP


class _GradientScalar(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, alpha):
        ctx.alpha = alpha
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.alpha, None


def gradient_scalar(x, alpha):
    return _GradientScalar.apply(x, alpha)


def gate(ref64, val32, s):
    """4 x max(torch-fp32's distance from float64, 2^-24 * s) -> (gate, e32); tests/helpers/box_reg_definitions.py"""
    e32 = (val32.double() - ref64.double()).abs().max().item()
    return 4.0 * max(e32, 2.0 ** -24 * float(s)), e32


# ---- the heads ---------------------------------------------------------------------------------------------------------------
def img_head(x, w):
    """x [B, C, H, W] -> logits [B, 1, H, W]"""
    return F.conv2d(F.relu(F.conv2d(x, w["conv1.weight"], w["conv1.bias"])), w["conv2.weight"], w["conv2.bias"])


def ins_head(x, w, masks=None):
    """x [R, D] -> logits [R, 1]; ``masks``: the two dropout masks (0/1, [R, 1024]; kept values are doubled: p = 0.5) or None"""
    h = F.relu(F.linear(x, w["fc1.weight"], w["fc1.bias"]))
    if masks is not None:
        h = h * masks[0].to(h.dtype) * 2.0
    h = F.relu(F.linear(h, w["fc2.weight"], w["fc2.bias"]))
    if masks is not None:
        h = h * masks[1].to(h.dtype) * 2.0
    return F.linear(h, w["fc3.weight"], w["fc3.bias"])


# ---- the loss kernels' definitions ---------------------------------------------------------------------------------------
def bce_terms(z, label):
    """max(z, 0) - z t + log1p(exp(-|z|)) per element"""
    return F.binary_cross_entropy_with_logits(z, torch.full_like(z, float(label)), reduction="none")


def bce(z, label, live=None):
    """-> (mean over the live elements, the same mean of the absolute terms); no live element: 0"""
    t = bce_terms(z, label)
    if live is not None:
        t = t[live]
    n = max(t.numel(), 1)
    return t.sum() / n, t.abs().sum() / n


def pooled_mean(prob, rois, pooled, scale, sampling_ratio=0, aligned=True, pool="matrices"):
    """prob [B, 1, H, W], rois [R, 5] (live rows only) -> [R]: the mean over the pooled x pooled bins of ROIAlign(prob)"""
    if pool == "oracle":
        from oracle import roi_align as ora
        out = ora.roi_align(prob, rois, pooled, scale, sampling_ratio, aligned).to(prob.dtype)
        return F.avg_pool2d(out, kernel_size=pooled, stride=pooled).reshape(-1)
    B, _, H, W = prob.shape
    m = RP.roi_align_matrices_opt(rois, H, W, pooled, scale, sampling_ratio, aligned)
    wy = (m.Ay.sum(1) / (m.count * float(pooled * pooled))[:, None]).to(prob.dtype)
    wx = m.Ax.sum(1).to(prob.dtype)
    return torch.einsum("rh,rhw,rw->r", wy, prob[:, 0][m.batch], wx)


def consistency(z_img, z_ins, rois, pooled, scale, sampling_ratio=0, aligned=True, pool="matrices"):
    """z_img [B, H, W], z_ins [R], rois [R, 5] (padding rows: batch index < 0) -> (mean_live |p_img - p_ins|, the same mean
    (its terms are absolute already), p_img - p_ins of the live rows); no live ROI: 0 (torch's l1_loss gives NaN)"""
    live = rois[:, 0] >= 0
    p_img = pooled_mean(torch.sigmoid(z_img)[:, None], rois[live], pooled, scale, sampling_ratio, aligned, pool)
    d = p_img.to(z_ins.dtype) - torch.sigmoid(z_ins[live])
    loss = d.abs().sum() / max(d.numel(), 1)
    return loss, loss.detach(), d


# ---- DAFasterRCNN's three methods ------------------------------------------------------------------------------------------
def image_dc_loss(feat, w_img, label, w_i):
    z = img_head(gradient_scalar(feat, -1.0 * w_i), w_img)
    return bce(z, label)[0]


def instance_dc_loss(box_features, w_ins, label, w_n, masks=None, live=None):
    z = ins_head(gradient_scalar(box_features, -1.0 * w_n), w_ins, masks)
    return bce(z[:, 0], label, live)[0]


def consistency_loss(feat, box_features, rois, w_img, w_ins, w_i, w_n, w_c, pooled, scale, sampling_ratio=0, aligned=True,
                     masks=None, pool="matrices"):
    z_img = img_head(gradient_scalar(feat, w_c * w_i), w_img)[:, 0]
    z_ins = ins_head(gradient_scalar(box_features, w_c * w_n), w_ins, masks)[:, 0]
    return consistency(z_img, z_ins, rois, pooled, scale, sampling_ratio, aligned, pool)[0]


def box_head(feat, rois, w_box, pooled, scale, sampling_ratio=0, aligned=True):
    """the named yamls' 2-FC box head on the live rois: oracle ROIAlign -> flatten (C, H, W) -> fc1, ReLU -> fc2, ReLU.
    (``oracle.roi_align`` is fp32: the box features of a float64 evaluation carry its rounding, as the recorded ones do)"""
    from oracle import roi_align as ora
    x = ora.roi_align(feat, rois, pooled, scale, sampling_ratio, aligned).to(feat.dtype).flatten(1)
    h = F.relu(F.linear(x, w_box["fc1.weight"], w_box["fc1.bias"]))
    return F.relu(F.linear(h, w_box["fc2.weight"], w_box["fc2.bias"]))


def evaluate_losses(feat, box_features, rois, w_img, w_ins, weights, label, pooler, masks, pool="matrices", extra_leaves=None):
    """The three loss methods on one domain, each with its own autograd gradients -> {which: (value, {leaf name: gradient})}
    for which in img / ins / cons; leaf names as tools/record_da_golden.py writes them (``feat``, ``box_features``,
    ``w_img/conv1.weight`` .., ``w_ins/fc1.weight`` .., and ``extra_leaves``).  ``feat`` and the weights must require grad;
    ``box_features`` [R, D] is a leaf or a function of ``feat``; ``masks``: ((ins fc1, ins fc2), (cons fc1, cons fc2)) or
    None (eval mode)."""
    w_i, w_n, w_c = weights
    pooled, sr, aligned = pooler
    live = rois[:, 0] >= 0
    scale = 1.0 / 32
    leaves = {"feat": feat, "box_features": box_features}
    leaves.update({"w_img/" + k: v for k, v in w_img.items()})
    leaves.update({"w_ins/" + k: v for k, v in w_ins.items()})
    leaves.update(extra_leaves or {})
    losses = {
        "img": lambda: image_dc_loss(feat, w_img, label, w_i),
        "ins": lambda: instance_dc_loss(box_features, w_ins, label, w_n, masks[0] if masks is not None else None, live),
        "cons": lambda: consistency_loss(feat, box_features, rois.to(feat.dtype), w_img, w_ins, w_i, w_n, w_c, pooled, scale, sr,
                                         aligned, masks[1] if masks is not None else None, pool)}
    out = {}
    for which, fn in losses.items():
        loss = fn()
        grads = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True, retain_graph=True)
        out[which] = (loss.detach(), {n: g for n, g in zip(leaves, grads) if g is not None})
    return out
