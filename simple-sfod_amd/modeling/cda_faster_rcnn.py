"""Conditional DA Faster R-CNN: ``CDAFasterRCNN`` with ``CDAStandardROIHeads`` behind ``TRAINER "da"``.

Mirrors the reference's ``daod/modeling/meta_arch/cda_faster_rcnn.py:22-300`` and ``daod/modeling/roi_heads/cda_roi_heads.py``
(the heads live in modeling/roi_heads.py beside the others).  It is ``DAFasterRCNN`` (modeling/da_faster_rcnn.py: ``DARPN``,
``DAImgHead``, the loader, the trainer and the image-level terms are that module's, unchanged) with a class-conditioned
instance-level classifier:

  * ``DC_ins`` reads ``multilinear_map(box_features, softmax(box_scores).detach())`` [R, (K + 1) * D], element
    ``c * D + d`` = p[r, c] * f[r, d]; its fc1 is a (K + 1) * D -> 1024 layer (``DC_ins.da_ins_fc1_level_<level>.weight``
    [1024, D * (K + 1)], the reference's key and shape).
  * ``DA_FASTER.ENTROPY_CONDITIONING``: ``conditional_instance_dc_loss`` weights each ROI's BCE term by
    ``w = 1 + exp(-entropy(p))``, divided by the mean weight; ``conditional_consistency_loss`` is not weighted.

``_CDADomainFn`` is ``_DADomainFn`` with that classifier.  The conditioned feature is 9 x the box features (151 MB per domain
at the yaml's shapes in bf16x3), so it is formed ONCE per domain by ``sfod_cda_condition_fwd`` (csrc/cda_condition.hip),
written directly as the GEMM operand, and fc1 + ReLU is evaluated once: the reference's two ``DAInsHead`` evaluations share
the input and fc1, and their dropout comes behind fc1's ReLU, so they differ only from there on (own masks, in the unchanged
``MASK_ORDER``).  Backward: fc2 / fc3 per evaluation; at fc1 the parameters take ``d1_ins + d1_cons`` (one weight-gradient
product over the conditioned feature), the input ``-w_n * d1_ins + w_c * w_n * d1_cons`` (one data-gradient product), then
``sfod_cda_condition_bwd`` contracts the classes away.  The same values as two evaluations, up to the rounding of the sums
(tests/test_cda_host.py holds the algebra in float64).  The condition is detached: no gradient reaches the class logits.
"""
import torch
import torch.nn as nn

from .. import native
from ..registry import META_ARCH_REGISTRY
from .da_faster_rcnn import DAFasterRCNN, _predictor_backward, _scalar
from .dann import ins_head_layers
from .roi_heads import CDAStandardROIHeads, _cls_kw  # noqa: F401  (the ROI heads of this architecture live beside the others)


class MultiLinearMap(nn.Module):
    """The reference's parameter-free module (cda_faster_rcnn.py:22-33), kept so that the module tree matches; it adds no
    state-dict key.  The training step forms the map inside ``_CDADomainFn`` (``native.cda_condition_fwd``, from the logits)."""

    def forward(self, f, g):
        raise NotImplementedError("the conditioned features are written by sfod_cda_condition_fwd from the class logits "
                                  "(native.cda_condition_fwd); this module only mirrors the reference's module tree")


def _ins_tail_logits(head, r1, masks, dtype):
    """``DAInsHead`` behind fc1's ReLU ``r1`` [R, 1024]: dropout, fc2, ReLU, dropout, fc3 -> the state ``ins_head_logits`` makes"""
    dt = native.dt_of_dtype(dtype)
    _, fc2, fc3 = ins_head_layers(head)
    z1 = native.mul_mask_(r1.clone(), masks[0], 2.0) if masks is not None else r1
    r2 = native.conv_fwd(z1, native.pack_fc_weight(fc2.weight.detach(), dt), fc2.bias.detach(), 1024, 1, act=1)
    z2 = native.mul_mask_(r2.clone(), masks[1], 2.0) if masks is not None else r2
    z = native.conv_fwd(z2, native.pack_fc_weight(fc3.weight.detach(), dt), fc3.bias.detach(), 1, 1,
                        out_dtype=torch.float32, ldy=8)
    return {"r1": r1, "z1": z1, "r2": r2, "z2": z2, "z": z, "masks": masks}


def _ins_tail_backward(head, ev, dz, compute_dtype):
    """``dz`` fp32 [R, 8] -> (d1: the gradient of fc1's pre-activation [R, 1024], [dw2, db2, dw3, db3]); the steps of
    ``ins_head_backward`` down to fc1"""
    dtype = native.grad_dtype_of(compute_dtype)
    dt = native.dt_of_dtype(dtype)
    _, fc2, fc3 = ins_head_layers(head)
    masks = ev["masks"]
    dzc = native.cast(dz, dtype)
    dw3 = native.conv_wgrad(ev["z2"], dzc, 1, 1, operand=dtype).view(1, -1)
    db3 = native.bias_grad(dz, 1)
    d2 = native.conv_fwd(dzc, native.pack_fc_weight(fc3.weight.detach(), dt, transpose=True, ld=8), None, 1024, 1)
    if masks is not None:
        native.mul_mask_(d2, masks[1], 2.0)
    native.act_bwd_(d2, ev["r2"], 1)
    dw2 = native.conv_wgrad(ev["z1"], d2, 1024, 1, operand=dtype).view(1024, -1)
    db2 = native.bias_grad(d2, 1024)
    d1 = native.conv_fwd(d2, native.pack_fc_weight(fc2.weight.detach(), dt, transpose=True), None, 1024, 1)
    if masks is not None:
        native.mul_mask_(d1, masks[0], 2.0)
    native.act_bwd_(d1, ev["r1"], 1)
    return d1, [dw2, db2, dw3, db3]


class _CDADomainFn(torch.autograd.Function):
    """``_DADomainFn`` with the class-conditioned instance-level classifier: same inputs, same five losses.  ``scores``:
    fp32 class logits [R, >= K + 1] to condition on, or None: the predictor's of this pass (``st["pred"]``)."""

    @staticmethod
    def forward(ctx, model, feat_nchw, samples, labeled, label, masks, scores, *params):
        heads, opts = model.roi_heads, model.da
        dtype = heads.compute_dtype
        dt = native.dt_of_dtype(dtype)
        rois = samples["rois"]
        dev = rois.device
        st = heads._box_forward(feat_nchw, rois)
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        l_cls, l_box = zero, zero.clone()
        if labeled:
            bp = heads.box_predictor
            loss, _ = native.frcnn_loss(st["pred"], heads.num_classes, rois, samples["gt_cls"], samples["gt_box"],
                                        samples["n_valid"], box_reg=bp._box_reg, **_cls_kw(bp))
            ctx.box_w = bp.box_reg_loss_weight
            l_cls, l_box = loss[0].clone(), (loss[1].clone() if ctx.box_w == 1.0 else loss[1] * ctx.box_w)
        # image level: one evaluation of DAImgHead for the BCE term and the consistency term
        x = native.nhwc_operand(feat_nchw, dtype)
        h1, z_img = model.DC_img.logits(x)
        l_img, _ = native.da_bce(z_img, label)
        # instance level: the conditioned feature once, fc1 + ReLU once, then the two evaluations under their own masks
        sc = st["pred"] if scores is None else scores
        xc, xc_grad, p, w = native.cda_condition_fwd(heads.box_features(st), sc, heads.num_classes + 1, rois,
                                                     entropy=opts.entropy_conditioning, out_dtype=dtype, with_grad_operand=True)
        fc1 = ins_head_layers(model.DC_ins)[0]
        r1 = native.conv_fwd(xc, native.pack_fc_weight(fc1.weight.detach(), dt), fc1.bias.detach(), 1024, 1, act=1)
        ev_ins = _ins_tail_logits(model.DC_ins, r1, masks[0] if masks is not None else None, dtype)
        ev_cons = _ins_tail_logits(model.DC_ins, r1, masks[1], dtype) if masks is not None else ev_ins
        if opts.entropy_conditioning:
            l_ins, _ = native.da_bce_weighted(ev_ins["z"], label, w, rois=rois)
        else:
            l_ins, _ = native.da_bce(ev_ins["z"], label, rois=rois)
        pool = heads.box_pooler
        l_cons, cstate = native.da_consistency_fwd(z_img, ev_cons["z"], rois, heads.pooled, pool.scale,
                                                   sampling_ratio=pool.sampling_ratio, aligned=pool.aligned)
        ctx.model, ctx.samples, ctx.labeled, ctx.label = model, samples, labeled, float(label)
        ctx.state = (st, x, h1, z_img, ev_ins, ev_cons, cstate, xc_grad, p, w)
        ctx.feat_dtype = feat_nchw.dtype
        ctx.mark_non_differentiable(*(() if labeled else (l_cls, l_box)))
        return l_cls, l_box, l_img[0].clone(), l_ins[0].clone(), l_cons[0].clone()

    @staticmethod
    def backward(ctx, g_cls, g_box, g_img, g_ins, g_cons):
        model, samples = ctx.model, ctx.samples
        heads, opts = model.roi_heads, model.da
        st, x, h1, z_img, ev_ins, ev_cons, cstate, xc_grad, p, w = ctx.state
        rois = samples["rois"]
        w_i, w_n, w_c = opts.img_weight, opts.ins_weight, opts.consistency_weight
        dtype = native.grad_dtype_of(heads.compute_dtype)
        dt = native.dt_of_dtype(dtype)
        # logit gradients: the three loss kernels
        _, dz_bce = native.da_bce(z_img, ctx.label, grad_scale=_scalar(g_img))
        if opts.entropy_conditioning:
            _, dz_ins = native.da_bce_weighted(ev_ins["z"], ctx.label, w, rois=rois, grad_scale=_scalar(g_ins))
        else:
            _, dz_ins = native.da_bce(ev_ins["z"], ctx.label, rois=rois, grad_scale=_scalar(g_ins))
        dz_cimg, dz_cins = native.da_consistency_bwd(z_img, ev_cons["z"], rois, cstate, _scalar(g_cons))
        # DAImgHead: parameters take both terms unscaled, the feature map what the two gradient-scalar layers pass
        dx_img, img_grads = model.DC_img.grads(x, h1, dz_bce + dz_cimg, dz_bce * (-w_i) + dz_cimg * (w_c * w_i))
        # DAInsHead: fc3 and fc2 per evaluation, parameter gradients summed
        d1_ins, tail_ins = _ins_tail_backward(model.DC_ins, ev_ins, dz_ins, heads.compute_dtype)
        d1_cons, tail_cons = _ins_tail_backward(model.DC_ins, ev_cons, dz_cins, heads.compute_dtype)
        tail_grads = [a + b for a, b in zip(tail_ins, tail_cons)]
        # fc1 once per direction: its parameters take both terms unscaled, its input what the gradient-scalar layers pass
        fc1 = ins_head_layers(model.DC_ins)[0]
        d1_par = d1_ins + d1_cons
        dw1 = native.conv_wgrad(xc_grad, d1_par, 1024, 1, operand=dtype).view(1024, -1)
        db1 = native.bias_grad(d1_par, 1024)
        d1_in = torch.add(d1_ins * (-w_n), d1_cons, alpha=w_c * w_n)
        dxc = native.conv_fwd(d1_in, native.pack_fc_weight(fc1.weight.detach(), dt, transpose=True), None, fc1.in_features, 1)
        dbf = native.cda_condition_bwd(dxc, p, rois)
        pred_grads = [None] * 4
        if ctx.labeled:
            if ctx.box_w != 1.0:
                g_box = g_box * ctx.box_w
            gs = torch.stack([g_cls.reshape(()), g_box.reshape(())]).float().contiguous()
            _, d_pred = native.frcnn_loss(st["pred"], heads.num_classes, rois, samples["gt_cls"], samples["gt_box"],
                                          samples["n_valid"], grad_scale=gs, box_reg=heads.box_predictor._box_reg,
                                          **_cls_kw(heads.box_predictor))
            dh, pred_grads = _predictor_backward(heads, st, d_pred)
            dbf = dbf + dh
        dfeat_roi, head_grads = heads._box_head_backward(st, rois, dbf.contiguous())
        dfeat = (dfeat_roi + dx_img.permute(0, 3, 1, 2)).to(native.out_dtype_of(ctx.feat_dtype))
        ctx.state = None
        return (None, dfeat, None, None, None, None, None, *head_grads, *pred_grads, *img_grads, dw1, db1, *tail_grads)


def cda_domain_losses(model, feat_nchw, samples, labeled, domain_label, masks, scores=None):
    """The five losses of one domain (``_CDADomainFn``) as a tuple; ``masks``: None in eval mode; ``scores``: class logits to
    condition on instead of the predictor's (they are detached either way)."""
    c1, c2 = model.DC_img.convs()
    fcs = ins_head_layers(model.DC_ins)
    params = model.roi_heads._params() + [c1.weight, c1.bias, c2.weight, c2.bias] + [p for fc in fcs for p in (fc.weight, fc.bias)]
    return _CDADomainFn.apply(model, feat_nchw, samples, bool(labeled), float(domain_label), masks, scores, *params)


@META_ARCH_REGISTRY.register()
class CDAFasterRCNN(DAFasterRCNN):
    """``DAFasterRCNN`` whose instance-level domain classifier is conditioned on the class probabilities (module doc).
    Same inputs and the same seven loss keys; eval: ``inference`` (the domain heads are not part of it)."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.entropy_conditioning = self.da.entropy_conditioning
        self.multilinear_map = MultiLinearMap()

    def _ins_head_in_features(self):
        cls_score = self.roi_heads.box_predictor.cls_score
        return cls_score.in_features * cls_score.out_features

    def _domain_losses(self, feat_nchw, samples, labeled, domain_label, masks):
        return cda_domain_losses(self, feat_nchw, samples, labeled, domain_label, masks)
