"""DA Faster R-CNN (Chen et al. 2018): ``DAFasterRCNN``, ``DARPN`` and ``DAStandardROIHeads`` behind ``TRAINER "da"``.

Mirrors the reference's ``daod/modeling/meta_arch/da_faster_rcnn.py:22-272`` (meta-architecture and its three domain losses),
``daod/modeling/roi_heads/da_roi_heads.py:15-129`` (ROI heads that return the box features and sample unlabeled proposals:
``DAStandardROIHeads``, in modeling/roi_heads.py beside the other heads) and
``daod/modeling/proposal_generator/rpn.py:62-113`` (``DARPN``: d2's RPN, no ground truth meaning no losses).

Per domain the step makes ONE backbone pass and ONE ROIAlign + box-head pass in each direction: ``_DADomainFn`` is one autograd
node over (features, rois, parameters) that returns the domain's losses -- a combined sibling of ``_ROILossFn`` and
``_DCInsLossFn``.  With w_i = DC_IMG_GRL_WEIGHT, w_n = DC_INS_GRL_WEIGHT, w_c = DC_CONSISTENCY_WEIGHT:

  * image level: ``DAImgHead`` is evaluated once (the reference calls it twice on the same features and weights).  Its logit
    gradient is the BCE term's plus the consistency term's; its parameters take both unscaled; the backbone feature gets
    ``-w_i * g_bce + w_c * w_i * g_cons`` (the two gradient-scalar layers).
  * instance level: ``DAInsHead`` is evaluated twice in training mode -- ``instance_dc_loss`` and ``consistency_loss`` draw
    independent dropout masks (call order ins_s, ins_t, cons_s, cons_t; drawn on the host with torch's generator, injectable
    as ``model._forced_masks``); in eval mode one evaluation serves both.  The box features get ``-w_n * g_ins + w_c * w_n *
    g_cons``, on the source side plus the predictor's gradient, then ONE ``_box_head_backward``.
  * target side: no detection loss; the box head and the backbone still receive the two domain gradients through ROIAlign.

One level only (modeling/da_options.py): ``assign_boxes_to_levels`` is all zeros and the ``F.interpolate(align_corners=True)``
of ``image_dc_loss`` is the identity.  The losses' values and logit gradients are the HIP kernels of csrc/da_losses.hip
(``sfod_da_bce``, ``sfod_da_consistency_fwd`` / ``_bwd``).  A domain without a live ROI gives consistency and instance losses
of 0 (the reference's ``l1_loss`` / BCE of an empty tensor is NaN: SURVEY.md).
"""
import torch

from .. import native
from ..registry import META_ARCH_REGISTRY, PROPOSAL_GENERATOR_REGISTRY
from .batched import gather_gt
from .da_options import da_options
from .dann import DAImgHead, DAInsHead, ins_head_backward, ins_head_layers, ins_head_logits
from .meta_arch import GeneralizedRCNN
from .roi_heads import DAStandardROIHeads, _cls_kw  # noqa: F401  (the ROI heads of this architecture live beside the others)
from .rpn import RPN

MASK_ORDER = ("ins_s", "ins_t", "cons_s", "cons_t")      # the reference's call order of DAInsHead in one training step


@PROPOSAL_GENERATOR_REGISTRY.register()
class DARPN(RPN):
    """d2's RPN where no ground truth means no losses (rpn.py:62-113): a training-mode call without ``gt_instances``
    returns the proposals and an empty loss dict."""

    def forward(self, images, features, gt_instances=None, compute_loss=True, **kw):
        return super().forward(images, features, gt_instances, compute_loss=compute_loss and gt_instances is not None, **kw)


def _predictor_backward(heads, st, d_pred):
    """gradient of the fused (cls_score | bbox_pred) product: -> (d box features, [dw_cls, db_cls, dw_box, db_box])"""
    dtype = native.grad_dtype_of(heads.compute_dtype)
    dt = native.dt_of_dtype(dtype)
    K, NP = heads.num_classes, heads.pred_cols
    h = heads.box_features(st)
    d_pred_c = native.cast(d_pred, dtype)
    dwp = native.conv_wgrad(h, d_pred_c, NP, 1, operand=dtype).view(NP, -1)
    dbp = native.bias_grad(d_pred, NP)
    wpt = st.get("wpt")
    if wpt is None:
        wpt = native.pack_fc_weight(st["wp"], dt, transpose=True, ld=heads.pred_ld)
    dh = native.conv_fwd(d_pred_c, wpt, None, st["wp"].shape[1], 1)
    return dh, [dwp[: K + 1].contiguous(), dbp[: K + 1].contiguous(), dwp[K + 1:].contiguous(), dbp[K + 1:].contiguous()]


def _scalar(g):
    return g.reshape(1).float().contiguous()


class _DADomainFn(torch.autograd.Function):
    """(features, sampled rois) of ONE domain -> (loss_cls, loss_box_reg, loss_DC_img, loss_DC_ins, loss_DC_consistency) of
    that domain, un-halved.  ``samples`` with ground truth (source) or without (target: the two detection losses are
    constant zeros).  ``masks``: ``(instance_dc_loss's two, consistency_loss's two)`` dropout masks (uint8 [R, 1024]) or
    None (eval mode: one ``DAInsHead`` evaluation serves both).  ``params``: ``roi_heads._params()``, then ``DC_img``'s
    four, then ``DC_ins``'s six."""

    @staticmethod
    def forward(ctx, model, feat_nchw, samples, labeled, label, masks, *params):
        heads, opts = model.roi_heads, model.da
        dtype = heads.compute_dtype
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
        # instance level
        bf = heads.box_features(st)
        ev_ins = ins_head_logits(model.DC_ins, bf, masks[0] if masks is not None else None, dtype)
        ev_cons = ins_head_logits(model.DC_ins, bf, masks[1], dtype) if masks is not None else ev_ins
        l_ins, _ = native.da_bce(ev_ins["z"], label, rois=rois)
        pool = heads.box_pooler
        l_cons, cstate = native.da_consistency_fwd(z_img, ev_cons["z"], rois, heads.pooled, pool.scale,
                                                   sampling_ratio=pool.sampling_ratio, aligned=pool.aligned)
        ctx.model, ctx.samples, ctx.labeled, ctx.label = model, samples, labeled, float(label)
        ctx.state = (st, x, h1, z_img, ev_ins, ev_cons, cstate)
        ctx.feat_dtype = feat_nchw.dtype
        ctx.mark_non_differentiable(*(() if labeled else (l_cls, l_box)))
        return l_cls, l_box, l_img[0].clone(), l_ins[0].clone(), l_cons[0].clone()

    @staticmethod
    def backward(ctx, g_cls, g_box, g_img, g_ins, g_cons):
        model, samples = ctx.model, ctx.samples
        heads, opts = model.roi_heads, model.da
        st, x, h1, z_img, ev_ins, ev_cons, cstate = ctx.state
        rois = samples["rois"]
        w_i, w_n, w_c = opts.img_weight, opts.ins_weight, opts.consistency_weight
        # logit gradients: the three loss kernels
        _, dz_bce = native.da_bce(z_img, ctx.label, grad_scale=_scalar(g_img))
        _, dz_ins = native.da_bce(ev_ins["z"], ctx.label, rois=rois, grad_scale=_scalar(g_ins))
        dz_cimg, dz_cins = native.da_consistency_bwd(z_img, ev_cons["z"], rois, cstate, _scalar(g_cons))
        # DAImgHead: parameters take both terms unscaled, the feature map what the two gradient-scalar layers pass
        dx_img, img_grads = model.DC_img.grads(x, h1, dz_bce + dz_cimg, dz_bce * (-w_i) + dz_cimg * (w_c * w_i))
        # DAInsHead: one backward per evaluation, parameter gradients summed
        bf = heads.box_features(st)
        dbf_ins, ins_grads = ins_head_backward(model.DC_ins, bf, ev_ins, dz_ins, heads.compute_dtype)
        dbf_cons, cons_grads = ins_head_backward(model.DC_ins, bf, ev_cons, dz_cins, heads.compute_dtype)
        ins_grads = [a + b for a, b in zip(ins_grads, cons_grads)]
        dbf = torch.add(dbf_ins * (-w_n), dbf_cons, alpha=w_c * w_n)
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
        return (None, dfeat, None, None, None, None, *head_grads, *pred_grads, *img_grads, *ins_grads)


def da_domain_losses(model, feat_nchw, samples, labeled, domain_label, masks):
    """The five losses of one domain (``_DADomainFn``) as a tuple; ``masks``: None in eval mode."""
    c1, c2 = model.DC_img.convs()
    fcs = ins_head_layers(model.DC_ins)
    params = model.roi_heads._params() + [c1.weight, c1.bias, c2.weight, c2.bias] + [p for fc in fcs for p in (fc.weight, fc.bias)]
    return _DADomainFn.apply(model, feat_nchw, samples, bool(labeled), float(domain_label), masks, *params)


@META_ARCH_REGISTRY.register()
class DAFasterRCNN(GeneralizedRCNN):
    """``forward(batched_inputs)``: a list (source only: the four detection losses) or a tuple ``(source_list,
    target_list)``, which adds ``loss_DC_img``, ``loss_DC_ins`` and ``loss_DC_consistency``, each 0.5 (source + target);
    labels: source 0, target 1.  Eval: ``inference``."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.da = da_options(cfg, backbone_features=set(self.backbone._out_feature_channels))
        self.levels = [self.da.level]
        self.pooler_resolution = cfg.MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION
        self.dc_img_grl_weight, self.dc_ins_grl_weight = self.da.img_weight, self.da.ins_weight
        self.dc_consistency_weight = self.da.consistency_weight
        if hasattr(self.backbone, "needed_features"):
            self.backbone.needed_features.add(self.da.level)
        self.DC_img = DAImgHead(self.backbone._out_feature_channels[self.da.level], self.levels,
                                compute_dtype=self.compute_dtype)
        self.DC_ins = DAInsHead(self._ins_head_in_features(), self.levels, compute_dtype=self.compute_dtype)

    def _ins_head_in_features(self):
        return self.roi_heads.box_predictor.cls_score.in_features

    def _domain_losses(self, feat_nchw, samples, labeled, domain_label, masks):
        return da_domain_losses(self, feat_nchw, samples, labeled, domain_label, masks)

    def _draw_masks(self, n_rois):
        """the dropout masks of one training step in the reference's call order, or what a test injected"""
        forced = getattr(self, "_forced_masks", None)
        if forced is not None:
            return forced
        dev = self.device
        return {k: [(torch.rand(n_rois[k[-1]], 1024, device=dev) >= 0.5).to(torch.uint8) for _ in range(2)] for k in MASK_ORDER}

    def forward(self, batched_inputs):
        if not self.training:
            return self.inference(batched_inputs)
        if isinstance(batched_inputs, tuple):
            batched_s, batched_t = batched_inputs
        else:
            batched_s, batched_t = batched_inputs, None
        rh, level = self.roi_heads, self.da.level
        images_s = self.preprocess_image(batched_s)
        gt = gather_gt(batched_s, self.device)
        features_s = self._features(images_s)
        proposals_s, proposal_losses = self.proposal_generator(images_s, features_s, gt, as_instances=False)
        losses = {}
        if batched_t is None:
            _, detector_losses, *_ = rh(images_s, features_s, proposals_s, gt, want_box_features=False)
            losses.update(detector_losses)
            losses.update(proposal_losses)
            return losses
        samples_s = rh.label_and_sample_proposals(proposals_s, gt)
        images_t = self.preprocess_image(batched_t)
        features_t = self._features(images_t)
        with torch.no_grad():
            proposals_t, _ = self.proposal_generator(images_t, features_t, None, as_instances=False)
        samples_t = rh.sample_unlabeled_proposals(proposals_t)
        masks = self._draw_masks({"s": samples_s["rois"].shape[0], "t": samples_t["rois"].shape[0]})
        l_cls, l_box, img_s, ins_s, cons_s = self._domain_losses(features_s[level], samples_s, True, 0,
                                                                 (masks["ins_s"], masks["cons_s"]))
        _, _, img_t, ins_t, cons_t = self._domain_losses(features_t[level], samples_t, False, 1,
                                                         (masks["ins_t"], masks["cons_t"]))
        losses.update({"loss_cls": l_cls, "loss_box_reg": l_box})
        losses.update(proposal_losses)
        losses["loss_DC_img"] = 0.5 * (img_s + img_t)
        losses["loss_DC_ins"] = 0.5 * (ins_s + ins_t)
        losses["loss_DC_consistency"] = 0.5 * (cons_s + cons_t)
        return losses
