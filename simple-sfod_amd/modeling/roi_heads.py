"""ROI heads on the HIP kernels behind ``StandardROIHeads`` /
``SourceFreeAdaptiveTeacherStandardROIHeads`` / ``AdaptiveTeacherStandardROIHeads`` / ``DAStandardROIHeads`` / ``CDAStandardROIHeads``.

Mirrors ``/root/reference/daod/modeling/roi_heads/source_free_adaptive_teacher_roi_heads.py``:
``_init_box_head`` ``:27-66``, ``forward`` ``:68-106`` (training+compute_loss -> label & sample,
4-tuple; otherwise inference, 2-tuple), ``_forward_box`` ``:108-163``,
``label_and_sample_proposals`` ``:165-215``; and the Detectron2 pieces it inherits (SURVEY.md
A.11-A.13): add_ground_truth_to_proposals, Matcher [0.5], subsample 512 @ 0.25, ROIAlignV2 7x7 (POOLER_TYPE,
POOLER_SAMPLING_RATIO and POOLER_RESOLUTION <= 16 are built: modeling/roi_pooler.py),
FastRCNNConvFCHead (NUM_CONV / CONV_DIM / NUM_FC / FC_DIM / NORM "" or "GN" are built: modeling/box_head_options.py; the named
yamls' 2-FC head keeps its own pass), FastRCNNOutputLayers losses / inference.

State-dict keys: ``roi_heads.box_head.{conv{k}.{weight,bias}, conv{k}.norm.{weight,bias}, fc{k}.{weight,bias}}`` (Detectron2's),
``roi_heads.box_predictor.{cls_score,bbox_pred}.*``.
"""
import math

import torch
import torch.nn as nn

from .. import native
from ..registry import ROI_BOX_HEAD_REGISTRY, ROI_HEADS_REGISTRY
from ..structures import Boxes, Instances, ShapeSpec
from .offchain import OffChain as _OffChain, heads_on as _heads_on
from .batched import BatchedDetections, BatchedGT, BatchedProposals
from .box_head_options import GN_EPS, GN_GROUPS, box_head_options
from .box_regression import ROI_DEFAULT_WEIGHTS, roi_box_reg_options
from .cls_loss_options import native_cls_loss
from .proposal_options import roi_iou_band
from .roi_pooler import roi_pooler_options


class ROIPooler(nn.Module):
    """Single-level ROIAlign pooler: ``pooler_type`` "ROIAlignV2" (aligned=True) or "ROIAlign" (aligned=False), an integer
    ``sampling_ratio`` in [0, 16] (0: the adaptive grid), ``output_size`` in [1, 16]; anything else raises a ValueError
    naming the key (modeling/roi_pooler.py).  Attributes read from outside (source_free_adaptive_teacher_rcnn.py:190-194)
    are kept.  ``options`` is what the native calls take: empty = the default entry points."""

    def __init__(self, output_size, scales, sampling_ratio, pooler_type, prefix="MODEL.ROI_BOX_HEAD"):
        super().__init__()
        assert len(scales) == 1
        output_size, self.sampling_ratio, self.aligned = roi_pooler_options(output_size, sampling_ratio, pooler_type, prefix)
        self.pooler_type = pooler_type
        self.options = {} if (self.sampling_ratio == 0 and self.aligned) else \
            {"sampling_ratio": self.sampling_ratio, "aligned": self.aligned}
        self.output_size = (output_size, output_size)
        self.scale = scales[0]
        min_level = -(math.log2(scales[0]))
        self.min_level = self.max_level = int(min_level)
        self.canonical_level = 4
        self.canonical_box_size = 224


@ROI_BOX_HEAD_REGISTRY.register()
class FastRCNNConvFCHead(nn.Module):
    """Detectron2's FastRCNNConvFCHead: NUM_CONV x (conv3x3 pad 1, ``bias = not norm``, [GroupNorm(32) at ``conv{k}.norm``],
    ReLU; c2_msra_fill), flatten in (C, H, W) order, NUM_FC x (linear, ReLU; c2_xavier_fill).  What is built, and the
    ValueErrors for the rest: modeling/box_head_options.py."""

    def __init__(self, cfg, input_shape):
        super().__init__()
        self.options = o = box_head_options(cfg)
        c, h, w = input_shape.channels, input_shape.height, input_shape.width
        self.convs = []
        for k in range(o.num_conv):
            conv = nn.Conv2d(c, o.conv_dim, kernel_size=3, padding=1, bias=not o.norm)
            nn.init.kaiming_normal_(conv.weight, mode="fan_out", nonlinearity="relu")
            if conv.bias is not None:
                nn.init.constant_(conv.bias, 0)
            if o.norm:
                conv.norm = nn.GroupNorm(GN_GROUPS, o.conv_dim, eps=GN_EPS)      # d2 get_norm("GN"): weight 1, bias 0
            self.add_module("conv{}".format(k + 1), conv)
            self.convs.append(conv)
            c = o.conv_dim
        self._in = c * h * w
        self.fcs = []
        d = self._in
        for k in range(o.num_fc):
            fc = nn.Linear(d, o.fc_dim)
            nn.init.kaiming_uniform_(fc.weight, a=1)
            nn.init.constant_(fc.bias, 0)
            self.add_module("fc{}".format(k + 1), fc)
            self.fcs.append(fc)
            d = o.fc_dim
        self._out = d
        # channels only behind an FC; else the last convolution's (C, H, W) map, flattened by the predictor in that order
        self._out_shape = ShapeSpec(channels=d) if o.num_fc else ShapeSpec(channels=c, height=h, width=w)

    @property
    def output_shape(self):
        return self._out_shape


class FastRCNNOutputLayers(nn.Module):
    def __init__(self, cfg, input_shape, roi_heads_name=None):
        super().__init__()
        d = input_shape.channels * (input_shape.height or 1) * (input_shape.width or 1)      # d2: a (C, H, W) input is flattened
        self.num_classes = cfg.MODEL.ROI_HEADS.NUM_CLASSES
        # BBOX_REG_LOSS_TYPE / SMOOTH_L1_BETA / BBOX_REG_WEIGHTS / CLS_AGNOSTIC_BBOX_REG / BBOX_REG_LOSS_WEIGHT (ValueError
        # naming the key for what is not built); ``_box_reg`` is what the native calls take: None = the default entry points
        self.box_reg, self.box_reg_loss_weight = roi_box_reg_options(cfg)
        self.box_reg_loss_type, self.smooth_l1_beta = self.box_reg.loss_type, self.box_reg.beta
        self.box_reg_weights, self.cls_agnostic_bbox_reg = self.box_reg.weights, self.box_reg.cls_agnostic
        self._box_reg = None if self.box_reg.is_default(ROI_DEFAULT_WEIGHTS) else self.box_reg
        # MODEL.ROI_HEADS.LOSS / SFOD.FOCAL_LOSS_GAMMA / MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE (modeling/cls_loss_options.py; a
        # ValueError naming the key for what is not built), under the ROI heads that build this predictor; ``_cls_loss`` is
        # what the native calls take: None = the entry points of before these keys were read
        self._cls_loss = native_cls_loss(cfg, roi_heads_name)
        self.cls_score = nn.Linear(d, self.num_classes + 1)
        self.bbox_pred = nn.Linear(d, 4 if self.cls_agnostic_bbox_reg else self.num_classes * 4)
        nn.init.normal_(self.cls_score.weight, std=0.01)
        nn.init.normal_(self.bbox_pred.weight, std=0.001)
        for l in [self.cls_score, self.bbox_pred]:
            nn.init.constant_(l.bias, 0)
        self.test_score_thresh = cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST
        self.test_nms_thresh = cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST
        self.test_topk_per_image = cfg.TEST.DETECTIONS_PER_IMAGE


_SCALE_CLAMP = math.log(1000.0 / 16)


def _apply_deltas(deltas, boxes, weights=ROI_DEFAULT_WEIGHTS):
    """d2 Box2BoxTransform.apply_deltas (A.5) in torch ops: the Instances-level API twins below use it; the
    step itself decodes inside the HIP kernels (detect.hip)."""
    deltas, boxes = deltas.float(), boxes.float()
    wx, wy, ww, wh = weights
    widths, heights = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    ctr_x, ctr_y = boxes[:, 0] + 0.5 * widths, boxes[:, 1] + 0.5 * heights
    dx, dy = deltas[:, 0::4] / wx, deltas[:, 1::4] / wy
    dw = torch.clamp(deltas[:, 2::4] / ww, max=_SCALE_CLAMP)
    dh = torch.clamp(deltas[:, 3::4] / wh, max=_SCALE_CLAMP)
    pcx, pcy = dx * widths[:, None] + ctr_x[:, None], dy * heights[:, None] + ctr_y[:, None]
    pw, ph = torch.exp(dw) * widths[:, None], torch.exp(dh) * heights[:, None]
    return torch.stack((pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph), dim=-1).reshape(deltas.shape)


class _PredictorAPI:
    """d2 ``FastRCNNOutputLayers.{predict_boxes, predict_probs, predict_boxes_for_gt_classes}`` on
    ``predictions = (scores [R,K+1], proposal_deltas [R,4K] or, class-agnostic, [R,4])`` and ``list[Instances]``
    proposals (A.12), under the configured BBOX_REG_WEIGHTS."""

    def predict_boxes(self, predictions, proposals):
        _, deltas = predictions
        if not len(proposals):
            return []
        pb = torch.cat([p.proposal_boxes.tensor for p in proposals], dim=0)
        return _apply_deltas(deltas, pb, self.box_reg_weights).split([len(p) for p in proposals])

    def predict_probs(self, predictions, proposals):
        scores, _ = predictions
        # the library's row softmax (sfod_predict_probs: the fused teacher post-processing's own operation order), or under
        # USE_SIGMOID_CE its sigmoid of every score
        cl = self._cls_loss
        probs = native.predict_probs(scores.float(), **({"cls_loss": cl} if cl is not None else {}))
        return probs.split([len(p) for p in proposals], dim=0)

    def predict_boxes_for_gt_classes(self, predictions, proposals):
        if not len(proposals):
            return []
        _, deltas = predictions
        pb = torch.cat([p.proposal_boxes.tensor for p in proposals], dim=0)
        N, K = pb.shape[0], deltas.shape[1] // 4
        boxes = _apply_deltas(deltas, pb, self.box_reg_weights)
        if K > 1:
            gt = torch.cat([p.gt_classes for p in proposals], dim=0).clamp(0, K - 1)
            boxes = boxes.view(N, K, 4)[torch.arange(N, device=boxes.device), gt]
        return boxes.split([len(p) for p in proposals])


for _name in ("predict_boxes", "predict_probs", "predict_boxes_for_gt_classes"):
    setattr(FastRCNNOutputLayers, _name, getattr(_PredictorAPI, _name))


class SourceFreeFastRCNNOutputLayers(FastRCNNOutputLayers):
    """source_free_fast_rcnn.py:14.  ``convert_bbox_scores`` (:15-36 -> ``fast_rcnn_inference_single_image_new``
    :82-147) only feeds the zero-weighted, logged BPC loss; this is its Instances-level twin in torch ops --
    the training step computes BPC from the same predictions in one fused kernel (``sfod_bpc_loss``)."""

    def convert_bbox_scores(self, predictions, proposals):
        boxes = self.predict_boxes(predictions, proposals)
        scores = self.predict_probs(predictions, proposals)
        image_shapes = [x.image_size for x in proposals]
        return self.fast_rcnn_inference_new(boxes, scores, image_shapes, self.test_score_thresh, self.test_nms_thresh,
                                            self.test_topk_per_image, proposals)

    def fast_rcnn_inference_new(self, boxes, scores, image_shapes, score_thresh, nms_thresh, topk_per_image, proposals):
        """:38-80 -- per image ``fast_rcnn_inference_single_image_new``; -> (list[Instances], list[row index])."""
        per_image = [self.fast_rcnn_inference_single_image_new(b, s, shape, score_thresh, nms_thresh, topk_per_image, p)
                     for s, b, shape, p in zip(scores, boxes, image_shapes, proposals)]
        return [x[0] for x in per_image], [x[1] for x in per_image]

    def fast_rcnn_inference_single_image_new(self, boxes, scores, image_shape, score_thresh=0.0, nms_thresh=0.0,
                                             topk_per_image=-1, proposal=None):
        """:82-147 -- rows with a non-finite box or score are dropped first (the returned row index counts the
        survivors), the background column goes, boxes are clipped, every (row, class) with ``score > 0`` is kept in
        row-major order; the thresholds are accepted and unused like the reference's (its NMS is commented out, :132-138).
        ``boxes`` [R, 4K] per-class or [R, 4] class-agnostic; ``scores`` [R, K+1] probabilities.
        Pinned by the reference-run fixture tests/golden/glue_ref.npz."""
        valid = torch.isfinite(boxes).all(dim=1) & torch.isfinite(scores).all(dim=1)
        if not valid.all():
            boxes, scores = boxes[valid], scores[valid]
        scores = scores[:, :-1]
        nreg = boxes.shape[1] // 4
        b = Boxes(boxes.reshape(-1, 4))
        b.clip(image_shape)
        boxes = b.tensor.view(-1, nreg, 4)
        mask = scores > 0                     # "We do not filter out anything here"
        inds = mask.nonzero()
        res = Instances(image_shape)
        res.pred_boxes = Boxes(boxes[inds[:, 0], 0] if nreg == 1 else boxes[mask])
        res.scores = scores[mask]
        res.pred_classes = inds[:, 1]
        return res, inds[:, 0]


def _cls_kw(box_predictor):
    """the ``cls_loss`` keyword of a native call: absent with every classification key at its default (the call of before)"""
    cl = box_predictor._cls_loss
    return {} if cl is None else {"cls_loss": cl}


class InstanceProposals:
    """4th value of the training-mode ROI heads (``instance_proposals``,
    source_free_adaptive_teacher_roi_heads.py:101,158): the per-class decoded predictions of the sampled
    proposals, kept as references to the pass's prediction matrix and sample arrays.  ``bpc_loss(gt)`` runs the
    fused kernel; ``to_instances()`` materialises the reference's ``list[Instances]`` (host API, syncs)."""

    def __init__(self, heads, pred, samples):
        self.heads, self.pred, self.samples = heads, pred, samples

    def bpc_loss(self, targets, iou_thresh=0.5):
        h, sm = self.heads, self.samples
        sizes = native.dev_const(tuple((int(s[0]), int(s[1])) for s in sm["image_sizes"]), torch.int32,
                                 self.pred.device)
        return native.bpc_loss(self.pred, h.num_classes, sm["rois"], sm["gt_cls"], sizes, targets.boxes,
                               targets.classes, targets.count, iou_thresh, box_reg=h.box_predictor._box_reg,
                               **_cls_kw(h.box_predictor))

    def to_instances(self):
        h, sm = self.heads, self.samples
        K = h.num_classes
        rois, cls = sm["rois"], sm["gt_cls"]
        props = []
        for b, size in enumerate(sm["image_sizes"]):
            m = rois[:, 0] == b
            p = Instances(size)
            p.proposal_boxes = Boxes(rois[m, 1:5])
            p.gt_classes = cls[m].long()
            props.append(p)
        order = torch.cat([torch.nonzero(rois[:, 0] == b).flatten() for b in range(len(props))])
        bp = h.box_predictor
        predictions = (self.pred[order, : K + 1], self.pred[order, K + 1: bp.box_reg.pred_cols(K)])
        for p, nb in zip(props, bp.predict_boxes_for_gt_classes(predictions, props)):     # :136-143
            p.proposal_boxes = Boxes(nb)
        return bp.convert_bbox_scores(predictions, props)[0]


class _ROILossFn(torch.autograd.Function):
    """features (+ sampled rois) -> (loss_cls, loss_box_reg) with a hand-written backward."""

    @staticmethod
    def forward(ctx, heads, feat_nchw, samples, *params):
        st = heads._box_forward(feat_nchw, samples["rois"])
        bp = heads.box_predictor
        loss, _ = native.frcnn_loss(st["pred"], heads.num_classes, samples["rois"], samples["gt_cls"],
                                    samples["gt_box"], samples["n_valid"], box_reg=bp._box_reg, **_cls_kw(bp))
        ctx.heads, ctx.st, ctx.samples = heads, st, samples
        ctx.feat_shape = feat_nchw.shape
        heads._last_pred = st["pred"]          # for InstanceProposals (BPC); alive until the backward anyway
        # BBOX_REG_LOSS_WEIGHT: applied here, an fp32 scalar multiplication like the ``loss * weight`` it replaces (1.0: the
        # node returns what it returned before the key was read)
        ctx.box_w = bp.box_reg_loss_weight
        return loss[0].clone(), (loss[1].clone() if ctx.box_w == 1.0 else loss[1] * ctx.box_w)

    @staticmethod
    def backward(ctx, g_cls, g_box):
        heads, st, samples = ctx.heads, ctx.st, ctx.samples
        if ctx.box_w != 1.0:
            g_box = g_box * ctx.box_w
        gs = torch.stack([g_cls.reshape(()), g_box.reshape(())]).float().contiguous()
        _, d_pred = native.frcnn_loss(st["pred"], heads.num_classes, samples["rois"], samples["gt_cls"],
                                      samples["gt_box"], samples["n_valid"], grad_scale=gs,
                                      box_reg=heads.box_predictor._box_reg, **_cls_kw(heads.box_predictor))
        dfeat, pgrads = heads._box_backward(st, samples["rois"], d_pred, ctx.feat_shape)
        ctx.st = None
        return (None, dfeat, None) + tuple(pgrads)


@ROI_HEADS_REGISTRY.register()
class StandardROIHeads(nn.Module):
    def __init__(self, cfg, input_shape):
        super().__init__()
        r = cfg.MODEL.ROI_HEADS
        self.num_classes = r.NUM_CLASSES
        self.batch_size_per_image = r.BATCH_SIZE_PER_IMAGE
        self.positive_fraction = r.POSITIVE_FRACTION
        self.proposal_append_gt = r.PROPOSAL_APPEND_GT
        # [t] / [0, 1], or an ignore band [lo, hi] / [0, -1, 1] (anything else: ValueError naming the keys).  ``_iou_lo`` is
        # what ``native.roi_match`` takes: None = the one-threshold entry point, as before the band was built
        lo, self.iou_threshold = roi_iou_band(cfg)
        self._iou_lo = None if lo == self.iou_threshold else lo
        self.box_in_features = self.in_features = r.IN_FEATURES
        assert len(self.in_features) == 1
        shape = input_shape[self.in_features[0]]
        res = cfg.MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION
        self.box_pooler = ROIPooler(res, (1.0 / shape.stride,), cfg.MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO,
                                    cfg.MODEL.ROI_BOX_HEAD.POOLER_TYPE)
        self.box_head = ROI_BOX_HEAD_REGISTRY.get(cfg.MODEL.ROI_BOX_HEAD.NAME)(
            cfg, ShapeSpec(channels=shape.channels, height=res, width=res))
        self.box_predictor = self._make_predictor(cfg, self.box_head.output_shape)
        self.pooled = res
        self.channels = shape.channels
        # the named yamls' 2-FC head runs the pass written for it below; every other built head the general one
        opts = getattr(self.box_head, "options", None)
        self._general = opts is not None and not opts.is_default()
        self.compute_dtype = native.mode_dtype(cfg.SFOD.COMPUTE_DTYPE)
        K = self.num_classes
        self.pred_cols = self.box_predictor.box_reg.pred_cols(K)      # K + 1 scores | 4K deltas (class-agnostic: 4)
        self.pred_ld = (self.pred_cols + 7) // 8 * 8
        self.bbox_threshold = cfg.SEMISUPNET.BBOX_THRESHOLD if "SEMISUPNET" in cfg else 0.7
        self.nms_numel_limit = 20000  # torchvision batched_nms switch for GPU tensors (A.6)
        self.train_on_pred_boxes = cfg.MODEL.ROI_BOX_HEAD.TRAIN_ON_PRED_BOXES

    def _make_predictor(self, cfg, shape):
        return FastRCNNOutputLayers(cfg, shape, roi_heads_name=type(self).__name__)

    def _params(self):
        bh, bp = self.box_head, self.box_predictor
        if self._general:      # the head's parameters in module order, then the predictor's
            return list(bh.parameters()) + [bp.cls_score.weight, bp.cls_score.bias, bp.bbox_pred.weight, bp.bbox_pred.bias]
        return [bh.fc1.weight, bh.fc1.bias, bh.fc2.weight, bh.fc2.bias, bp.cls_score.weight, bp.cls_score.bias,
                bp.bbox_pred.weight, bp.bbox_pred.bias]

    # ---- the training pass's weights, packed ahead of time ---------------------------------------------------------------
    @torch.no_grad()
    def prefetch_weights(self):
        """Pack the box head's and predictor's weights in the forms the training pass multiplies with -- forward and
        backward -- NOW; the next ``_box_forward`` takes them instead of packing (fc1 is 103 MB: four launches of 60-90 us
        that otherwise sit between the pseudo labels and the losses).  The trainer calls it (``model.prefetch_features``)
        while the teacher is still labelling; nothing changes the weights before this step's update, and what is not
        taken by then is dropped at the start of the next step (``drop_prefetched``)."""
        if self._general:      # nothing is packed ahead for the other heads: their pass packs where it multiplies
            return
        dt = native.dt_of_dtype(self.compute_dtype)
        gdt = native.dt_of_dtype(native.grad_dtype_of(self.compute_dtype))
        bh, bp, C = self.box_head, self.box_predictor, self.channels
        wp = torch.cat([bp.cls_score.weight.detach(), bp.bbox_pred.weight.detach()])
        self._packed = {
            "w1": native.pack_fc_weight(bh.fc1.weight.detach(), dt, chw_c=C),
            "w2": native.pack_fc_weight(bh.fc2.weight.detach(), dt),
            "wp": wp, "bpb": torch.cat([bp.cls_score.bias.detach(), bp.bbox_pred.bias.detach()]),
            "wpp": native.pack_fc_weight(wp, dt),
            "wpt": native.pack_fc_weight(wp, gdt, transpose=True, ld=self.pred_ld),
            "w2t": native.pack_fc_weight(bh.fc2.weight.detach(), gdt, transpose=True),
            "w1t": native.pack_fc_weight(bh.fc1.weight.detach(), gdt, chw_c=C, transpose=True)}

    # ---- box branch: ROIAlign -> fc1 -> fc2 -> fused (cls_score | bbox_pred) -------------------------
    def _box_forward(self, feat_nchw, rois):
        if self._general:
            return self._box_forward_general(feat_nchw, rois)
        dtype = self.compute_dtype
        dt = native.dt_of_dtype(dtype)
        feat = native.nhwc_operand(feat_nchw, dtype)
        bh, bp = self.box_head, self.box_predictor
        C, PP = self.channels, self.pooled * self.pooled
        pk = self.__dict__.pop("_packed", None) or {}
        pooled = native.roi_align_fwd(feat, rois, self.pooled, self.box_pooler.scale, **self.box_pooler.options)
        R = pooled.shape[0]
        x0 = pooled.view(R, PP * C)
        w1 = pk["w1"] if pk else native.pack_fc_weight(bh.fc1.weight.detach(), dt, chw_c=C)
        h1 = native.conv_fwd(x0, w1, bh.fc1.bias.detach(), bh.fc1.out_features, 1, act=1)
        w2 = pk["w2"] if pk else native.pack_fc_weight(bh.fc2.weight.detach(), dt)
        h2 = native.conv_fwd(h1, w2, bh.fc2.bias.detach(), bh.fc2.out_features, 1, act=1)
        wp = pk["wp"] if pk else torch.cat([bp.cls_score.weight.detach(), bp.bbox_pred.weight.detach()])
        bpb = pk["bpb"] if pk else torch.cat([bp.cls_score.bias.detach(), bp.bbox_pred.bias.detach()])
        wpp = pk["wpp"] if pk else native.pack_fc_weight(wp, dt)
        pred = native.conv_fwd(h2, wpp, bpb, wp.shape[0], 1, out_dtype=torch.float32, ldy=self.pred_ld)
        st = {"x0": x0, "h1": h1, "h2": h2, "pred": pred, "wp": wp, "feat_shape": tuple(feat.shape)}
        for k in ("wpt", "w2t", "w1t"):           # the backward's forms ride with the pass's state
            if k in pk:
                st[k] = pk[k]
        return st

    def _box_backward(self, st, rois, d_pred, feat_shape_nchw):
        if self._general:
            return self._box_backward_general(st, rois, d_pred)
        dtype = native.grad_dtype_of(self.compute_dtype)      # operands of the backward products ("f16x3": bf16 pairs)
        dt = native.dt_of_dtype(dtype)
        bh = self.box_head
        K = self.num_classes
        NP = self.pred_cols
        d_pred_c = native.cast(d_pred, dtype)
        # predictor: its parameter gradients beside the data-gradient path (``_OffChain``), like fc2's and fc1's below
        off = _OffChain(_heads_on(d_pred))
        dwp, dbp = off.run(lambda: (native.conv_wgrad(st["h2"], d_pred_c, NP, 1, operand=dtype).view(NP, -1),
                                    native.bias_grad(d_pred, NP)), st["h2"], d_pred_c, d_pred)
        wpt = st.get("wpt")
        if wpt is None:
            wpt = native.pack_fc_weight(st["wp"], dt, transpose=True, ld=self.pred_ld)
        dh2 = native.conv_fwd(d_pred_c, wpt, None, bh.fc2.out_features, 1)
        dfeat, (dw1, db1, dw2, db2) = self._box_head_backward(st, rois, dh2)     # (joins the side stream)
        off.join(dwp, dbp)
        pgrads = [dw1, db1, dw2, db2, dwp[: K + 1].contiguous(), dbp[: K + 1].contiguous(),
                  dwp[K + 1:].contiguous(), dbp[K + 1:].contiguous()]
        return dfeat, pgrads

    def _box_head_backward(self, st, rois, dh2):
        """grad wrt the box-head output (``box_features`` = relu(fc2), consumed in place) -> (grad wrt the feature
        map as an NCHW view, the head's parameter gradients as a list in ``_params()`` order: [dw1, db1, dw2, db2]); an entry is
        None when it went straight into the flat gradient (dw1)."""
        if self._general:
            return self._box_head_backward_general(st, rois, dh2)
        dtype = native.grad_dtype_of(self.compute_dtype)      # operands of the backward products ("f16x3": bf16 pairs)
        dt = native.dt_of_dtype(dtype)
        bh = self.box_head
        C = self.channels
        native.act_bwd_(dh2, st["h2"], 1)
        # fc2
        off = _OffChain(_heads_on(dh2))
        dw2, db2 = off.run(lambda: (native.conv_wgrad(st["h1"], dh2, bh.fc2.out_features, 1, operand=dtype).view(bh.fc2.out_features, -1),
                                    native.bias_grad(dh2, bh.fc2.out_features)), st["h1"], dh2)
        w2t = st.get("w2t")
        if w2t is None:
            w2t = native.pack_fc_weight(bh.fc2.weight.detach(), dt, transpose=True)
        dh1 = native.conv_fwd(dh2, w2t, None, bh.fc2.in_features, 1)
        native.act_bwd_(dh1, st["h1"], 1)
        # fc1 (K axis in (p, c) order inside the kernels, (c, p) in the state dict).  Its weight gradient (the largest of the
        # heads: 26-420 GFLOP + the 103-411 MB un-packing pass) does not feed the data-gradient path: it runs on a side
        # stream beside dx0 and the ROIAlign backward -- a latency-bound gather that leaves most of the chip idle -- like the
        # backbone's weight gradients beside its data-gradient chain (SFOD_HEAD_WGRAD_STREAM=0: one stream)
        def fc1_param_grads():
            dw1p = native.conv_wgrad(st["x0"], dh1, bh.fc1.out_features, 1, operand=dtype).view(bh.fc1.out_features, -1)
            dw1_ = native.grad_sink(bh.fc1.weight)
            if dw1_ is not None:     # 103 MB: accumulate straight into the flat gradient, nothing for autograd to add
                native.unpack_fc_wgrad(dw1p, dw1_, chw_c=C, accumulate=True)
                dw1_ = None
            else:
                dw1_ = torch.empty_like(bh.fc1.weight)
                native.unpack_fc_wgrad(dw1p, dw1_, chw_c=C)
            return dw1_, native.bias_grad(dh1, bh.fc1.out_features)

        dw1, db1 = off.run(fc1_param_grads, st["x0"], dh1)     # dh1 (after its ReLU mask) and x0 are complete on the main stream
        w1t = st.get("w1t")
        if w1t is None:
            w1t = native.pack_fc_weight(bh.fc1.weight.detach(), dt, chw_c=C, transpose=True)
        dx0 = native.conv_fwd(dh1, w1t, None, bh.fc1.in_features, 1)
        B, H, W, _ = st["feat_shape"]
        dfeat = native.roi_align_bwd(dx0.view(-1, self.pooled * self.pooled, C), rois, (B, H, W, C), self.pooled,
                                     self.box_pooler.scale, **self.box_pooler.options)
        off.join(dw1, db1, dw2, db2)     # the heads' gradients are final before anyone (all-reduce, SGD, autograd) reads them
        return dfeat.permute(0, 3, 1, 2), [dw1, db1, dw2, db2]

    def box_features(self, st):
        """the box head's output of a pass's state (``box_features`` of the reference: what the instance-level domain
        discriminator reads), [R, FC_DIM]"""
        if not self._general:
            return st["h2"]
        if not st["hs"]:
            raise ValueError("MODEL.ROI_BOX_HEAD.NUM_FC 0: the box head has no flat FC features (SEMISUPNET.INS_DC / "
                             "DOMAIN_CLASSIFIER.INSTANCE need NUM_FC >= 1)")
        return st["hs"][-1]

    # ---- the general pass: ROIAlign -> NUM_CONV x (conv3x3 [+ GroupNorm] + ReLU) -> NUM_FC x (linear + ReLU) -> predictor ----
    def _box_forward_general(self, feat_nchw, rois):
        dtype = self.compute_dtype
        dt = native.dt_of_dtype(dtype)
        feat = native.nhwc_operand(feat_nchw, dtype)
        bh, bp, P = self.box_head, self.box_predictor, self.pooled
        pooled = native.roi_align_fwd(feat, rois, P, self.box_pooler.scale, **self.box_pooler.options)
        R = pooled.shape[0]
        x = pooled.view(R, P, P, self.channels)
        xw = x                                     # what the next layer's weight gradient reads (converted there if need be)
        convs = []
        for conv in bh.convs:
            # (a backbone width the 3x3 kernels do not take -- not 8 x a power of two -- gets zero channels behind; CONV_DIM is
            # held to such a width by box_head_options, so only the first layer's input can need it)
            cp = native.conv3x3_channels(x.shape[-1], dt)
            same = xw is x
            x = native.pad_channels(x, cp)
            xw = x if same else native.pad_channels(xw, cp)
            w = native.pack_conv_weight(conv.weight.detach(), cp, dt)
            norm = getattr(conv, "norm", None)
            if norm is not None:
                y = native.conv_fwd(x, w, None, conv.out_channels, 3, act=0)
                z, zg, mean, rstd = native.group_norm_relu_fwd(y, norm.weight.detach(), norm.bias.detach(), norm.num_groups,
                                                               norm.eps, out_dtype=dtype, with_grad_operand=True)
                convs.append({"xw": xw, "y": y, "mean": mean, "rstd": rstd})
                x, xw = z, zg
            else:
                y = native.conv_fwd(x, w, conv.bias.detach(), conv.out_channels, 3, act=1)
                convs.append({"xw": xw, "y": y})
                x = xw = y
        chw = x.shape[-1]                          # (c, p) state-dict order of the first flat layer <-> (p, c) in the kernels
        flat = x.view(R, -1)
        h, hs = flat, []
        for i, fc in enumerate(bh.fcs):
            w = native.pack_fc_weight(fc.weight.detach(), dt, chw_c=chw if i == 0 else 0)
            h = native.conv_fwd(h, w, fc.bias.detach(), fc.out_features, 1, act=1)
            hs.append(h)
        wp = torch.cat([bp.cls_score.weight.detach(), bp.bbox_pred.weight.detach()])
        bpb = torch.cat([bp.cls_score.bias.detach(), bp.bbox_pred.bias.detach()])
        wpp = native.pack_fc_weight(wp, dt, chw_c=0 if hs else chw)
        pred = native.conv_fwd(h, wpp, bpb, wp.shape[0], 1, out_dtype=torch.float32, ldy=self.pred_ld)
        return {"x0": pooled.view(R, -1), "convs": convs, "flat": xw.view(R, -1), "chw": chw, "hs": hs, "pred": pred, "wp": wp,
                "feat_shape": tuple(feat.shape)}

    def _box_backward_general(self, st, rois, d_pred):
        dtype = native.grad_dtype_of(self.compute_dtype)
        dt = native.dt_of_dtype(dtype)
        K, NP = self.num_classes, self.pred_cols
        h = st["hs"][-1] if st["hs"] else st["flat"]
        chw = 0 if st["hs"] else st["chw"]
        d_pred_c = native.cast(d_pred, dtype)
        off = _OffChain(_heads_on(d_pred))

        def pred_grads():
            dwp = native.conv_wgrad(h, d_pred_c, NP, 1, operand=dtype).view(NP, -1)
            if chw:      # the predictor reads the (C, H, W) map: back to the state dict's (c, p) order
                dw = torch.empty(NP, dwp.shape[1], dtype=torch.float32, device=dwp.device)
                native.unpack_fc_wgrad(dwp, dw, chw_c=chw)
                dwp = dw
            return dwp, native.bias_grad(d_pred, NP)

        dwp, dbp = off.run(pred_grads, h, d_pred_c, d_pred)
        wpt = native.pack_fc_weight(st["wp"], dt, chw_c=chw, transpose=True, ld=self.pred_ld)
        dh = native.conv_fwd(d_pred_c, wpt, None, st["wp"].shape[1], 1)
        dfeat, hg = self._box_head_backward_general(st, rois, dh)     # (joins the side stream)
        off.join(dwp, dbp)
        return dfeat, hg + [dwp[: K + 1].contiguous(), dbp[: K + 1].contiguous(), dwp[K + 1:].contiguous(),
                            dbp[K + 1:].contiguous()]

    def _box_head_backward_general(self, st, rois, dh):
        """``_box_head_backward`` of any built head: the layers in reverse; weight, bias and GroupNorm-parameter gradients in
        ``box_head.parameters()`` order (None: added straight into the parameter's ``grad_sink``).  The weight and bias
        gradients run beside the data-gradient path; the GroupNorm backward is ON that path (it makes the convolution's dy)
        and sums dgamma / dbeta in a fixed order (include/sfod_hip.h), so the pass is reproducible bit for bit under
        SFOD.DETERMINISTIC."""
        dtype = native.grad_dtype_of(self.compute_dtype)
        dt = native.dt_of_dtype(dtype)
        bh, P = self.box_head, self.pooled
        off = _OffChain(_heads_on(dh))
        grads = {}
        d = dh
        for i in reversed(range(len(bh.fcs))):
            fc, xin, chw = bh.fcs[i], (st["hs"][i - 1] if i else st["flat"]), (0 if i else st["chw"])
            native.act_bwd_(d, st["hs"][i], 1)

            def fc_param_grads(fc=fc, xin=xin, d=d, chw=chw):
                dw = native.conv_wgrad(xin, d, fc.out_features, 1, operand=dtype).view(fc.out_features, -1)
                if chw:
                    dwp, dw = dw, native.grad_sink(fc.weight)
                    if dw is not None:
                        native.unpack_fc_wgrad(dwp, dw, chw_c=chw, accumulate=True)
                        dw = None
                    else:
                        dw = torch.empty_like(fc.weight)
                        native.unpack_fc_wgrad(dwp, dw, chw_c=chw)
                return dw, native.bias_grad(d, fc.out_features)

            grads[fc.weight], grads[fc.bias] = off.run(fc_param_grads, xin, d)
            wt = native.pack_fc_weight(fc.weight.detach(), dt, chw_c=chw, transpose=True)
            d = native.conv_fwd(d, wt, None, fc.in_features, 1)
        for k in reversed(range(len(bh.convs))):
            conv, rec = bh.convs[k], st["convs"][k]
            d = d.view(rec["y"].shape)
            norm = getattr(conv, "norm", None)
            if norm is not None:
                gs, bs = native.grad_sink(norm.weight), native.grad_sink(norm.bias)
                into = gs is not None and bs is not None
                dy, dg, db = native.group_norm_relu_bwd(d, rec["y"], rec["mean"], rec["rstd"], norm.weight.detach(),
                                                        norm.bias.detach(), norm.num_groups, dgamma=gs if into else None,
                                                        dbeta=bs if into else None, accumulate=into,
                                                        out_dtype=dtype if native.is_pairs(dtype) else None)
                grads[norm.weight], grads[norm.bias] = (None, None) if into else (dg, db)
            else:
                dy = native.act_bwd_(d, rec["y"], 1)
                grads[conv.bias] = off.run(lambda dy=dy, conv=conv: native.bias_grad(dy, conv.out_channels), dy)
            grads[conv.weight] = off.run(lambda rec=rec, dy=dy, conv=conv: native.conv_weight_grad(
                rec["xw"], dy, conv.weight, operand=dtype), rec["xw"], dy)
            wr = native.pack_conv_weight(conv.weight.detach(), dy.shape[-1], dt, rot180=True)
            d = native.conv_fwd(dy, wr, None, conv.in_channels, 3)
        B, H, W, C = st["feat_shape"]
        dfeat = native.roi_align_bwd(d.view(-1, P * P, C), rois, (B, H, W, C), P, self.box_pooler.scale,
                                     **self.box_pooler.options)
        out = [grads[p] for p in bh.parameters()]
        off.join(*out)
        return dfeat.permute(0, 3, 1, 2), out

    # ---- label_and_sample_proposals (roi_heads.py:165-215) ----------------------------------------
    @torch.no_grad()
    def label_and_sample_proposals(self, proposals, targets, branch="", keys=None):
        props = proposals
        B, P, _ = props.boxes.shape
        if self.proposal_append_gt:
            boxes, count = native.append_gt(props.boxes, props.count, targets.boxes, targets.count)
        else:
            boxes, count = props.boxes, props.count
        matched, cls = native.roi_match(boxes, count, targets.boxes, targets.classes, targets.count,
                                        self.iou_threshold, self.num_classes,
                                        **({"lo": self._iou_lo} if self._iou_lo is not None else {}))
        keys = keys if keys is not None else getattr(self, "_forced_keys", None)
        if keys is None:
            keys = torch.randint(0, 2 ** 31 - 1, (B, boxes.shape[1]), dtype=torch.int32, device=boxes.device)
        sidx, scnt = native.subsample_roi(cls, keys, self.batch_size_per_image, self.positive_fraction,
                                          self.num_classes)
        rois, gt_cls, gt_box, n_valid = native.roi_build_samples(boxes, cls, matched, sidx, scnt, targets.boxes,
                                                                 targets.count)
        return {"rois": rois, "gt_cls": gt_cls, "gt_box": gt_box, "n_valid": n_valid, "count": scnt,
                "sampled_idxs": sidx, "image_sizes": props.image_sizes}

    @torch.no_grad()
    def _inference(self, feat, proposals, sizes_dev=None):
        rois = native.make_rois(proposals.boxes, proposals.count)
        st = self._box_forward(feat, rois)
        bp = self.box_predictor
        if sizes_dev is None:
            sizes_dev = native.dev_const(tuple((int(s[0]), int(s[1])) for s in proposals.image_sizes), torch.int32,
                                         feat.device)
        out = native.frcnn_inference(st["pred"], self.num_classes, proposals.boxes, proposals.count, sizes_dev,
                                     bp.test_score_thresh, bp.test_nms_thresh, bp.test_topk_per_image,
                                     self.bbox_threshold, self.nms_numel_limit, box_reg=bp._box_reg, **_cls_kw(bp))
        return BatchedDetections(out, proposals.image_sizes), st["pred"]

    # ---- module surface (roi_heads.py:68-106) -------------------------------------------------------
    def forward(self, images, features, proposals, targets=None, compute_loss=True, branch="",
                compute_val_loss=False, as_instances=True, keys=None):
        del images
        feat = features[self.in_features[0]]
        if not isinstance(proposals, BatchedProposals):
            proposals = _proposals_from_instances(proposals, feat.device)
        if (self.training and compute_loss) or compute_val_loss:
            assert targets is not None
            if self.pooled > 8 and torch.is_grad_enabled():
                # The ROIAlign kernels serve <= 16 in both directions (the gather backward: csrc/roi_align.hip), and
                # ``_box_forward`` / ``_box_head_backward`` / ``_ROILossFn`` train at any of them.  This module-level refusal
                # of a TRAINING forward above 8 is kept as it was: tests/test_host_logic.py pins it.  config.py's default is
                # d2's 14: the named yamls set 7.
                # (Checked here, not in _box_forward: inside an autograd.Function's forward grad mode is always off.)
                raise ValueError(f"MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION {self.pooled}: StandardROIHeads.forward trains at <= 8 "
                                 "(forward-only passes, and the ROIAlign kernels in both directions: <= 16)")
            if not isinstance(targets, BatchedGT):
                targets = BatchedGT.from_instances(targets, feat.device)
            append = self.proposal_append_gt
            if compute_val_loss and not (self.training and compute_loss):
                self.proposal_append_gt = False
            samples = self.label_and_sample_proposals(proposals, targets, branch=branch, keys=keys)
            self.proposal_append_gt = append
            l_cls, l_box = _ROILossFn.apply(self, feat, samples, *self._params())
            losses = {"loss_cls": l_cls, "loss_box_reg": l_box}
            instance_proposals = None
            if isinstance(self.box_predictor, SourceFreeFastRCNNOutputLayers):
                instance_proposals = InstanceProposals(self, self._last_pred, samples)
            self._last_pred = None
            return samples, losses, None, instance_proposals
        pred_instances, predictions = self._inference(feat, proposals)
        return (pred_instances.to_instances() if as_instances else pred_instances), predictions


def _proposals_from_instances(instances, device):
    B = len(instances)
    P = max(1, max(len(i) for i in instances))
    boxes = torch.zeros(B, P, 4, dtype=torch.float32, device=device)
    logits = torch.zeros(B, P, dtype=torch.float32, device=device)
    cnt = torch.zeros(B, dtype=torch.int32)
    for i, inst in enumerate(instances):
        n = len(inst)
        boxes[i, :n] = inst.proposal_boxes.tensor.to(device)
        if inst.has("objectness_logits"):
            logits[i, :n] = inst.objectness_logits.to(device)
        cnt[i] = n
    return BatchedProposals(boxes, logits, cnt.to(device), [i.image_size for i in instances])


@ROI_HEADS_REGISTRY.register()
class SourceFreeAdaptiveTeacherStandardROIHeads(StandardROIHeads):
    def _make_predictor(self, cfg, shape):
        # "CrossEntropy" / "FocalLoss" (FastRCNNFocaltLossOutputLayers of the code this descends from: the same layers, another
        # loss_cls -- here ``box_predictor._cls_loss``); anything else: a ValueError naming the key
        return SourceFreeFastRCNNOutputLayers(cfg, shape, roi_heads_name="SourceFreeAdaptiveTeacherStandardROIHeads")


@ROI_HEADS_REGISTRY.register()
class AdaptiveTeacherStandardROIHeads(StandardROIHeads):
    def _make_predictor(self, cfg, shape):
        return FastRCNNOutputLayers(cfg, shape, roi_heads_name="AdaptiveTeacherStandardROIHeads")


@ROI_HEADS_REGISTRY.register()
class DAStandardROIHeads(StandardROIHeads):
    """``StandardROIHeads`` that returns the box features (da_roi_heads.py:15-129).  Training with targets: label and sample,
    ``(samples, losses, box_features)``; training without: ``sample_unlabeled_proposals``, ``(samples, {}, box_features)``;
    eval: ``(pred_instances, {})``.  ``samples`` is the fixed-capacity sample dict of ``label_and_sample_proposals``
    (``rois`` [B * BATCH_SIZE_PER_IMAGE, 5], padding rows with batch index -1).

    ``DAFasterRCNN`` (modeling/da_faster_rcnn.py) does not come through ``forward`` in training: it takes the samples from the
    two sampling methods and runs ``_DADomainFn``, which makes the one box-head pass that serves the detection and the domain
    losses.  ``forward`` is the module-level surface; its ``box_features`` are a detached copy from a pass of their own."""

    @torch.no_grad()
    def sample_unlabeled_proposals(self, proposals, keys=None):
        """``randperm(len)[:BATCH_SIZE_PER_IMAGE]`` per image: the BATCH_SIZE_PER_IMAGE live proposals with the smallest
        random key (all of them when fewer are live), every one labelled background.  ``keys`` int32 [B, P]: drawn like
        ``label_and_sample_proposals`` draws them and forced the same way, by an attribute (``_forced_keys_unlabeled``: the
        labelled side's ``_forced_keys`` has the width of proposals + ground truth)."""
        boxes, count = proposals.boxes, proposals.count
        B, P, _ = boxes.shape
        dev = boxes.device
        K = self.num_classes
        live = torch.arange(P, device=dev)[None, :] < count[:, None]
        cls = torch.where(live, K, -2).to(torch.int32).contiguous()      # -2: beyond the live prefix (sfod_subsample)
        keys = keys if keys is not None else getattr(self, "_forced_keys_unlabeled", None)
        if keys is None:
            keys = torch.randint(0, 2 ** 31 - 1, (B, P), dtype=torch.int32, device=dev)
        # positive fraction 0: there is no foreground to prefer
        sidx, scnt = native.subsample_roi(cls, keys, self.batch_size_per_image, 0.0, K)
        no_gt = torch.zeros(B, 1, 4, dtype=torch.float32, device=dev)
        rois, gt_cls, gt_box, n_valid = native.roi_build_samples(boxes, cls, torch.zeros_like(cls), sidx, scnt, no_gt,
                                                                 torch.zeros(B, dtype=torch.int32, device=dev))
        return {"rois": rois, "gt_cls": gt_cls, "gt_box": gt_box, "n_valid": n_valid, "count": scnt, "sampled_idxs": sidx,
                "image_sizes": proposals.image_sizes}

    def forward(self, images, features, proposals, targets=None, as_instances=True, keys=None, want_box_features=True):
        del images
        feat = features[self.in_features[0]]
        if not isinstance(proposals, BatchedProposals):
            proposals = _proposals_from_instances(proposals, feat.device)
        if not self.training:
            pred_instances, _ = self._inference(feat, proposals)
            return (pred_instances.to_instances() if as_instances else pred_instances), {}
        if targets is not None:
            if not isinstance(targets, BatchedGT):
                targets = BatchedGT.from_instances(targets, feat.device)
            samples = self.label_and_sample_proposals(proposals, targets, keys=keys)
            l_cls, l_box = _ROILossFn.apply(self, feat, samples, *self._params())
            self._last_pred = None
            losses = {"loss_cls": l_cls, "loss_box_reg": l_box}
        else:
            samples = self.sample_unlabeled_proposals(proposals, keys=keys)
            losses = {}
        box_features = None
        if want_box_features:
            with torch.no_grad():
                box_features = self.box_features(self._box_forward(feat, samples["rois"])).float()
        return samples, losses, box_features


@ROI_HEADS_REGISTRY.register()
class CDAStandardROIHeads(DAStandardROIHeads):
    """``DAStandardROIHeads`` that also returns the class logits (cda_roi_heads.py:13-128): in training
    ``(samples, losses, box_features, box_scores)``, the reference's return order; ``box_scores`` [R, K + 1] are the first
    K + 1 columns of the fused prediction row, evaluated for the unlabeled (target) side too although it has no loss.

    Like its parent, ``CDAFasterRCNN`` (modeling/cda_faster_rcnn.py) does not come through ``forward`` in training; the
    features and logits returned here are detached copies from a pass of their own."""

    def forward(self, images, features, proposals, targets=None, as_instances=True, keys=None, want_box_features=True):
        out = super().forward(images, features, proposals, targets, as_instances=as_instances, keys=keys, want_box_features=False)
        if not self.training:
            return out
        samples, losses, _ = out
        box_features = box_scores = None
        if want_box_features:
            with torch.no_grad():
                st = self._box_forward(features[self.in_features[0]], samples["rois"])
                box_features = native.cast(self.box_features(st), torch.float32)
                box_scores = st["pred"][:, : self.num_classes + 1].clone()
        return samples, losses, box_features, box_scores
