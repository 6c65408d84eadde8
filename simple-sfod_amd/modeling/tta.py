"""``TEST.AUG``: multi-scale and flip test-time augmentation (Detectron2's ``GeneralizedRCNNWithTTA`` for boxes).

Per input dict: the test-size tensor is resized to every ``TEST.AUG.MIN_SIZES`` entry (and mirrored, with ``FLIP``) by the
Pillow-exact resize kernel, the flip in the same launch; each augmentation goes through ``model.inference(...,
do_postprocess=False)``; ``sfod_tta_merge`` takes all detections of the batch back to the native frames and the teacher
post-processing's sort -> class-wise NMS -> top-k chain merges them (``native.tta_merge``).  Nothing between the first resize
and the final ``Instances`` copies to the host: the passes hand over their fixed-capacity containers, the transform tables
are host constants cached on the device (modeling/tta_options.py).

One deliberate deviation from Detectron2: its ``_batch_inference`` runs the augmented inputs in chunks of 3 of MIXED sizes,
zero-padded to the largest, and the padding leaks into the border activations.  Here a pass holds tensors of one size only:
one augmentation of one image and, with ``FLIP``, its mirrored twin.
"""
import torch
import torch.nn as nn

from .. import native
from .batched import BatchedDetections
from .tta_options import TTAOptions

SCORE_THRESH = 1e-8          # d2 _merge_detections: fast_rcnn_inference_single_image(..., 1e-8, NMS_THRESH_TEST, DETECTIONS_PER_IMAGE)


class GeneralizedRCNNWithTTA(nn.Module):
    def __init__(self, cfg, model):
        super().__init__()
        self.options = TTAOptions(cfg)      # ValueError naming the key
        if not hasattr(model, "inference") or getattr(model, "roi_heads", None) is None:
            raise TypeError(f"TEST.AUG needs a meta-architecture whose eval path is inference() with ROI heads, got "
                            f"{type(model).__name__}")
        self.cfg = cfg
        self.model = model
        self.num_classes = int(cfg.MODEL.ROI_HEADS.NUM_CLASSES)
        self.nms_thresh = float(cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST)
        self.max_det = self.options.max_det
        self.numel_limit = int(getattr(model.roi_heads, "nms_numel_limit", 20000))
        # the wrapper is born in the model's mode: inference_on_dataset restores the WRAPPER's previous mode afterwards, and
        # that must be the model's own
        nn.Module.train(self, model.training)

    @property
    def device(self):
        return self.model.device

    def plan_of(self, inp):
        h, w = int(inp["image"].shape[1]), int(inp["image"].shape[2])
        return self.options.plan(h, w, int(inp.get("height", h)), int(inp.get("width", w)))

    def augmented_inputs(self, inp, plan, index):
        """the tensors of pass ``index`` (one MIN_SIZES entry): the resize and, with FLIP, the mirrored resize, one launch each"""
        ha, wa = plan.sizes[index]
        img = inp["image"].to(self.device, non_blocking=True)
        out = []
        for f in range(self.options.per_size):
            out.append({"image": native.weak_augment_u8(img, None, (ha, wa), native.FLIP_HORIZONTAL if f else native.FLIP_NONE),
                        "height": ha, "width": wa})
        return out

    @torch.no_grad()
    def merged(self, batched_inputs):
        """-> BatchedDetections at the native frame sizes; no host synchronisation"""
        if self.model.training:
            raise RuntimeError("GeneralizedRCNNWithTTA runs a model in eval mode only (call model.eval() first)")
        opt = self.options
        plans = [self.plan_of(x) for x in batched_inputs]
        parts = {"det_boxes": [], "det_scores": [], "det_classes": [], "det_count": []}
        for inp, plan in zip(batched_inputs, plans):
            for index in range(len(plan.sizes)):
                res = self.model.inference(self.augmented_inputs(inp, plan, index), do_postprocess=False, as_instances=False)
                if res.d["det_scores"].shape[1] != self.max_det:
                    raise RuntimeError(f"the model's passes hold {res.d['det_scores'].shape[1]} detections per image, "
                                       f"TEST.DETECTIONS_PER_IMAGE is {self.max_det}")
                for k, v in parts.items():
                    v.append(res.d[k])
        B, A, cap = len(batched_inputs), opt.num_aug, self.max_det
        dev = self.device
        table = native.dev_const(tuple(p.table for p in plans), torch.float32, dev)
        sizes = native.dev_const(tuple(p.native_hw for p in plans), torch.int32, dev)
        out = native.tta_merge(torch.cat(parts["det_boxes"]).view(B, A, cap, 4), torch.cat(parts["det_scores"]).view(B, A, cap),
                               torch.cat(parts["det_classes"]).view(B, A, cap), torch.cat(parts["det_count"]).view(B, A),
                               table, sizes, self.num_classes, SCORE_THRESH, self.nms_thresh, self.max_det, self.numel_limit)
        return BatchedDetections(out, [p.native_hw for p in plans])

    def forward(self, batched_inputs):
        """list of input dicts -> list of ``{"instances": Instances((H0, W0))}`` with pred_boxes, scores, pred_classes (d2:
        no further detector_postprocess)"""
        if not batched_inputs:
            return []
        return [{"instances": inst} for inst in self.merged(batched_inputs).to_instances()]
