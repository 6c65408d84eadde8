"""Definitions of the proposal and matcher options (test infrastructure, CPU, fp32 torch), built on ``oracle.box_ops`` /
``oracle.model``: Detectron2's ``_create_grid_offsets`` with an offset, ``Boxes.inside_box``, ``find_top_rpn_proposals`` with a
minimum size, and ``Matcher`` [lo, hi] / [0, -1, 1] + ``_sample_proposals``' class targets."""
import torch

from oracle import box_ops as OB


def grid_anchors(hf, wf, stride, cell, offset=0.0):
    """Anchors of one level in (y, x, a) order: float32(offset * stride) + float32(x * stride), one fp32 add -- what a float32
    ``torch.arange(offset * stride, n * stride, step=stride)`` yields on a GPU."""
    shift = torch.tensor(offset * stride, dtype=torch.float32)
    sx = shift + (torch.arange(wf) * stride).float()
    sy = shift + (torch.arange(hf) * stride).float()
    yy, xx = torch.meshgrid(sy, sx, indexing="ij")
    xx, yy = xx.reshape(-1), yy.reshape(-1)
    shifts = torch.stack((xx, yy, xx, yy), dim=1)
    return (shifts.view(-1, 1, 4) + cell.float().view(1, -1, 4)).reshape(-1, 4)


def inside_box(boxes, image_size, boundary_threshold=0):
    """d2 Boxes.inside_box; image_size = (h, w); fp32 comparisons"""
    h, w = image_size
    t = torch.tensor(float(boundary_threshold), dtype=torch.float32)
    hh, ww = torch.tensor(float(h), dtype=torch.float32) + t, torch.tensor(float(w), dtype=torch.float32) + t
    return (boxes[:, 0] >= -t) & (boxes[:, 1] >= -t) & (boxes[:, 2] < ww) & (boxes[:, 3] < hh)


def label_anchors(anchors, gt, thresholds, image_size=None, boundary_thresh=-1):
    """RPN.label_and_sample_anchors before the subsampling: Matcher(thresholds, [0, -1, 1], low quality on), then anchors
    outside the image grown by ``boundary_thresh`` (>= 0) become -1.  -> (matched idx int64, labels int8)"""
    idx, lab = OB.matcher(OB.pairwise_iou(gt, anchors), list(thresholds), [0, -1, 1], True)
    lab = lab.clone()
    if boundary_thresh >= 0:
        lab[~inside_box(anchors, image_size, boundary_thresh)] = -1
    return idx, lab


def rpn_proposals(anchors, logits, deltas, image_sizes, pre_topk, post_topk, nms_thresh, min_size=0.0,
                  weights=(1.0, 1.0, 1.0, 1.0)):
    """find_top_rpn_proposals, one level: decode, top-k by logit (stable), clip, nonempty(min_size), NMS, post top-k
    -> [(boxes [n, 4], logits [n])]"""
    out = []
    for n in range(logits.shape[0]):
        props = OB.apply_deltas(deltas[n], anchors, weights)
        k = min(pre_topk, logits.shape[1])
        order = torch.sort(logits[n], descending=True, stable=True)[1][:k]
        boxes = OB.clip_boxes(props[order], image_sizes[n])
        scores = logits[n][order]
        keep = OB.nonempty(boxes, float(min_size))
        boxes, scores = boxes[keep], scores[keep]
        keep = OB.nms(boxes, scores, nms_thresh)[:post_topk]
        out.append((boxes[keep], scores[keep]))
    return out


def roi_classes(boxes, gt_boxes, gt_classes, lo, hi, num_classes):
    """Matcher([lo, hi], [0, -1, 1], no low quality) + _sample_proposals' targets: class of the matched ground truth at
    IoU >= hi, -1 (ignored) in [lo, hi), ``num_classes`` below; all ``num_classes`` without ground truth.  lo == hi is
    Matcher([t], [0, 1]).  -> (matched idx int64, cls int64)"""
    if len(gt_boxes) == 0:
        return torch.zeros(len(boxes), dtype=torch.int64), torch.full((len(boxes),), num_classes, dtype=torch.int64)
    M = OB.pairwise_iou(gt_boxes, boxes)
    if lo == hi:
        idx, lab = OB.matcher(M, [hi], [0, 1], False)
    else:
        idx, lab = OB.matcher(M, [lo, hi], [0, -1, 1], False)
    cls = gt_classes.long()[idx].clone()
    cls[lab == 0] = num_classes
    cls[lab == -1] = -1
    return idx, cls
