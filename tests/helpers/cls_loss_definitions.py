"""Classification losses of the Fast R-CNN head, restated literally in torch ops (evaluated on the CPU, float64 or float32).

Neither Detectron2 nor Unbiased Teacher is importable here and the reference carries the focal branch only as a comment
(daod/modeling/roi_heads/source_free_adaptive_teacher_roi_heads.py:19,56-57), so the definitions are written out:

* ``FocalLoss`` (Unbiased Teacher ``FastRCNNFocalLoss`` / ``FocalLoss.forward``): per live row
  ``CE = cross_entropy(scores[r, :K+1], c, reduction="none")``, ``p = exp(-CE)``, ``term = (1 - p) ** gamma * CE``,
  ``loss_cls = sum(term) / N``, N = the number of live rows.
* sigmoid CE (Detectron2 ``FastRCNNOutputLayers.sigmoid_cross_entropy_loss``): target = the one-hot of ``c`` over K + 1
  columns with the last column dropped, ``loss_cls = sum(binary_cross_entropy_with_logits(scores[:, :K], target, "none")) / N``;
  ``predict_probs`` is ``sigmoid`` of all K + 1 columns.
* ``CrossEntropy``: ``sum(cross_entropy(..., "none")) / N`` (the mean over the live rows).

Rows with class -1 are padding and take no part.
"""
import torch
import torch.nn.functional as F

KINDS = ("ce", "focal", "sigmoid")


def live_rows(classes):
    return classes >= 0


def cls_terms(scores, classes, kind, gamma=1.5):
    """scores [n, K + 1], classes [n] in [0, K] (live rows only) -> the per-row loss terms [n], in scores' dtype"""
    c = classes.long()
    K = scores.shape[1] - 1
    if kind == "sigmoid":
        target = F.one_hot(c, K + 1)[:, :K].to(scores.dtype)
        return F.binary_cross_entropy_with_logits(scores[:, :K], target, reduction="none").sum(dim=1)
    ce = F.cross_entropy(scores, c, reduction="none")
    if kind == "ce":
        return ce
    assert kind == "focal"
    p = torch.exp(-ce)
    return (1 - p) ** gamma * ce


def cls_loss(scores, classes, kind, gamma=1.5, normalizer=None):
    """the loss over the live rows of ``scores`` [R, >= K + 1 columns given as [R, K + 1]] -> (loss, sum of |terms| / N)"""
    live = live_rows(classes)
    t = cls_terms(scores[live], classes[live], kind, gamma)
    n = float(normalizer if normalizer is not None else int(live.sum()))
    return t.sum() / n, t.abs().sum() / n


def evaluate(scores, classes, kind, gamma, grad_mul, dtype, normalizer=None):
    """-> (loss, sum|terms| / N, grad_mul * d loss / d scores [R, K + 1]) evaluated in ``dtype`` by torch autograd"""
    z = scores.to(dtype).clone().requires_grad_(True)
    loss, s = cls_loss(z, classes, kind, gamma, normalizer)
    (g,) = torch.autograd.grad(loss, z)
    return loss.detach(), s.detach(), g * grad_mul


def probs(scores, sigmoid):
    """predict_probs: softmax over the K + 1 columns, or under USE_SIGMOID_CE the sigmoid of every column"""
    return torch.sigmoid(scores) if sigmoid else torch.softmax(scores, dim=1)


def gate(ref64, val32, s):
    """The project's gate (tests/test_gpu_box_reg_options.py): 4 x max(torch-fp32's distance from float64, 2^-24 * s); where
    torch's fp32 evaluation is not finite the floor alone.  -> (gate, e32)"""
    if not bool(torch.isfinite(val32).all()):
        return 4.0 * 2.0 ** -24 * float(s), float("nan")
    e32 = (val32.double() - ref64.double()).abs().max().item()
    return 4.0 * max(e32, 2.0 ** -24 * float(s)), e32
