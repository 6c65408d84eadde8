"""The box-regression definitions the ``sfod_*_opt`` kernels are checked against, written with torch ops so that they
run in any dtype on the CPU (float64 = the reference, float32 = torch's own rounding of the same formulas) and autograd
supplies the gradients.

Restated from Detectron2 (``Box2BoxTransform``, ``_dense_box_regression_loss``, ``FastRCNNOutputLayers.box_reg_loss``) and
fvcore (``smooth_l1_loss``, ``giou_loss``); see include/sfod_hip.h for the same text beside the entry points.  Also the
seeded input generators and tie margins of tests/test_gpu_box_reg_options.py, shared with its CPU self-test.
"""
import math

import torch

SCALE_CLAMP = math.log(1000.0 / 16)
GIOU_EPS = 1e-7


def get_deltas(src, gt, weights):
    wx, wy, ww, wh = weights
    sw, sh = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    scx, scy = src[:, 0] + 0.5 * sw, src[:, 1] + 0.5 * sh
    tw, th = gt[:, 2] - gt[:, 0], gt[:, 3] - gt[:, 1]
    tcx, tcy = gt[:, 0] + 0.5 * tw, gt[:, 1] + 0.5 * th
    return torch.stack((wx * (tcx - scx) / sw, wy * (tcy - scy) / sh, ww * torch.log(tw / sw), wh * torch.log(th / sh)), 1)


def apply_deltas(deltas, src, weights):
    """deltas [N, 4], src [N, 4] -> boxes [N, 4]; SCALE_CLAMP on dw / dh, no clipping"""
    wx, wy, ww, wh = weights
    w, h = src[:, 2] - src[:, 0], src[:, 3] - src[:, 1]
    cx, cy = src[:, 0] + 0.5 * w, src[:, 1] + 0.5 * h
    dx, dy = deltas[:, 0] / wx, deltas[:, 1] / wy
    dw = torch.clamp(deltas[:, 2] / ww, max=SCALE_CLAMP)
    dh = torch.clamp(deltas[:, 3] / wh, max=SCALE_CLAMP)
    pcx, pcy = dx * w + cx, dy * h + cy
    pw, ph = torch.exp(dw) * w, torch.exp(dh) * h
    return torch.stack((pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph), 1)


def smooth_l1_terms(pred, target, beta):
    """per-component terms [N, 4]; beta < 1e-5: |pred - target|"""
    n = (pred - target).abs()
    if beta < 1e-5:
        return n
    return torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)


def giou_terms(p, g, eps=GIOU_EPS):
    """per-pair terms [N] of fvcore's giou_loss"""
    iw = torch.min(p[:, 2], g[:, 2]) - torch.max(p[:, 0], g[:, 0])
    ih = torch.min(p[:, 3], g[:, 3]) - torch.max(p[:, 1], g[:, 1])
    inter = torch.where((iw > 0) & (ih > 0), iw * ih, torch.zeros_like(iw))
    union = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1]) + (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]) - inter
    enc = (torch.max(p[:, 2], g[:, 2]) - torch.min(p[:, 0], g[:, 0])) * (torch.max(p[:, 3], g[:, 3]) - torch.min(p[:, 1], g[:, 1]))
    return 1 - inter / (union + eps) + (enc - union) / (enc + eps)


def box_reg_terms(deltas, src, gt, weights, loss_type, beta):
    """terms of the foreground boxes (any shape; the loss is their sum times the head's normaliser)"""
    if loss_type == "giou":
        return giou_terms(apply_deltas(deltas, src, weights), gt)
    assert loss_type == "smooth_l1"
    return smooth_l1_terms(deltas, get_deltas(src, gt, weights), beta)


def evaluate(deltas, src, gt, weights, loss_type, beta, scale, dtype):
    """-> (loss = scale * sum of terms, sum of |terms| * scale, d loss / d deltas) in ``dtype`` on the CPU"""
    d = deltas.to(dtype).clone().requires_grad_(True)
    terms = box_reg_terms(d, src.to(dtype), gt.to(dtype), weights, loss_type, beta)
    loss = terms.sum() * scale
    loss.backward()
    return loss.detach(), (terms.detach().abs().sum() * abs(scale)), d.grad


def gate(ref64, val32, s):
    """4 x max(torch-fp32's distance from float64, 2^-24 * s): the tolerance of a device quantity whose definition torch
    itself evaluates in fp32 at distance |val32 - ref64|; s = the sum of absolute terms (a loss) or the largest magnitude
    (a gradient tensor).  -> (gate, e32)"""
    e32 = (val32.double() - ref64.double()).abs().max().item()
    return 4.0 * max(e32, 2.0 ** -24 * float(s)), e32


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------
def make_boxes(n, g):
    """proposal / anchor boxes: xy uniform in [0, 900), sizes uniform in [16, 266); fp32"""
    xy = torch.rand(n, 2, generator=g, dtype=torch.float64) * 900
    wh = torch.rand(n, 2, generator=g, dtype=torch.float64) * 250 + 16
    return torch.cat([xy, xy + wh], 1).float()


def make_gt(boxes, g, loss_type):
    """smooth-L1: box + N(0, 6) per coordinate; GIoU: box + N(0, 12), at least 4 px wide and high, every sixth row shifted by
    +400 px (disjoint from its box: sizes are < 266)"""
    n = boxes.shape[0]
    if loss_type == "giou":
        gt = boxes.double() + torch.randn(n, 4, generator=g, dtype=torch.float64) * 12
        gt[:, 2:] = torch.max(gt[:, 2:], gt[:, :2] + 4)
        gt[::6] += 400
    else:
        gt = boxes.double() + torch.randn(n, 4, generator=g, dtype=torch.float64) * 6
        gt[:, 2:] = torch.max(gt[:, 2:], gt[:, :2] + 1)
    return gt.float()


def make_deltas(n, g):
    return (torch.randn(n, 4, generator=g, dtype=torch.float64) * torch.tensor([1, 1, 0.5, 0.5], dtype=torch.float64)).float()


def tie_margins(deltas, src, gt, weights, loss_type, beta):
    """float64 distances from the points where the definition is not differentiable (or where fp32 and float64 may take
    different branches).  GIoU: min |p - g| over coordinates, min |overlap extent|; smooth-L1: min | |d| - beta |."""
    d, s, t = deltas.double(), src.double(), gt.double()
    if loss_type == "giou":
        p = apply_deltas(d, s, weights)
        coord = (p - t).abs().min().item()
        iw = torch.min(p[:, 2], t[:, 2]) - torch.max(p[:, 0], t[:, 0])
        ih = torch.min(p[:, 3], t[:, 3]) - torch.max(p[:, 1], t[:, 1])
        disjoint = int(((iw <= 0) | (ih <= 0)).sum())
        return {"coord": coord, "extent": torch.cat([iw, ih]).abs().min().item(), "disjoint": disjoint}
    n = (d - get_deltas(s, t, weights)).abs()
    out = {"zero": n.min().item()}
    if beta >= 1e-5:
        out["beta"] = (n - beta).abs().min().item()
    return out


def assert_margins(m, loss_type, px=0.01, beta_margin=1e-4):
    """the seeded cases keep 0.01 px / 1e-4; inputs a model produced itself (module tests) are held to ``px`` / ``beta_margin``
    of the caller's choosing, which must stay well above fp32's rounding of the compared values"""
    if loss_type == "giou":
        assert m["coord"] >= px and m["extent"] >= px, m
    else:
        assert m.get("beta", 1.0) >= beta_margin and m["zero"] > 0, m
