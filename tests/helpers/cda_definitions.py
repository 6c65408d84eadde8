"""The class-conditioned domain losses of conditional DA Faster R-CNN as plain torch definitions
(``CDAFasterRCNN.conditional_instance_dc_loss`` / ``conditional_consistency_loss`` and ``MultiLinearMap``,
daod/modeling/meta_arch/cda_faster_rcnn.py:22-33, 263-300; ``entropy``, daod/modeling/utils.py), usable in float64 and
float32; gradients by autograd.  The pieces are the ones csrc/cda_condition.hip computes -- condition, entropy weight, weighted
BCE, contraction -- and the module's two losses are composed from them and tests/helpers/da_definitions.py.
Only tests/ and tools/record_cda_golden.py import this module.
"""
import torch

from helpers import da_definitions as D

ENTROPY_EPS = 1e-5


def condition(scores):
    """class logits [R, C] -> detached probabilities"""
    return torch.softmax(scores, dim=1).detach()


def conditioned(f, p):
    """f [R, D], p [R, C] -> [R, C * D], element c * D + d = p[r, c] * f[r, d]"""
    return (p[:, :, None] * f[:, None, :]).reshape(f.shape[0], -1)


def entropy_weight(p):
    """1 + exp(-H), H = -sum_c p_c log(p_c + 1e-5) (the constant in p's dtype)"""
    h = -(p * torch.log(p + torch.tensor(ENTROPY_EPS, dtype=p.dtype))).sum(dim=1)
    return 1.0 + torch.exp(-h)


def weighted_bce(z, label, w, live=None):
    """-> (sum w bce / sum w over the live elements, sum w |bce| / sum w); no live element: 0"""
    t = D.bce_terms(z, label)
    if live is not None:
        t, w = t[live], w[live]
    if t.numel() == 0:
        return t.sum(), t.sum()
    return (w * t).sum() / w.sum(), (w * t.abs()).sum() / w.sum()


def contraction(dx, p):
    """dx [R, C * D], p [R, C] -> [R, D]: sum_c p[r, c] dx[r, c * D + d]"""
    R, C = p.shape
    return torch.einsum("rc,rcd->rd", p, dx.reshape(R, C, -1))


def conditional_instance_dc_loss(box_features, scores, w_ins, label, w_n, entropy, masks=None, live=None):
    p = condition(scores)
    z = D.ins_head(D.gradient_scalar(conditioned(box_features, p), -1.0 * w_n), w_ins, masks)[:, 0]
    if entropy:
        return weighted_bce(z, label, entropy_weight(p), live)[0]
    return D.bce(z, label, live)[0]


def conditional_consistency_loss(feat, box_features, scores, rois, w_img, w_ins, w_i, w_n, w_c, pooled, scale, sampling_ratio=0,
                                 aligned=True, masks=None, pool="matrices"):
    z_img = D.img_head(D.gradient_scalar(feat, w_c * w_i), w_img)[:, 0]
    x = conditioned(box_features, condition(scores))
    z_ins = D.ins_head(D.gradient_scalar(x, w_c * w_n), w_ins, masks)[:, 0]
    return D.consistency(z_img, z_ins, rois, pooled, scale, sampling_ratio, aligned, pool)[0]


def evaluate_losses(feat, box_features, scores, rois, w_img, w_ins, weights, label, pooler, entropy, masks, pool="matrices",
                    extra_leaves=None):
    """``da_definitions.evaluate_losses`` for the conditional architecture: the three loss methods on one domain, each with its
    own autograd gradients -> {which: (value, {leaf name: gradient})}.  The instance-level terms are evaluated on the live rows
    only (a padding row's logits may hold anything); their box-feature gradient comes back at full height, zero on padding."""
    w_i, w_n, w_c = weights
    pooled, sr, aligned = pooler
    live = rois[:, 0] >= 0
    scale = 1.0 / 32
    leaves = {"feat": feat, "box_features": box_features}
    leaves.update({"w_img/" + k: v for k, v in w_img.items()})
    leaves.update({"w_ins/" + k: v for k, v in w_ins.items()})
    leaves.update(extra_leaves or {})
    bf, sc = box_features[live], scores[live].to(feat.dtype)
    lm = [[m[live] for m in pair] for pair in masks] if masks is not None else None
    losses = {
        "img": lambda: D.image_dc_loss(feat, w_img, label, w_i),
        "ins": lambda: conditional_instance_dc_loss(bf, sc, w_ins, label, w_n, entropy, lm[0] if lm is not None else None),
        "cons": lambda: conditional_consistency_loss(feat, bf, sc, rois[live].to(feat.dtype), w_img, w_ins, w_i, w_n, w_c, pooled,
                                                     scale, sr, aligned, lm[1] if lm is not None else None, pool)}
    out = {}
    for which, fn in losses.items():
        loss = fn()
        grads = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True, retain_graph=True)
        out[which] = (loss.detach(), {n: g for n, g in zip(leaves, grads) if g is not None})
    return out


def one_fc1_form(x, w_ins, dz_fn, w_n, w_c, masks):
    """The execution the device path uses, in x's dtype: fc1 + ReLU once on the conditioned feature ``x`` [R, K], the two
    evaluations from there under their own masks; ``dz_fn(z_ins, z_cons)`` -> the two logit gradients.  Backward by hand:
    the parameters of fc1 take ``d1_ins + d1_cons``, its input ``-w_n d1_ins + w_c w_n d1_cons``.
    -> (z_ins, z_cons, dx, {"fc1.weight": .., "fc1.bias": .., "fc2.weight": .., ..})"""
    W1, b1, W2, b2, W3, b3 = (w_ins[k] for k in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias"))
    r1 = torch.relu(x @ W1.t() + b1)

    def tail(m):
        z1 = r1 * m[0].to(r1.dtype) * 2.0 if m is not None else r1
        r2 = torch.relu(z1 @ W2.t() + b2)
        z2 = r2 * m[1].to(r1.dtype) * 2.0 if m is not None else r2
        return z1, r2, z2, (z2 @ W3.t() + b3)[:, 0]

    evs = [tail(masks[0] if masks is not None else None), tail(masks[1] if masks is not None else None)]
    dzs = dz_fn(evs[0][3], evs[1][3])
    d1s, g = [], {k: torch.zeros_like(v) for k, v in w_ins.items()}
    for (z1, r2, z2, _), dz, m in zip(evs, dzs, masks if masks is not None else (None, None)):
        dz = dz[:, None]
        g["fc3.weight"] += dz.t() @ z2
        g["fc3.bias"] += dz.sum(0)
        d2 = dz @ W3
        if m is not None:
            d2 = d2 * m[1].to(d2.dtype) * 2.0
        d2 = d2 * (r2 > 0)
        g["fc2.weight"] += d2.t() @ z1
        g["fc2.bias"] += d2.sum(0)
        d1 = d2 @ W2
        if m is not None:
            d1 = d1 * m[0].to(d1.dtype) * 2.0
        d1s.append(d1 * (r1 > 0))
    d1_par = d1s[0] + d1s[1]
    g["fc1.weight"] = d1_par.t() @ x
    g["fc1.bias"] = d1_par.sum(0)
    dx = (d1s[0] * (-w_n) + d1s[1] * (w_c * w_n)) @ W1
    return evs[0][3], evs[1][3], dx, g
