"""Definitions and bounds for the box-head architecture options (MODEL.ROI_BOX_HEAD.{NUM_CONV, CONV_DIM, NUM_FC, FC_DIM, NORM}).

Definitions: torch float64 on the CPU -- ``F.conv2d`` (3x3, pad 1), ``F.group_norm(x, 32, w, b, 1e-5)``, ``F.linear``, ``relu``,
gradients by autograd -- composed with ``oracle.model.fast_rcnn_losses`` as it is.

Bounds of the GroupNorm kernels (sfod_group_norm_relu_fwd / _bwd, include/sfod_hip.h).  They count the roundings of an honest
fp32 evaluation in the kernel's order, the way definition_check.bn_forward_bound / bn_backward_bounds do; none is fitted to a
kernel (tests/test_box_head_options_host.py validates them against a torch fp32 evaluation on the CPU).  u = 2^-24, LAMBDA = 8
the project's allowance for an fp32 sum of n terms (LAMBDA sqrt(n) u sum |terms|), n = PP * C / groups the elements of one
(ROI, group), mean|.| the mean over those elements, d = y - mean, xhat = d * rstd.

  statistics
    e_mu   = (LAMBDA sqrt(n) + 1) u mean|y|                           the sum of n terms, one division
    e_var  = (LAMBDA sqrt(n) + 5) u var + e_mu^2                      d rounded (2 u var), squares and sum, division; a mean off
                                                                      by e_mu adds exactly e_mu^2 (the cross term vanishes)
    e_rs   = 0.5 e_var / (var + eps) + 5 u      (relative)            var + eps, sqrt, 1 / x: one rounding each, two spare
    tol_mean = e_mu,  tol_rstd = rstd e_rs
  forward, z = relu(fma(xhat, gamma, beta))
    e_xh   = rstd (e_mu + u |d|) + |xhat| (e_rs + u)                  the mean's error AMPLIFIED BY rstd, d's rounding, rstd's
                                                                      error, the product's rounding
    bound  = |gamma| e_xh + u (|xhat gamma| + |beta|) + r_out |z|     one rounding of the fused multiply-add; ReLU is 1-Lipschitz
  backward, gz = dz [pre-activation > 0], g = gz gamma, m1 = mean_grp(g), m2 = mean_grp(g xhat), dy = rstd (g - m1 - xhat m2)
    e_m1   = (LAMBDA sqrt(n) + 3) u mean_grp|g|                       product, sum, division
    e_m2   = (LAMBDA sqrt(n) + 4) u mean_grp|g xhat| + mean_grp(|g| e_xh)
    dy     : rstd (3 u (|g| + |m1| + |xhat m2|) + e_m1 + e_xh |m2| + |xhat| e_m2) + |dy| (e_rs + u) + r_out |dy|
    dbeta  : (LAMBDA sqrt(M) + 1) u sum |gz|,   M = R * PP            (+ u (|before| + |dbeta|) when accumulating)
    dgamma : (LAMBDA sqrt(M) + 2) u sum |gz xhat| + sum |gz| e_xh     (likewise)
  An element whose defined pre-activation lies within its forward bound (without r_out) of zero may take the other side of
  the gate in fp32: such elements are left out of the dy comparison (``near_gate``; the tests cap their share at 0.1 %).
Only tests/ import this module.
"""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from helpers.definition_check import LAMBDA, U32, _r_out

GROUPS, EPS = 32, 1e-5


# ---- GroupNorm on [R, PP, C] (the kernels' layout) --------------------------------------------------------------------------
def _nchw(t):            # [R, PP, C] -> [R, C, PP]: F.group_norm wants channels second
    return t.permute(0, 2, 1)


def gn_forward(y, gamma, beta, groups=GROUPS, eps=EPS, relu=True):
    """float64 definition -> namespace: z (activated), pre (pre-activation), mean / rstd [R, groups], xhat, and the pieces of
    the bounds.  y [R, PP, C] (the kernel's exact input values)."""
    y, gamma, beta = y.detach().double(), gamma.detach().double(), beta.detach().double()
    R, PP, C = y.shape
    cpg = C // groups
    n = PP * cpg
    pre = _nchw(F.group_norm(_nchw(y), groups, gamma, beta, eps))
    yg = y.view(R, PP, groups, cpg)
    mean = yg.mean(dim=(1, 3))
    d = yg - mean.view(R, 1, groups, 1)
    var = (d * d).mean(dim=(1, 3))
    rstd = torch.rsqrt(var + eps)
    xhat = (d * rstd.view(R, 1, groups, 1)).reshape(R, PP, C)
    assert torch.allclose(xhat * gamma + beta, pre, rtol=1e-9, atol=1e-9)        # the restatement IS F.group_norm's
    sq = math.sqrt(n)
    e_mu = (LAMBDA * sq + 1) * U32 * yg.abs().mean(dim=(1, 3))
    e_var = (LAMBDA * sq + 5) * U32 * var + e_mu * e_mu
    e_rs = 0.5 * e_var / (var + eps) + 5 * U32

    def per_elem(t):      # [R, groups] -> [R, PP, C]
        return t.view(R, 1, groups, 1).expand(R, PP, groups, cpg).reshape(R, PP, C)
    e_xh = per_elem(rstd) * (per_elem(e_mu) + U32 * d.reshape(R, PP, C).abs()) + xhat.abs() * (per_elem(e_rs) + U32)
    z = torch.relu(pre) if relu else pre
    return SimpleNamespace(z=z, pre=pre, mean=mean, rstd=rstd, xhat=xhat, n=n, groups=groups, cpg=cpg, e_mu=e_mu, e_rs=e_rs,
                           e_xh=e_xh, gamma=gamma, beta=beta, tol_mean=e_mu, tol_rstd=rstd * e_rs, per_elem=per_elem,
                           pre_bound=gamma.abs() * e_xh + U32 * ((xhat * gamma).abs() + beta.abs()))


def gn_forward_bound(defn, out="fp32"):
    """per-element bound of the kernel's z against ``defn.z`` (module docstring), output rounding included"""
    return defn.pre_bound + _r_out(defn.z, out)


def near_gate(defn):
    """elements whose defined pre-activation is within its forward bound of zero: fp32 may gate them the other way"""
    return defn.pre.abs() <= defn.pre_bound


def gn_backward(defn, y, dz, relu=True):
    """float64 definition by autograd through F.group_norm (+ relu) -> namespace dy, dgamma, dbeta and the bounds' pieces."""
    y = y.detach().double().clone().requires_grad_(True)
    ga, be = defn.gamma.clone().requires_grad_(True), defn.beta.clone().requires_grad_(True)
    z = _nchw(F.group_norm(_nchw(y), defn.groups, ga, be, EPS))
    if relu:
        z = torch.relu(z)
    dz = dz.detach().double()
    z.backward(dz)
    R, PP, C = y.shape
    gz = dz * (defn.pre > 0) if relu else dz
    g = gz * defn.gamma

    def grp_mean(t):      # [R, PP, C] -> [R, groups]
        return t.view(R, PP, defn.groups, defn.cpg).mean(dim=(1, 3))
    m1, m2 = grp_mean(g), grp_mean(g * defn.xhat)
    return SimpleNamespace(dy=y.grad, dgamma=ga.grad, dbeta=be.grad, gz=gz, g=g, m1=m1, m2=m2,
                           m1_abs=grp_mean(g.abs()), m2_abs=grp_mean((g * defn.xhat).abs()),
                           m2_exh=grp_mean(g.abs() * defn.e_xh))


def gn_backward_bounds(defn, bw, out="fp32"):
    """-> (tol_dbeta [C], tol_dgamma [C], bound of dy [R, PP, C]) (module docstring)"""
    R, PP, C = bw.dy.shape
    sq, M = math.sqrt(defn.n), R * PP
    pe = defn.per_elem
    e_m1 = (LAMBDA * sq + 3) * U32 * bw.m1_abs
    e_m2 = (LAMBDA * sq + 4) * U32 * bw.m2_abs + bw.m2_exh
    xa = defn.xhat.abs()
    inner = 3 * U32 * (bw.g.abs() + pe(bw.m1).abs() + xa * pe(bw.m2).abs()) + pe(e_m1) + defn.e_xh * pe(bw.m2).abs() + xa * pe(e_m2)
    bnd = pe(defn.rstd) * inner + bw.dy.abs() * (pe(defn.e_rs) + U32) + _r_out(bw.dy, out)
    tol_db = (LAMBDA * math.sqrt(M) + 1) * U32 * bw.gz.abs().sum(dim=(0, 1))
    tol_dg = (LAMBDA * math.sqrt(M) + 2) * U32 * (bw.gz * defn.xhat).abs().sum(dim=(0, 1)) + (bw.gz.abs() * defn.e_xh).sum(dim=(0, 1))
    return tol_db, tol_dg, bnd


# ---- an honest fp32 evaluation in the kernel's order, on the CPU (validates the bounds; never compared with a kernel) -----
def gn_fp32_kernel_order(y, gamma, beta, dz=None, groups=GROUPS, eps=EPS):
    """fp32 throughout: per channel a running sum over the pixels, the group's channels added one after the other, sum / n;
    then the centred squares the same way; rstd = 1 / sqrt(var + eps); xhat = (y - mean) * rstd, z = relu(xhat * gamma + beta).
    With ``dz`` also the backward in the kernel's order -> (z, mean, rstd[, dy, dgamma, dbeta])."""
    y, gamma, beta = y.float(), gamma.float(), beta.float()
    R, PP, C = y.shape
    cpg = C // groups
    n = torch.tensor(float(PP * cpg), dtype=torch.float32)

    def grp_sum(t):       # [R, PP, C] fp32 -> [R, groups]: pixels first (running sum), then the group's channels
        acc = torch.zeros(R, C, dtype=torch.float32)
        for p in range(PP):
            acc = acc + t[:, p]
        acc = acc.view(R, groups, cpg)
        s = torch.zeros(R, groups, dtype=torch.float32)
        for c in range(cpg):
            s = s + acc[:, :, c]
        return s

    def pe(t):
        return t.view(R, 1, groups, 1).expand(R, PP, groups, cpg).reshape(R, PP, C)
    mean = grp_sum(y) / n
    d = y - pe(mean)
    var = grp_sum(d * d) / n
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))
    xhat = d * pe(rstd)
    pre = xhat * gamma + beta
    z = torch.relu(pre)
    if dz is None:
        return z, mean, rstd
    gz = dz.float() * (pre > 0)
    g = gz * gamma
    m1, m2 = grp_sum(g) / n, grp_sum(g * xhat) / n
    dy = pe(rstd) * ((g - pe(m1)) - xhat * pe(m2))
    dbeta = torch.zeros(C, dtype=torch.float32)
    dgamma = torch.zeros(C, dtype=torch.float32)
    for r in range(R):
        dbeta = dbeta + gz[r].sum(0)
        dgamma = dgamma + (gz[r] * xhat[r]).sum(0)
    return z, mean, rstd, dy, dgamma, dbeta


def gn_case(R, PP, C, seed, pad_rows=0):
    """the tests' inputs: y = randn + 0.3, gamma / beta = randn, dz = randn; the last ``pad_rows`` ROIs all zero (y and dz)"""
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(R, PP, C, generator=g) + 0.3
    dz = torch.randn(R, PP, C, generator=g)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    if pad_rows:
        y[R - pad_rows:] = 0
        dz[R - pad_rows:] = 0
    return y, dz, gamma, beta


# ---- the head as a float64 composition -------------------------------------------------------------------------------------
def box_head_forward(sd, pooled, num_conv, num_fc, norm, prefix="roi_heads."):
    """pooled [R, C, P, P] (NCHW, any float dtype; computed in ITS dtype) through Detectron2's FastRCNNConvFCHead and the
    predictor with the state dict ``sd`` -> (scores, deltas, box_features)"""
    w = lambda k: sd[prefix + k].to(pooled.dtype)
    x = pooled
    for k in range(1, num_conv + 1):
        b = None if norm else w(f"box_head.conv{k}.bias")
        x = F.conv2d(x, w(f"box_head.conv{k}.weight"), b, padding=1)
        if norm:
            x = F.group_norm(x, GROUPS, w(f"box_head.conv{k}.norm.weight"), w(f"box_head.conv{k}.norm.bias"), EPS)
        x = torch.relu(x)
    x = x.flatten(1)
    for k in range(1, num_fc + 1):
        x = torch.relu(F.linear(x, w(f"box_head.fc{k}.weight"), w(f"box_head.fc{k}.bias")))
    return (F.linear(x, w("box_predictor.cls_score.weight"), w("box_predictor.cls_score.bias")),
            F.linear(x, w("box_predictor.bbox_pred.weight"), w("box_predictor.bbox_pred.bias")), x)
