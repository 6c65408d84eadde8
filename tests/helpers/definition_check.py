"""Per-element check of a device result against its mode's definition (oracle/split_precision.py).

A kernel of a split-precision or plain mode computes the definition's products exactly and differs from the definition only
by its fp32 accumulation order and its output rounding.  So, per element,

    |got - defined| <= LAMBDA * sqrt(K) * 2^-24 * mag + r_out * |defined|        (+ 2^-24 * mag for "fp32": product rounding)

with ``mag`` = sum_k |a_k| |b_k| (+ |bias|) of that element, K the number of summed products, r_out the output rounding
(the unit roundoff: 2^-24 fp32, 2^-8 bf16).  LAMBDA = 8 is the probabilistic bound of an fp32 sum (its rms error is well below sqrt(K) u mag).
Unlike a relative-L2 gate over the whole tensor, this does not dilute a fault confined to a tile, a halo row or a channel.

Two more checks on the same data.  Per 16 x 16-pixel block and per output channel, the error's L2 norm relative to the L2
norm of the bound (rho, scale-free) must stay within BLOCK_FACTOR times the same figure of the whole tensor (at least
RHO_FLOOR): the accumulation order is the same in every tile, so a block or a channel that departs from the rest is a fault
even when each of its elements stays under its bound (a truncated split moves a channel ~30x above the fp32 noise).  And,
given the kernel's BatchNorm statistics, mean and invstd per channel against the fp64 statistics of ``defined``.

The kernels between the convolutions (BatchNorm forward / backward, ROIAlign, bias gradients: oracle/pointwise_definitions.py)
are not plain sums of products; their bounds (bn_forward_bound, bn_backward_bounds, roi_align_bound, bias_grad_bound below)
count the roundings of an honest fp32 evaluation and are passed as ``bnd``; the same per-element, per-block and per-channel
checks apply (a "block" of a [R, P, P, C] ROIAlign output is one ROI).

Tensors are NHWC [B, H, W, C] (layout="nhwc", the kernels' own), NCHW (layout="nchw") or [rows, C] (layout="rows").
Only tests/ import this module.
"""
import math

import torch

LAMBDA = 8.0
BLOCK = 16
BLOCK_FACTOR = 4.0
RHO_FLOOR = 0.01
U32 = 2.0 ** -24
R_OUT = {"fp32": 2.0 ** -24, "bf16": 2.0 ** -8, "bf16x3": 2.0 ** -16, "f16x3": 2.0 ** -21}   # output rounding (pairs: the split)


def _nhwc(t, layout):
    t = t.detach().double()
    if layout == "nhwc":
        return t
    if layout == "nchw":
        return t.permute(0, 2, 3, 1)
    if layout == "rows":
        return t.reshape(1, t.shape[0], 1, -1)
    if layout == "oihw":                 # weight gradients: [Cout, Cin, kh, kw] -> one "pixel" row per (Cin, kh, kw)
        return t.reshape(t.shape[0], -1).t().reshape(1, -1, 1, t.shape[0])
    raise ValueError(layout)


def _sqrt(K):
    return K.double().sqrt() if torch.is_tensor(K) else math.sqrt(K)


def bound(defined, mag, K, mode, out="fp32"):
    """K: the number of summed products, a scalar or a tensor of the element's shape (broadcastable)."""
    b = LAMBDA * _sqrt(K) * U32 * mag + R_OUT[out] * defined.abs()
    if out == "f16x3":
        b = b + 2.0 ** -25                  # half pairs below 2^-3: an absolute 2^-25
    if mode == "fp32":
        b = b + U32 * mag
    return b


def _block_norms(x, bs):
    """sum of squares per (b, block_y, block_x) [B, ny, nx] and per channel [C] of an NHWC tensor."""
    B, H, W, C = x.shape
    ny, nx = -(-H // bs), -(-W // bs)
    p = torch.zeros(B, ny * bs, nx * bs, C, dtype=x.dtype, device=x.device)
    p[:, :H, :W] = x * x
    per_block = p.view(B, ny, bs, nx, bs, C).sum(dim=(2, 4, 5))
    per_chan = (x * x).sum(dim=(0, 1, 2))
    return per_block, per_chan


def assert_matches_definition(got, defined, mag, K, mode, layout="nhwc", relu=False, out="fp32", label="", stats=None,
                              quiet=False, extra=None, bnd=None, uniform=("block", "channel")):
    """-> the worst ratio |got - defined| / bound over the elements (printed, so that the margin is in the suite log).

    relu: ``got`` is an activated output -- compared as relu(got) against relu(defined).  stats: (mean, invstd, eps) the
    kernel's BatchNorm statistics of this output, checked per channel against the fp64 statistics of ``defined`` (pre-ReLU).
    extra: an absolute allowance added to the bound (same layout), e.g. the fp32 rounding of an affine epilogue.
    K may be a tensor (same layout, broadcastable).  bnd: the complete per-element bound (same layout) of a kernel that is
    not a plain sum of products (bn_forward_bound, roi_align_bound, ... below); mag / K / mode's bound are not used then.
    uniform: which of the two uniformity checks apply; both by default (convolutions, ROIAlign with one ROI as the block,
    ROIAlign's gradient map).  They presume that error / bound is about the same in every block and channel.  BatchNorm's
    channels do not meet that, by construction: ``mag`` = (|y| + |mean|) |invstd gamma| + |beta| overestimates the rounding
    error much more on a channel whose |mean| is many times its spread (y - mean is then nearly exact, yet |y| + |mean| is
    large) than on a centred one, and invstd * gamma is rounded ONCE per channel -- a systematic relative error of up to u on
    the whole channel, none where the product is exact.  An honest fp32 evaluation in the kernel's own order reaches 0.07 -
    0.13 on its worst channel against 0.008 for the tensor (limit 0.04) with every element below 0.27 of its bound.  So the
    BatchNorm checks, and only they, pass ("block",): per element and per block they are held like everything else."""
    g, d, m = _nhwc(got, layout), _nhwc(defined, layout), _nhwc(mag, layout)
    assert g.shape == d.shape == m.shape, (g.shape, d.shape, m.shape)
    d_pre = d
    if relu:
        g, d = torch.relu(g), torch.relu(d)
    if bnd is not None:
        bnd = _nhwc(bnd, layout).expand_as(d)
    else:
        bnd = bound(d_pre, m, _nhwc(K, layout) if torch.is_tensor(K) else K, mode, out)
    if extra is not None:
        bnd = bnd + _nhwc(extra, layout)
    err = (g - d).abs()
    nan = torch.isnan(g)
    ratio = torch.where(nan, torch.full_like(err, float("inf")), err / bnd.clamp_min(1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    eb, bb = _block_norms(torch.where(nan, torch.zeros_like(err), err), BLOCK), _block_norms(bnd, BLOCK)
    blk_ratio = (eb[0] / bb[0].clamp_min(1e-300)).sqrt()
    ch_ratio = (eb[1] / bb[1].clamp_min(1e-300)).sqrt()
    rho = math.sqrt(float(eb[1].sum()) / max(float(bb[1].sum()), 1e-300))
    limit = BLOCK_FACTOR * max(rho, RHO_FLOOR)
    bad = int((ratio > 1.0).sum())
    msg = []
    if bad:
        idx = tuple(int(i) for i in torch.nonzero(ratio == ratio.max())[0])
        msg.append(f"{bad} of {ratio.numel()} elements exceed the bound; worst at (b, y, x, c) = {idx}: got {float(g[idx]):.9g}, "
                   f"defined {float(d[idx]):.9g}, bound {float(bnd[idx]):.3g} (ratio {worst:.3g})")
    wb, wc = float(blk_ratio.max()), float(ch_ratio.max())
    if ("block" in uniform and wb > limit) or ("channel" in uniform and wc > limit) or bad:
        bi = tuple(int(i) for i in torch.nonzero(blk_ratio == blk_ratio.max())[0])
        ci = int(torch.argmax(ch_ratio))
        msg.append(f"worst {BLOCK}x{BLOCK} block (b, by, bx) = {bi}: L2 error / L2 bound {wb:.3g}; worst channel {ci}: {wc:.3g} "
                   f"(whole tensor {rho:.3g}, limit {limit:.3g})")
    if stats is not None:
        msg += _check_stats(stats, d_pre, bnd)
    if not quiet:
        print(f"[definition {label} {mode}] worst error / bound {worst:.3g}; L2 error / L2 bound: tensor {rho:.3g}, "
              f"worst block {wb:.3g}, worst channel {wc:.3g}")
    assert not msg, f"{label} ({mode}): " + "; ".join(msg)
    return worst


def _check_stats(stats, d, bnd):
    """BatchNorm mean / invstd of the kernel against the fp64 statistics of the definition.  The kernel's statistics see its
    own outputs (each within bnd of d) and sum them in fp32 (LAMBDA sqrt(M) u of the magnitudes)."""
    mean_k, invstd_k, eps = stats
    mean_k, invstd_k = mean_k.detach().double().to(d.device), invstd_k.detach().double().to(d.device)
    mu, var, invstd, tol_mu, tol_var, tol_inv = stats_tolerances(d, bnd, eps)
    out = []
    bad_mu = (mean_k - mu).abs() > tol_mu
    bad_inv = (invstd_k - invstd).abs() > tol_inv
    if bad_mu.any():
        c = int(torch.argmax((mean_k - mu).abs() / tol_mu))
        out.append(f"BatchNorm mean of {int(bad_mu.sum())} channels off; channel {c}: {float(mean_k[c]):.9g} vs {float(mu[c]):.9g} "
                   f"(tol {float(tol_mu[c]):.3g})")
    if bad_inv.any():
        c = int(torch.argmax((invstd_k - invstd).abs() / tol_inv))
        out.append(f"BatchNorm invstd of {int(bad_inv.sum())} channels off; channel {c}: {float(invstd_k[c]):.9g} vs "
                   f"{float(invstd[c]):.9g} (tol {float(tol_inv[c]):.3g})")
    return out


def stats_tolerances(d, bnd, eps):
    """fp64 mean / biased variance / invstd per channel of ``d`` [..., C] and what a kernel's fp32 statistics of outputs within
    ``bnd`` of d may differ from them by (see _check_stats) -> (mu, var, invstd, tol_mu, tol_var, tol_inv)."""
    v = d.reshape(-1, d.shape[-1])
    e = bnd.reshape(-1, d.shape[-1])
    M = v.shape[0]
    mu = v.mean(0)
    dev = v - mu
    var = (dev * dev).mean(0)
    invstd = torch.rsqrt(var + eps)
    sum_err = LAMBDA * math.sqrt(M) * U32
    tol_mu = e.mean(0) + sum_err * v.abs().mean(0) + U32 * mu.abs()
    tol_var = 2 * (dev.abs() * e).mean(0) + (e * e).mean(0) + tol_mu * tol_mu + sum_err * var + 4 * U32 * var
    tol_inv = invstd * (0.5 * tol_var / (var + eps) + 8 * U32)
    return mu, var, invstd, tol_mu, tol_var, tol_inv


# ---- the kernels between the convolutions (oracle/pointwise_definitions.py) ----------------------------------------------
# Every bound below counts roundings of an honest fp32 evaluation; none is fitted to a kernel.
def _r_out(defined, out):
    b = R_OUT[out] * defined.abs()
    return b + 2.0 ** -25 if out == "f16x3" else b          # half pairs below 2^-3: an absolute 2^-25 (as in bound())


def bn_forward_bound(defined, mag, out="fp32"):
    """BatchNorm affine (+ residual): 5 u mag + r_out |defined| -- one rounding for y - mean, one for invstd * gamma, up to two
    for the multiply-add, one for the residual add.  ReLU and the 2x2 max are 1-Lipschitz (the max in the sup norm of its
    window): for a pooled output pass mag = the window maximum of the magnitudes and defined = the pooled definition."""
    return 5 * U32 * mag + _r_out(defined, out)


def bn_backward_bounds(defn, mag, gamma, invstd, out="fp32"):
    """-> (tol_dbeta [C], tol_dgamma [C], bound of dy [B, H, W, C]) for oracle.pointwise_definitions.bn_backward's result.
        dbeta:  (LAMBDA sqrt(M) + 1) u sum |g|                      an fp32 sum of M terms, stored in fp32
        dgamma: (LAMBDA sqrt(M) + 4) u sum |g| |xhat|               + the roundings of xhat (2) and of the product
        dy:     |gamma invstd| (6 u (|g| + |dbeta| / M + |xhat| |dgamma| / M) + tol_dbeta / M + |xhat| tol_dgamma / M)
                + r_out |dy|                                         the kernel applies ITS dbeta / dgamma"""
    M = defn.M
    tol_db = (LAMBDA * math.sqrt(M) + 1) * U32 * mag.dbeta
    tol_dg = (LAMBDA * math.sqrt(M) + 4) * U32 * mag.dgamma
    gi = (gamma.detach().double() * invstd.detach().double()).abs()
    inner = 6 * U32 * (defn.g.abs() + defn.dbeta.abs() / M + mag.xhat * defn.dgamma.abs() / M) + tol_db / M + mag.xhat * tol_dg / M
    return tol_db, tol_dg, gi * inner + _r_out(defn.dy, out)


def roi_align_bound(defined, mag, aux, out="fp32"):
    """(LAMBDA sqrt(K) + grid_h + grid_w + 4) u mag + coord + r_out |defined|.  K = the number of feature pixels (forward) or
    (ROI, bin) pairs (backward) summed; grid_h + grid_w + 4: the fp32 sums that build Ay / Ax, their product, 1 / count and the
    scaling; coord: the kernel's sample coordinates may differ from the definition's (fp32, torchvision's written order, no
    contraction) by eps_c = 4 u (|coordinate| + 1), e.g. by a contracted multiply-add -- bilinear interpolation is continuous and
    piecewise linear, so a sample moves by at most (eps_y + eps_x) (|f11| + |f12| + |f21| + |f22|); summed over the bin's
    samples and divided by count (oracle.pointwise_definitions.roi_align_forward / _backward compute it)."""
    return (LAMBDA * _sqrt(aux.K) + aux.gsum + 4) * U32 * mag + aux.coord + _r_out(defined, out)


def bias_grad_bound(mag, M, db_before=None):
    """per column: LAMBDA sqrt(M) u sum |dy| (+ u |db_before| when accumulating: one more fp32 add)."""
    b = LAMBDA * math.sqrt(M) * U32 * mag
    return b if db_before is None else b + U32 * db_before.detach().double().abs()


def assert_channels_within(got, defined, tol, label=""):
    """per-channel vectors (dgamma, dbeta, bias gradients, running statistics): |got - defined| <= tol, every channel.
    -> the worst ratio (printed)."""
    g, d, t = got.detach().double().flatten(), defined.detach().double().flatten(), tol.detach().double().flatten()
    d, t = d.to(g.device), t.to(g.device)
    assert g.shape == d.shape == t.shape, (g.shape, d.shape, t.shape)
    err = (g - d).abs()
    ratio = torch.where(torch.isnan(g), torch.full_like(err, float("inf")), err / t.clamp_min(1e-300))
    ratio = torch.where((err == 0) & ~torch.isnan(g), torch.zeros_like(ratio), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"[definition {label}] worst channel error / bound {worst:.3g}")
    bad = ratio > 1.0
    if bad.any():
        c = int(torch.argmax(ratio))
        raise AssertionError(f"{label}: {int(bad.sum())} of {ratio.numel()} channels exceed the bound; worst channel {c}: got "
                             f"{float(g[c]):.9g}, defined {float(d[c]):.9g}, bound {float(t[c]):.3g} (ratio {worst:.3g})")
    return worst


def expected_patch_kernel(wg, cin_phys, split, out=None, red=False):
    """The kernel the halo-patch forward runs for a forced variant wg = 1..9 (include/sfod_hip.h sfod_set_conv3x3_variant):
    cin_phys the physical 16-bit channel count (2 x logical for operand pairs), split 0 plain operands, 1 bf16 pairs, 2 half
    pairs; out the output type ("float" / "bf16_t", default: float for pairs, bf16_t otherwise).  Where the variant cannot
    take the shape, the documented other kernel (compare with expected_patch_kernel(wg, 64, split) to tell).  red: the form
    with the BatchNorm-backward epilogue (sfod_conv_dgrad_bnred)."""
    c64 = cin_phys % 64 == 0
    if split and c64 and wg in (5, 6, 7, 8, 9):
        nw, nip, nwn = {5: (8, 4, 2), 6: (4, 8, 2), 7: (4, 4, 1), 8: (8, 4, 1), 9: (8, 2, 1)}[wg]
        return f"k_conv3x3_m16<{nw},{nip},{split},{int(red)},0,{nwn}>"
    shape = {1: 1, 2: 2, 3: 3, 4: 4, 5: 2, 6: 2, 7: 3, 8: 4, 9: 3}[wg]
    if split and wg in (7, 9):
        shape = 2                           # pairs without physical Cin % 64: the 32x32x16 kernel of shape 2 / 1
    if split and wg == 8:
        shape = 1
    if shape in (3, 4) and not c64:
        shape = 2 if shape == 3 else 1
    g, fm = {1: (1, 4), 2: (1, 2), 3: (2, 1), 4: (2, 2)}[shape]
    out = out or ("float" if split else "bf16_t")
    return f"k_conv3x3_patch<{g},{fm},{out},{split},{int(red)}>"


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()
