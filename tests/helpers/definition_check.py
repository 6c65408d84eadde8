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


def bound(defined, mag, K, mode, out="fp32"):
    b = LAMBDA * math.sqrt(K) * U32 * mag + R_OUT[out] * defined.abs()
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
                              quiet=False, extra=None):
    """-> the worst ratio |got - defined| / bound over the elements (printed, so that the margin is in the suite log).

    relu: ``got`` is an activated output -- compared as relu(got) against relu(defined).  stats: (mean, invstd, eps) the
    kernel's BatchNorm statistics of this output, checked per channel against the fp64 statistics of ``defined`` (pre-ReLU).
    extra: an absolute allowance added to the bound (same layout), e.g. the fp32 rounding of an affine epilogue."""
    g, d, m = _nhwc(got, layout), _nhwc(defined, layout), _nhwc(mag, layout)
    assert g.shape == d.shape == m.shape, (g.shape, d.shape, m.shape)
    d_pre = d
    if relu:
        g, d = torch.relu(g), torch.relu(d)
    bnd = bound(d_pre, m, K, mode, out)
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
    if wb > limit or wc > limit or bad:
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
