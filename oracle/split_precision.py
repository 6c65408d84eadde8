"""Oracle (test infrastructure): CPU restatement of the split-precision product the MFMA kernels compute
(include/sfod_hip.h, SFOD_BF16X3 / SFOD_F16X3) -- NOT of anything in the reference, whose arithmetic is plain fp32: this
pins what the device modes are DEFINED to compute, so that a kernel is checked against its own definition (agreement at
the level of the fp32 accumulation order, ~1e-7) as well as against the exact product (tests/test_gpu_bf16x3.py,
tests/test_gpu_f16x3.py).  Only tests/ may import this module.

    operand v  ->  hi = rnd16(v), lo = rnd16(v - hi)            rnd16 = bfloat16 or IEEE half (round to nearest even)
    product    ->  hi_a * hi_b + hi_a * lo_b + lo_a * hi_b      (lo_a * lo_b dropped), summed over K in high precision here
    f16x3 weights: stored as w * s, s = the power of two with max|w| * s in [2^13, 2^14); the result is multiplied by 1 / s
"""
import math

import torch


def split_pairs(v, fmt):
    """fp32 tensor -> (hi, lo) as fp64 tensors holding the exactly representable 16-bit values."""
    v = v.float()
    if fmt == "bf16":
        hi = v.bfloat16().float()
        lo = (v - hi).bfloat16().float()
    elif fmt == "f16":
        c = v.clamp(-65504.0, 65504.0)          # beyond half's range (infinities too): exactly +-65504, lo = 0; NaN stays NaN
        hi = c.half().float()
        lo = (c - hi).half().float()
    else:
        raise ValueError(fmt)
    return hi.double(), lo.double()


def weight_scale(w):
    """the per-tensor power of two of the SFOD_F16X3 weight packers (csrc/common.h wscale_from_absmax)."""
    amax = float(w.abs().max())
    if amax == 0.0 or not math.isfinite(amax):
        return 1.0
    return 2.0 ** (13 - math.floor(math.log2(amax)))


def linear(x, w, fmt):
    """x [M, K], w [N, K] fp32 -> x @ w.T as the split-precision modes define it (fp64 accumulation)."""
    s = weight_scale(w) if fmt == "f16" else 1.0
    xh, xl = split_pairs(x, fmt)
    wh, wl = split_pairs(w.float() * s, fmt)
    return (xh @ wh.t() + xh @ wl.t() + xl @ wh.t()) / s


# ---- every compute mode, for any product -----------------------------------------------------------------------------
# mode: "bf16x3" / "f16x3" (the pair modes above), "bf16" (exact products of the bf16-rounded operands) or "fp32" (exact
# products of the fp32 operands).  A mode's result is sum over its terms of op(a, b) / s, op a bilinear fp64 product.
MODES = ("bf16x3", "f16x3", "bf16", "fp32")
PAIR_FORMAT = {"bf16x3": "bf16", "f16x3": "f16"}


def terms(a, b, mode, scale_b=False):
    """-> ([(a_i, b_i) fp64], s): the operand pairs whose products the mode sums, and the power of two b was stored under
    (scale_b: b is a forward weight of the f16x3 mode, packed as w * weight_scale(w))."""
    if mode in PAIR_FORMAT:
        fmt = PAIR_FORMAT[mode]
        s = weight_scale(b) if (scale_b and fmt == "f16") else 1.0
        ah, al = split_pairs(a, fmt)
        bh, bl = split_pairs(b.float() * s, fmt)
        return [(ah, bh), (ah, bl), (al, bh)], s
    if mode == "bf16":
        return [(a.float().bfloat16().double(), b.float().bfloat16().double())], 1.0
    if mode == "fp32":
        return [(a.float().double(), b.float().double())], 1.0
    raise ValueError(mode)


def conv2d(x, w, mode, padding=1, stride=1, bias=None):
    """x [B, Cin, H, W], w [Cout, Cin, kh, kw] fp32 -> the convolution as ``mode`` defines it (fp64; f16x3 weights under
    their power-of-two scale, as the packers store them).  ``bias`` is added exactly."""
    ts, s = terms(x, w, mode, scale_b=True)
    y = sum(torch.nn.functional.conv2d(a, b, None, stride=stride, padding=padding) for a, b in ts) / s
    return y if bias is None else y + bias.double().view(1, -1, 1, 1)


def conv2d_wgrad(x, dy, w_shape, mode, padding=1, stride=1):
    """d/dw of sum(conv2d(x, w) * dy) as ``mode`` defines it: x [B, Cin, H, W], dy [B, Cout, Ho, Wo] -> [Cout, Cin, kh, kw].
    The backward products of "f16x3" take bf16 pairs (gradients do not fit half's range, include/sfod_hip.h)."""
    mode = "bf16x3" if mode == "f16x3" else mode
    ts, _ = terms(x, dy, mode)
    return sum(torch.nn.grad.conv2d_weight(a, w_shape, b, stride=stride, padding=padding) for a, b in ts)


def rot180(w):
    """OIHW weights -> the weights of the data gradient (in / out swapped, taps flipped): conv2d(dy, rot180(w)) = dx."""
    return w.flip(2, 3).transpose(0, 1).contiguous()


def magnitude(x, w, padding=1, stride=1, bias=None):
    """sum_k |x_k| |w_k| per output of the convolution (+ |bias|): the scale of the fp32 accumulation error."""
    m = torch.nn.functional.conv2d(x.double().abs(), w.double().abs(), None, stride=stride, padding=padding)
    return m if bias is None else m + bias.double().abs().view(1, -1, 1, 1)


def magnitude_wgrad(x, dy, w_shape, padding=1, stride=1):
    return torch.nn.grad.conv2d_weight(x.double().abs(), w_shape, dy.double().abs(), stride=stride, padding=padding)


def magnitude_linear(x, w, bias=None):
    m = x.double().abs() @ w.double().abs().t()
    return m if bias is None else m + bias.double().abs()


def linear_mode(x, w, mode, bias=None):
    """linear() for every mode: x [M, K], w [N, K] -> x @ w.T (+ bias)."""
    ts, s = terms(x, w, mode, scale_b=True)
    y = sum(a @ b.t() for a, b in ts) / s
    return y if bias is None else y + bias.double()
