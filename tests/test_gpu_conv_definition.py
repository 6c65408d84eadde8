"""The convolution kernels against their mode's DEFINITION, per element (tests/helpers/definition_check.py).

oracle/split_precision.py defines what each mode computes (bf16x3 / f16x3: hi*hi + hi*lo + lo*hi of the rounded pairs, f16x3
weights under their power-of-two scale; bf16: exact products of bf16 operands; fp32: exact products).  A kernel may differ
from that only by its fp32 accumulation order and its output rounding, so every element is held to
LAMBDA * sqrt(K) * 2^-24 * sum|a||b| (+ output rounding), and every 16 x 16-pixel block and channel to the level of the
whole tensor -- a fault confined to one tile, halo row or channel fails here at any tensor size.  The definitions are
computed on the device in fp64 with torch's own ops (unfold + matmul), never with the project's kernels.  Every case that
forces a workgroup shape, tile or pipe asserts that the kernel it names ran (native.last_conv_kernel).

Default selection: the planner's choice per kernel x mode + one full-chip case per form; forced variants / tiles / pipes are
``sweep``.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import definition_check as dc
from oracle import split_precision as sp

pytestmark = pytest.mark.gpu
DEV = "cuda"
SW = pytest.mark.sweep
PAIR = {"bf16x3": "SPLIT_DTYPE", "f16x3": "SPLITH_DTYPE"}
DT = {"bf16x3": "BF16X3", "f16x3": "F16X3", "bf16": "BF16", "fp32": "F32"}


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _unfold_mm(x, w2d, k, padding, stride, chunk):
    """fp64 conv of NCHW x with w2d [Cout, Cin*k*k] by unfold + matmul, a few images at a time -> NHWC."""
    outs = []
    for b0 in range(0, x.shape[0], chunk):
        xb = x[b0:b0 + chunk]
        cols = F.unfold(xb, k, padding=padding, stride=stride)                     # [b, Cin*k*k, L]
        Ho = (x.shape[2] + 2 * padding - k) // stride + 1
        Wo = (x.shape[3] + 2 * padding - k) // stride + 1
        outs.append((w2d @ cols).view(xb.shape[0], -1, Ho, Wo).permute(0, 2, 3, 1))
    return torch.cat(outs)


def conv_def(x, w, mode, padding=1, stride=1, bias=None, chunk=1):
    """(defined, magnitude) NHWC fp64 on the device: sp.conv2d / sp.magnitude computed by unfold + matmul."""
    k = w.shape[-1]
    ts, s = sp.terms(x, w, mode, scale_b=True)
    y = sum(_unfold_mm(a, b.reshape(b.shape[0], -1), k, padding, stride, chunk) for a, b in ts) / s
    mag = _unfold_mm(x.double().abs(), w.double().abs().reshape(w.shape[0], -1), k, padding, stride, chunk)
    if bias is not None:
        y, mag = y + bias.double(), mag + bias.double().abs()
    return y, mag


def wgrad_def(x, dy, k, mode, padding=1):
    """(defined, magnitude) OIHW fp64 of the weight gradient: sum over images of dy_b [Cout, L] @ cols_b [L, Cin*k*k]."""
    mode = "bf16x3" if mode == "f16x3" else mode
    ts, _ = sp.terms(x, dy, mode)
    Cout, Cin = dy.shape[1], x.shape[1]
    acc = torch.zeros(Cout, Cin * k * k, dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(acc)
    for b in range(x.shape[0]):
        for a, d in ts:
            acc += d[b].reshape(Cout, -1) @ F.unfold(a[b:b + 1], k, padding=padding)[0].t()
        mag += dy[b].double().abs().reshape(Cout, -1) @ F.unfold(x[b:b + 1].double().abs(), k, padding=padding)[0].t()
    return acc.view(Cout, Cin, k, k), mag.view(Cout, Cin, k, k)


def operand(native, x_nhwc, mode):
    if mode in PAIR:
        return native.cast(x_nhwc.contiguous(), getattr(native, PAIR[mode]))
    return x_nhwc.contiguous().bfloat16() if mode == "bf16" else x_nhwc.contiguous().float()


def ran(native, expected, label):
    got = native.last_conv_kernel()
    assert got == expected, f"{label}: expected {expected} to run, ran {got}"


# ---- halo-patch forward --------------------------------------------------------------------------------------------
PATCH_SHAPES = [
    (2, 37, 75, 64, 128),       # tiles overhanging the map in x and y
    (2, 9, 13, 32, 200),        # Cout tail, a map smaller than one tile, one 64-physical-channel body: every variant's kernel
    (1, 33, 40, 64, 136),       # Cout tail (a partial 64-channel tile of the 16x16x32 kernels), tile overhang
    (2, 9, 13, 16, 200),        # one 32-physical-channel slice: only the 32x32x16 shapes 1 / 2 (variants 3-9 skip)
    (1, 33, 40, 48, 136),       # 96 physical channels (not a multiple of 64): likewise
]
LDY_PAD = 3                     # the "ldy" form: a row pitch that is not a multiple of 4 (the kernels' scalar store path)


def _patch_cases():
    out = []
    for mode in ("bf16x3", "f16x3"):
        for shape in PATCH_SHAPES:
            for form in ("plain", "relu_stats", "ldy"):
                for wg in range(10):
                    marks = [SW] if wg else []
                    out.append(pytest.param(mode, shape, form, wg, marks=marks, id=f"{mode}-{'x'.join(map(str, shape))}-{form}-{wg}"))
    for shape in ((2, 37, 75, 64, 128), (1, 33, 40, 64, 136)):      # plain bf16 operands: Cin % 32 (no pairs)
        for wg in range(5):
            out.append(pytest.param("bf16", shape, "plain", wg, marks=[SW] if wg else [],
                                    id=f"bf16-{'x'.join(map(str, shape))}-plain-{wg}"))
    return out


@pytest.mark.parametrize("mode,shape,form,wg", _patch_cases())
def test_patch_forward_matches_its_definition(native, mode, shape, form, wg):
    B, H, W, Cin, Cout = shape
    g = torch.Generator(device=DEV).manual_seed(sum(shape) + wg)
    x = torch.randn(B, Cin, H, W, device=DEV, generator=g) + 0.3
    w = torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g) / math.sqrt(Cin * 9)
    bias = torch.randn(Cout, device=DEV, generator=g)
    xd = operand(native, nhwc(x), mode)
    wp = native.pack_conv_weight(w, Cin, getattr(native, DT[mode]))
    split = {"bf16x3": 1, "f16x3": 2, "bf16": 0}[mode]
    cin_phys = Cin * (2 if split else 1)
    if wg and dc.expected_patch_kernel(wg, cin_phys, split) != dc.expected_patch_kernel(wg, 64, split):
        pytest.skip(f"variant {wg} needs physical Cin % 64 == 0 (here {cin_phys}): this shape runs "
                    f"{dc.expected_patch_kernel(wg, cin_phys, split)}, covered by the planner's and the shape's own cases")
    try:
        native.set_conv_algo(2)
        native.set_conv3x3_variant(wg)
        assert native.query("sfod_conv_fwd_algo", B, H, W, Cin, Cout, 3, getattr(native, DT[mode])) == 2
        if form == "plain":
            y = native.conv_fwd(xd, wp, bias, Cout, 3)
        elif form == "relu_stats":
            y, stats = native.conv_fwd(xd, wp, bias, Cout, 3, act=1, want_stats=True)
        else:
            y = native.conv_fwd(xd, wp, None, Cout, 3, ldy=Cout + LDY_PAD)
        kern = native.last_conv_kernel()
        if wg:
            ran(native, dc.expected_patch_kernel(wg, cin_phys, split), f"variant {wg}")
        if form == "relu_stats":
            mean, invstd = native.bn_finalize(stats, B * H * W, Cout, torch.zeros(Cout, device=DEV),
                                              torch.ones(Cout, device=DEV), 0.1, 1e-5)
    finally:
        native.set_conv_algo(0)
        native.set_conv3x3_variant(0)
    defined, mag = conv_def(x, w, mode, bias=None if form == "ldy" else bias)
    K = Cin * 9
    out = "bf16" if y.dtype == torch.bfloat16 else "fp32"
    label = f"patch {form} {shape} wg {wg} ({kern})"
    if form == "ldy":
        assert (y[..., Cout:] == 0).all()
        y = y[..., :Cout]
    dc.assert_matches_definition(y, defined, mag, K, mode, relu=form == "relu_stats", out=out, label=label,
                                 stats=(mean, invstd, 1e-5) if form == "relu_stats" else None)


@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
def test_patch_forward_layer_size_channel_tail_matches_its_definition(native, mode):
    """The planner's own choice at layer size with a Cout tail and a row pitch that is not a multiple of 4: the 16x16x32
    kernel's scalar store path (partial 64-channel tile, unaligned rows) with ReLU and BatchNorm statistics."""
    B, H, W, Cin, Cout = 8, 75, 150, 64, 200
    g = torch.Generator(device=DEV).manual_seed(31)
    x = torch.randn(B, Cin, H, W, device=DEV, generator=g) + 0.3
    w = torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g) / math.sqrt(Cin * 9)
    bias = torch.randn(Cout, device=DEV, generator=g)
    split = 2 if mode == "f16x3" else 1
    y, st = native.conv_fwd(operand(native, nhwc(x), mode), native.pack_conv_weight(w, Cin, getattr(native, DT[mode])), bias,
                            Cout, 3, act=1, ldy=Cout + LDY_PAD, want_stats=True)
    ran(native, f"k_conv3x3_m16<8,4,{split},0,0,2>", "planner's choice")
    mean, invstd = native.bn_finalize(st, B * H * W, Cout, torch.zeros(Cout, device=DEV), torch.ones(Cout, device=DEV), 0.1, 1e-5)
    assert (y[..., Cout:] == 0).all()
    defined, mag = conv_def(x, w, mode, bias=bias)
    dc.assert_matches_definition(y[..., :Cout], defined, mag, Cin * 9, mode, relu=True, label="layer-size channel tail",
                                 stats=(mean, invstd, 1e-5))


# ---- data gradient (rot180 weights) and its fused BatchNorm-backward reduction -------------------------------------------
@pytest.mark.parametrize("shape,wg", [((2, 37, 75, 64, 128), 0), ((1, 40, 64, 128, 64), 0)] +
                         [pytest.param((2, 18, 25, 256, 256), v, marks=SW) for v in (1, 2, 4, 5, 6, 7, 8, 9)])
def test_dgrad_and_its_batchnorm_reduction_match_their_definition(native, shape, wg):
    B, H, W, Cup, C = shape               # the upper layer maps C -> Cup channels; its data gradient has C channels
    g = torch.Generator(device=DEV).manual_seed(B * H + W + C + wg)
    dy = torch.randn(B, Cup, H, W, device=DEV, generator=g) * 1e-3
    w = torch.randn(Cup, C, 3, 3, device=DEV, generator=g) / math.sqrt(9 * C)
    y = torch.randn(B, H, W, C, device=DEV, generator=g) * 2 + 0.3
    gamma, beta = torch.rand(C, device=DEV, generator=g) + 0.5, torch.randn(C, device=DEV, generator=g) * 0.3
    mean = y.mean(dim=(0, 1, 2))
    invstd = torch.rsqrt(y.var(dim=(0, 1, 2), unbiased=False) + 1e-5)
    dys = native.cast(nhwc(dy), native.SPLIT_DTYPE)
    wr = native.pack_conv_weight(w, Cup, native.BF16X3, rot180=True)
    try:
        native.set_conv_algo(2)              # the halo-patch kernel wherever the shape allows it (small maps: auto may not)
        native.set_conv3x3_variant(wg)
        served = native.query("sfod_conv_dgrad_bnred_blocks", B, H, W, Cup, C, native.BF16X3) > 0
        assert served or wg
        dz_plain = native.conv_fwd(dys, wr, None, C, 3)
        kern = native.last_conv_kernel()
        if wg:
            ran(native, dc.expected_patch_kernel(wg, 2 * Cup, 1), f"dgrad variant {wg}")
        fused = native.conv_dgrad_bnred(dys, wr, C, y, mean, invstd, gamma, beta)
        kern_red = native.last_conv_kernel()
        if wg and fused is not None:
            ran(native, dc.expected_patch_kernel(wg, 2 * Cup, 1, red=True), f"dgrad_bnred variant {wg}")
    finally:
        native.set_conv_algo(0)
        native.set_conv3x3_variant(0)
    defined, mag = conv_def(dy, sp.rot180(w), "bf16x3")
    dc.assert_matches_definition(dz_plain, defined, mag, Cup * 9, "bf16x3", label=f"dgrad {shape} wg {wg} ({kern})")
    if not served:                        # a forced shape without the epilogue: refused, never silently mis-served
        assert fused is None
        return
    dz, ws = fused
    dc.assert_matches_definition(dz, defined, mag, Cup * 9, "bf16x3", label=f"dgrad_bnred {shape} wg {wg} ({kern_red})")
    # the partial rows: sum over pixels of (dz, dz * xhat) where relu(bn(y)) > 0, against fp64 on the defined dz
    nblk = ws.shape[0] - native.BN_BWD_SCRATCH_ROWS
    part = ws[:nblk].double().sum(0)
    xhat = (y.double() - mean.double()) * invstd.double()
    pre = xhat * gamma.double() + beta.double()
    live = (pre > 0).double()
    near = (pre.abs() < 1e-5).double()              # the kernel's fp32 mask may differ from fp64 only here
    M = B * H * W
    db = (defined * live).sum(dim=(0, 1, 2))
    dg = (defined * live * xhat).sum(dim=(0, 1, 2))
    bnd = dc.bound(defined, mag, Cup * 9, "bf16x3")
    s32 = dc.LAMBDA * math.sqrt(M) * dc.U32
    tol_b = (bnd * live).sum(dim=(0, 1, 2)) + s32 * (defined.abs() * live).sum(dim=(0, 1, 2)) + (defined.abs() * near).sum(dim=(0, 1, 2))
    tol_g = ((bnd + 4 * dc.U32 * defined.abs()) * live * xhat.abs()).sum(dim=(0, 1, 2)) + \
        s32 * (defined.abs() * live * xhat.abs()).sum(dim=(0, 1, 2)) + (defined.abs() * near * xhat.abs()).sum(dim=(0, 1, 2))
    rb, rg = ((part[:C] - db).abs() / tol_b).max().item(), ((part[C:] - dg).abs() / tol_g).max().item()
    print(f"[definition dgrad_bnred partial rows {shape} wg {wg}] worst error / bound: dbeta {rb:.3g}, dgamma {rg:.3g}")
    assert rb <= 1 and rg <= 1, (rb, rg)


# ---- BatchNorm folded into the convolution's input --------------------------------------------------------------------
def test_bnin_matches_its_definition(native):
    B, H, W, Cin, Cout = 4, 150, 300, 256, 256
    g = torch.Generator(device=DEV).manual_seed(9)
    y_pre = torch.randn(B, H, W, Cin, device=DEV, generator=g) * 1.7 + 0.4
    gamma = torch.rand(Cin, device=DEV, generator=g) + 0.5
    beta = torch.rand(Cin, device=DEV, generator=g) + 0.2
    mean = y_pre.mean(dim=(0, 1, 2))
    invstd = torch.rsqrt(y_pre.var(dim=(0, 1, 2), unbiased=False) + 1e-5)
    w = torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g) / (3 * Cin ** 0.5)
    bias = torch.randn(Cout, device=DEV, generator=g)
    wp = native.pack_conv_weight(w, Cin, native.BF16X3)
    assert native.conv_fwd_bnin_supported(y_pre, wp, Cout)
    y = native.conv_fwd_bnin(y_pre, mean, invstd, gamma, beta, wp, bias, Cout)
    ran(native, "k_conv3x3_m16<4,8,1,0,1,2>", "bnin")
    # the operand: relu(bn(y_pre)) in fp32 (the kernel's rounding of the affine may differ by an ulp: 2^-24 |a| per operand,
    # inside the bound's 2^-24 sqrt(K) LAMBDA)
    z = torch.relu((y_pre - mean) * (invstd * gamma) + beta).permute(0, 3, 1, 2)
    defined, mag = conv_def(z, w, "bf16x3", bias=bias)
    dc.assert_matches_definition(y, defined, mag, Cin * 9, "bf16x3", label="bnin 4x150x300 256->256", extra=2 * dc.U32 * mag)


# ---- halo-patch weight gradient ------------------------------------------------------------------------------------------
WG_SHAPES = [(2, 37, 75, 64, 128), (1, 20, 50, 32, 32), (2, 30, 44, 72, 136)]


@pytest.mark.parametrize("pipe", [2, pytest.param(1, marks=SW), pytest.param(0, marks=SW)])
@pytest.mark.parametrize("shape", WG_SHAPES)
def test_patch_wgrad_matches_its_definition(native, shape, pipe):
    B, H, W, Cin, Cout = shape
    g = torch.Generator(device=DEV).manual_seed(sum(shape) + pipe)
    x = torch.randn(B, Cin, H, W, device=DEV, generator=g)
    dy = torch.randn(B, Cout, H, W, device=DEV, generator=g) * 1e-4
    xd, dyd = native.cast(nhwc(x), native.SPLIT_DTYPE), native.cast(nhwc(dy), native.SPLIT_DTYPE)
    try:
        native.set_conv_algo(2)
        native.set_wgrad3x3_pipe(pipe)
        dwp = native.conv_wgrad(xd, dyd, Cout, 3)
        kern = native.last_conv_kernel()
        expect = {2: "k_wgrad3x3_w64" if Cin >= 64 else "k_wgrad3x3_patch<4,1,1>", 1: "k_wgrad3x3_patch<4,1,1>",
                  0: "k_wgrad3x3_patch<4,1,0>"}[pipe]
        ran(native, expect, f"wgrad pipe {pipe}")
        direct = torch.full((Cout, Cin, 3, 3), float("nan"), device=DEV)
        native.conv_wgrad_oihw(xd, dyd, direct, accumulate=False)
        ran(native, expect, f"wgrad_oihw pipe {pipe}")
    finally:
        native.set_conv_algo(0)
        native.set_wgrad3x3_pipe(2)
    dw = torch.empty(Cout, Cin, 3, 3, device=DEV)
    native.unpack_conv_wgrad(dwp, dw)
    defined, mag = wgrad_def(x, dy, 3, "bf16x3")
    K = B * H * W
    dc.assert_matches_definition(dw, defined, mag, K, "bf16x3", layout="oihw", label=f"wgrad {shape} pipe {pipe} ({kern})")
    dc.assert_matches_definition(direct, defined, mag, K, "bf16x3", layout="oihw", label=f"wgrad_oihw {shape} pipe {pipe}")


@pytest.mark.parametrize("mode", ["bf16x3", "fp32"])
@pytest.mark.parametrize("shape", [(2, 17, 23, 128, 512, 1), (1, 300, 1, 1000, 200, 1), (3, 16, 16, 8, 64, 3)])
def test_generic_wgrad_matches_its_definition(native, shape, mode):
    """The generic weight-gradient kernels: 1x1 convolutions / linear layers (64 x 64 and the wide 128 x 256 tile) and the
    first layer (3 channels in one 8-channel group), K = B * H * W."""
    B, H, W, Cin, Cout, k = shape
    g = torch.Generator(device=DEV).manual_seed(B + H + Cin + Cout)
    x = torch.randn(B, Cin, H, W, device=DEV, generator=g)
    if Cin == 8:
        x[:, 3:] = 0
    dy = torch.randn(B, Cout, H, W, device=DEV, generator=g) * 1e-3
    xd, dyd = operand(native, nhwc(x), mode), operand(native, nhwc(dy), mode)
    dwp = native.conv_wgrad(xd, dyd, Cout, k)
    kern = native.last_conv_kernel()
    assert kern.startswith("k_conv_wgrad") or kern.startswith("k_wgrad3x3"), kern
    dw = torch.empty(Cout, Cin, k, k, device=DEV)
    native.unpack_conv_wgrad(dwp.contiguous(), dw)
    defined, mag = wgrad_def(x, dy, k, mode, padding=k // 2)
    dc.assert_matches_definition(dw, defined, mag, B * H * W, mode, layout="oihw", label=f"generic wgrad {shape} ({kern})")


# ---- ResNet stem and the first VGG layer -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("hw", [(67, 93), (16, 9)])
def test_stem7x7_matches_its_definition(native, mode, hw):
    H, W = hw
    B = 2
    g = torch.Generator(device=DEV).manual_seed(H * W)
    x = torch.zeros(B, H, W, 4, device=DEV)
    x[..., :3] = torch.randn(B, H, W, 3, device=DEV, generator=g) * 40
    w = torch.randn(64, 3, 7, 7, device=DEV, generator=g) / 12
    bias = torch.randn(64, device=DEV, generator=g)
    wm = torch.zeros(64, 160, device=DEV)
    wm[:, :147] = w.permute(0, 2, 3, 1).reshape(64, 147)             # k = (ky * 7 + kx) * 3 + c
    wp = native.pack_fc_weight(wm, getattr(native, DT[mode]))
    assert native.stem7x7_supported(x, getattr(native, DT[mode]))
    y = native.stem7x7(x, wp, bias, act=0)
    ran(native, "k_stem7x7<2>" if mode == "f16x3" else "k_stem7x7<1>", "stem")
    yr = native.stem7x7(x, wp, bias, act=1)
    defined, mag = conv_def(x.permute(0, 3, 1, 2)[:, :3], w, mode, padding=3, stride=2, bias=bias)
    dc.assert_matches_definition(y, defined, mag, 147, mode, label=f"stem7x7 {hw}")
    dc.assert_matches_definition(yr, defined, mag, 147, mode, relu=True, label=f"stem7x7 relu {hw}")


@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("hw", [(50, 70), (9, 500)])
def test_conv_first_matches_its_definition(native, mode, hw):
    H, W = hw
    B, Cout = 2, 64
    g = torch.Generator(device=DEV).manual_seed(H + W)
    x = torch.zeros(B, H, W, 8, device=DEV)
    x[..., :3] = torch.randn(B, H, W, 3, device=DEV, generator=g) * 50
    w = torch.randn(Cout, 3, 3, 3, device=DEV, generator=g) / 5
    bias = torch.randn(Cout, device=DEV, generator=g)
    xd = operand(native, x, mode)
    wp = native.pack_conv_weight(w, 8, getattr(native, DT[mode]))
    assert native.query("sfod_conv_fwd_algo", B, H, W, 8, Cout, 3, getattr(native, DT[mode])) == 3
    y, st = native.conv_fwd(xd, wp, bias, Cout, 3, want_stats=True)
    split = 2 if mode == "f16x3" else 1
    ran(native, f"k_conv_first_x3<{split}>", "conv_first")
    st2 = native.conv_first_stats(xd, wp, bias)
    mean, invstd = native.bn_finalize(st2, B * H * W, Cout, torch.zeros(Cout, device=DEV), torch.ones(Cout, device=DEV),
                                      0.1, 1e-5)
    defined, mag = conv_def(x.permute(0, 3, 1, 2)[:, :3], w, mode, bias=bias)
    dc.assert_matches_definition(y, defined, mag, 27, mode, label=f"conv_first {hw}", stats=(mean, invstd, 1e-5))
    gamma, beta = torch.rand(Cout, device=DEV, generator=g) + 0.5, torch.randn(Cout, device=DEV, generator=g) * 0.2
    scale = gamma * invstd
    shift = beta - mean * scale
    z = native.conv_first_apply(xd, wp, bias, scale, shift, relu=True)
    ran(native, f"k_conv_first_x3<{split}>", "conv_first apply")
    sc, sh = scale.double(), shift.double()
    zdef = defined * sc + sh
    extra = 4 * dc.U32 * ((defined * sc).abs() + sh.abs())           # fp32 rounding of the affine epilogue
    dc.assert_matches_definition(native.cast(z, torch.float32), zdef, mag * sc.abs(), 27, mode, relu=True, out=mode,
                                 label=f"conv_first apply {hw}", extra=extra)


# ---- generic implicit GEMM ---------------------------------------------------------------------------------------------------
def _gemm_cases():
    out = []
    for mode in ("bf16x3", "f16x3", "bf16", "fp32"):
        out.append(pytest.param(mode, (22800, 256, 1024), 0, id=f"{mode}-22800x256x1024-0"))
    for mode in ("bf16x3", "f16x3"):
        for shape in ((22800, 256, 1024), (5000, 96, 200), (700, 1024, 256)):
            for tile in (6, 7, 8):
                out.append(pytest.param(mode, shape, tile, marks=SW, id=f"{mode}-{'x'.join(map(str, shape))}-{tile}"))
    return out


@pytest.mark.parametrize("mode,shape,tile", _gemm_cases())
def test_gemm_tiles_match_their_definition(native, mode, shape, tile):
    M, K, N = shape
    g = torch.Generator(device=DEV).manual_seed(M + K + N)
    x = torch.randn(M, K, device=DEV, generator=g)
    w = torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)
    bias = torch.randn(N, device=DEV, generator=g)
    xd = operand(native, x, mode).view(M, 1, 1, K)
    wp = native.pack_fc_weight(w, getattr(native, DT[mode]))
    try:
        native.set_gemm_tile(tile)
        y = native.conv_fwd(xd, wp, bias, N, 1, act=1)
        kern = native.last_conv_kernel()
    finally:
        native.set_gemm_tile(0)
    split = {"bf16x3": 1, "f16x3": 2}.get(mode, 0)
    if tile:
        wn, wr, nst = {6: (2, 4, 3), 7: (2, 2, 3), 8: (2, 4, 4)}[tile]
        ran(native, f"k_conv_fwd<bf16_t,float,2,{wn},1,{wr},{nst},{split},64>", f"tile {tile}")
    defined = sp.linear_mode(x, w, mode, bias)
    mag = sp.magnitude_linear(x, w, bias)
    out = "bf16" if y.dtype == torch.bfloat16 else "fp32"
    dc.assert_matches_definition(y.view(M, N), defined, mag, K, mode, layout="rows", relu=True, out=out,
                                 label=f"gemm {shape} tile {tile} ({kern})")


@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("case", ["algo1_3x3", "splitk", "wide"])
def test_generic_gemm_forms_match_their_definition(native, mode, case):
    """The generic kernel forced onto a 3x3 layer (algo 1), the split-K linear layer (fc1 at one frame: K slabs summed by a
    second launch) and the 256 x 256 tile of wide linear layers."""
    g = torch.Generator(device=DEV).manual_seed(len(case) + len(mode))
    dt = getattr(native, DT[mode])
    if case == "algo1_3x3":
        B, H, W, Cin, Cout = 2, 19, 37, 64, 128
        x = torch.randn(B, Cin, H, W, device=DEV, generator=g)
        w = torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g) / math.sqrt(9 * Cin)
        bias = torch.randn(Cout, device=DEV, generator=g)
        try:
            native.set_conv_algo(1)
            y = native.conv_fwd(operand(native, nhwc(x), mode), native.pack_conv_weight(w, Cin, dt), bias, Cout, 3)
            kern = native.last_conv_kernel()
        finally:
            native.set_conv_algo(0)
        assert kern.startswith("k_conv_fwd<bf16_t,float,2,"), kern
        defined, mag = conv_def(x, w, mode, bias=bias)
        dc.assert_matches_definition(y, defined, mag, Cin * 9, mode, label=f"generic 3x3 ({kern})")
        return
    M, K, N = (512, 25088, 1024) if case == "splitk" else (12900, 264, 1000)
    x = torch.relu(torch.randn(M, K, device=DEV, generator=g))
    w = torch.randn(N, K, device=DEV, generator=g) * 0.01
    bias = torch.randn(N, device=DEV, generator=g)
    y = native.conv_fwd(operand(native, x, mode), native.pack_fc_weight(w, dt), bias, N, 1)
    kern = native.last_conv_kernel()
    split = 2 if mode == "f16x3" else 1
    if case == "splitk":
        ran(native, f"k_conv_fwd<bf16_t,float,2,1,1,4,3,{split},128>+k_splitk_sum", "split-K")
    else:
        ran(native, f"k_conv_fwd<bf16_t,float,2,4,1,4,3,{split},64>", "256 x 256 tile")
    defined, mag = sp.linear_mode(x, w, mode, bias), sp.magnitude_linear(x, w, bias)
    dc.assert_matches_definition(y, defined, mag, K, mode, layout="rows", label=f"{case} {M}x{K}x{N} ({kern})")


# ---- full chip -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
def test_full_chip_patch_forward_matches_its_definition(native, mode):
    B, H, W, Cin, Cout = 8, 150, 300, 256, 256
    g = torch.Generator(device=DEV).manual_seed(21)
    x = torch.randn(B, Cin, H, W, device=DEV, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g) / (3 * Cin ** 0.5)
    bias = torch.randn(Cout, device=DEV, generator=g)
    y, st = native.conv_fwd(operand(native, nhwc(x), mode), native.pack_conv_weight(w, Cin, getattr(native, DT[mode])), bias,
                            Cout, 3, act=1, want_stats=True)
    kern = native.last_conv_kernel()
    mean, invstd = native.bn_finalize(st, B * H * W, Cout, torch.zeros(Cout, device=DEV), torch.ones(Cout, device=DEV), 0.1, 1e-5)
    defined, mag = conv_def(x, w, mode, bias=bias)
    del x
    dc.assert_matches_definition(y, defined, mag, Cin * 9, mode, relu=True, label=f"full-chip patch ({kern})",
                                 stats=(mean, invstd, 1e-5))


def test_full_chip_patch_wgrad_matches_its_definition(native):
    B, H, W, Cin, Cout = 8, 150, 300, 256, 256
    g = torch.Generator(device=DEV).manual_seed(22)
    x = torch.randn(B, Cin, H, W, device=DEV, generator=g)
    dy = torch.randn(B, Cout, H, W, device=DEV, generator=g) * 1e-3
    xd, dyd = native.cast(nhwc(x), native.SPLIT_DTYPE), native.cast(nhwc(dy), native.SPLIT_DTYPE)
    dw = torch.empty(Cout, Cin, 3, 3, device=DEV)
    native.conv_wgrad_oihw(xd, dyd, dw, accumulate=False)
    kern = native.last_conv_kernel()
    del xd, dyd
    defined, mag = wgrad_def(x, dy, 3, "bf16x3")
    dc.assert_matches_definition(dw, defined, mag, B * H * W, "bf16x3", layout="oihw", label=f"full-chip wgrad ({kern})")
