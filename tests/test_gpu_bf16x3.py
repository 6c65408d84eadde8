"""GPU parity tests of the SFOD_BF16X3 mode (fp32-equivalent arithmetic on the bf16 matrix pipe).

Every MFMA operand is the pair hi = bf16(v), lo = bf16(v - hi); a product is hi*hi + hi*lo + lo*hi accumulated in
fp32.  Per-product error <= 3 * 2^-16 (worst case), ~4e-6 rms measured (tools/experiments/mfma_split_precision.hip),
so every kernel here must agree with an fp64-accumulated reference on the UNROUNDED fp32 operands to ~1e-5 -- the
tolerances below are 3e-5 relative (L2), 25x tighter than the 1e-4 of BASELINE.json's north_star and >100x tighter
than what one bf16 pass achieves (2e-3).  The storage layout (8 hi | 8 lo per 8 channels) is checked bit for bit.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import definition_check as dc

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 3e-5


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def split_ref(x):
    """fp32 [..., C] -> bf16 [..., 2C] in the documented layout (per 8 channels: 8 hi then 8 lo)."""
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    s = x.shape
    hi = hi.reshape(*s[:-1], s[-1] // 8, 1, 8)
    lo = lo.reshape(*s[:-1], s[-1] // 8, 1, 8)
    return torch.cat([hi, lo], dim=-2).reshape(*s[:-1], 2 * s[-1])


def to_split(native, x_dev):
    return native.cast(x_dev.contiguous(), native.SPLIT_DTYPE)


def ran_forced(native, wg, cin):
    """A forced workgroup shape ran the kernel it names -- or, where the channel count does not allow it, the documented one."""
    if wg:
        assert native.last_conv_kernel() == dc.expected_patch_kernel(wg, 2 * cin, 1), native.last_conv_kernel()


def conv_ref64(x, w, bias=None, padding=0):
    return F.conv2d(x.double(), w.double(), None if bias is None else bias.double(), padding=padding)


def test_cast_layout_and_round_trip(native):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(37, 5, 64, generator=g) * torch.logspace(-6, 3, 64)
    x[0, 0, :8] = torch.tensor([0.0, -0.0, 1.0, 1e-30, -3e38, 65504.0, 2 ** -126, 1 + 2 ** -12])
    s = to_split(native, x.to(DEV))
    assert s.dtype == native.SPLIT_DTYPE and s.shape == x.shape
    assert torch.equal(s.view(torch.bfloat16).cpu().view(torch.int16), split_ref(x).view(torch.int16))
    back = native.cast(s, torch.float32).cpu()
    assert torch.equal(back, split_ref(x).float().reshape(37, 5, 8, 2, 8).sum(-2).reshape(37, 5, 64))
    err = ((back - x).abs() / x.abs().clamp_min(1e-37)).max().item()
    assert err <= 2.0 ** -16
    assert torch.equal(native.cast(native.cast(back.to(DEV), native.SPLIT_DTYPE), torch.float32).cpu(), back)


@pytest.mark.parametrize("shape", [
    # B, H, W, Cin, Cout, ks
    (2, 9, 13, 64, 64, 3),
    (1, 18, 37, 64, 128, 3),
    (2, 7, 5, 128, 256, 3),
    (1, 5, 6, 512, 512, 3),
    (3, 16, 16, 3, 64, 3),      # first layer: 3 channels in one 8-channel group
    (1, 18, 37, 512, 75, 1),    # RPN 1x1 heads fused
    (2, 1, 1, 256, 1024, 1),
    (1, 10, 12, 24, 40, 3),     # channel counts that are multiples of 8 only (non power of two -> 1x1 below)
])
@pytest.mark.parametrize("act", [0, 1])
def test_conv_fwd_generic_kernel(native, shape, act):
    B, H, W, Cin, Cout, ks = shape
    if Cin == 24:
        ks = 1
    g = torch.Generator().manual_seed(hash(shape) % 1000)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, ks, ks, generator=g) / math.sqrt(Cin * ks * ks)
    bias = torch.randn(Cout, generator=g)
    cin_pad = (Cin + 7) // 8 * 8
    ref = conv_ref64(x, w, bias, padding=ks // 2)
    ref = F.relu(ref) if act else ref
    xd = torch.zeros(B, H, W, cin_pad, device=DEV)
    xd[..., :Cin] = nhwc(x).to(DEV)
    wp = native.pack_conv_weight(w.to(DEV), cin_pad, native.BF16X3)
    assert wp.dtype == native.SPLIT_DTYPE
    try:
        native.set_conv_algo(1)
        y = native.conv_fwd(to_split(native, xd), wp, bias.to(DEV), Cout, ks, act=act)
        y2 = native.conv_fwd(xd, wp, bias.to(DEV), Cout, ks, act=act)     # fp32 input: converted by the wrapper
    finally:
        native.set_conv_algo(0)
    assert y.dtype == torch.float32
    assert rel_err(nchw(y.cpu()), ref) < TOL
    assert torch.equal(y, y2)


@pytest.mark.parametrize("shape", [
    # B, H, W, Cin, Cout  -- halo-patch kernel on physical channels 2 * Cin
    (2, 37, 75, 64, 128),
    (1, 20, 50, 64, 64),
    (1, 33, 40, 128, 64),
    (2, 9, 13, 16, 200),      # a single 32-physical-channel slice, Cout tail
    (1, 70, 150, 48, 136),    # several tiles per image, 3 slices
    (3, 5, 6, 256, 256),
])
@pytest.mark.parametrize("variant", ["plain", "relu_stats", "ldy"])
@pytest.mark.parametrize("wg", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9])   # 7 / 8 / 9: the 64-channel tile shapes on 16x16x32 (round 6)
def test_conv3x3_patch_kernel(native, shape, variant, wg):
    B, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, Cin, H, W, generator=g) + 0.3
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    bias = torch.randn(Cout, generator=g)
    ref = conv_ref64(x, w, bias, padding=1)
    xd = to_split(native, nhwc(x).to(DEV))
    wp = native.pack_conv_weight(w.to(DEV), Cin, native.BF16X3)
    try:
        native.set_conv_algo(2)
        native.set_conv3x3_variant(wg)
        assert native.query("sfod_conv_fwd_algo", B, H, W, Cin, Cout, 3, native.BF16X3) == 2
        if variant == "plain":
            y = native.conv_fwd(xd, wp, bias.to(DEV), Cout, 3)
            ran_forced(native, wg, Cin)
            assert rel_err(nchw(y.cpu()), ref) < TOL
        elif variant == "relu_stats":
            y, stats = native.conv_fwd(xd, wp, bias.to(DEV), Cout, 3, act=1, want_stats=True)
            ran_forced(native, wg, Cin)
            assert rel_err(nchw(y.cpu()), F.relu(ref)) < TOL
            rm, rv = torch.zeros(Cout, device=DEV), torch.ones(Cout, device=DEV)
            mean, invstd = native.bn_finalize(stats, B * H * W, Cout, rm, rv, 0.1, 1e-5)
            torch.testing.assert_close(mean.cpu().double(), ref.mean(dim=(0, 2, 3)), rtol=1e-4, atol=2e-5)
            torch.testing.assert_close(invstd.cpu().double(), torch.rsqrt(ref.var(dim=(0, 2, 3), unbiased=False) + 1e-5),
                                       rtol=1e-4, atol=1e-5)
        else:
            y = native.conv_fwd(xd, wp, None, Cout, 3, ldy=Cout + 8)
            ran_forced(native, wg, Cin)
            assert rel_err(nchw(y[..., :Cout].cpu()), ref - bias.double().view(1, -1, 1, 1)) < TOL
            assert (y[..., Cout:] == 0).all()
    finally:
        native.set_conv_algo(0)
        native.set_conv3x3_variant(0)


@pytest.mark.parametrize("shape", [(2, 9, 13, 64, 64, 3), (1, 11, 7, 128, 256, 3), (1, 6, 5, 512, 75, 1),
                                   (3, 8, 8, 3, 64, 3), (1, 40, 1, 1024, 41, 1),
                                   # bottleneck shapes on odd-sized maps (ResNet-C4 path)
                                   (2, 17, 23, 128, 128, 3), (2, 17, 23, 64, 64, 3), (2, 17, 23, 512, 128, 1),
                                   (2, 17, 23, 128, 512, 1), (2, 17, 23, 64, 256, 1),
                                   # wide-tile weight gradient (128 x 256 per workgroup): ragged tiles, many pixel splits
                                   (1, 300, 1, 1000, 200, 1), (4, 10, 10, 256, 136, 1), (2, 40, 64, 264, 128, 1)])
@pytest.mark.parametrize("algo", [1, 0, 4])      # 1: generic kernels only, 4: wide-tile weight gradient wherever it applies
def test_conv_dgrad_and_wgrad(native, shape, algo):
    B, H, W, Cin, Cout, ks = shape
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, Cin, H, W, generator=g).double().requires_grad_(True)
    w = (torch.randn(Cout, Cin, ks, ks, generator=g) / math.sqrt(Cin * ks * ks)).double().requires_grad_(True)
    dy = (torch.randn(B, Cout, H, W, generator=g) * 1e-5).double()       # gradient-sized values: no range issue in bf16 pairs
    F.conv2d(x, w, None, padding=ks // 2).backward(dy)
    cin_pad, cout_pad = (Cin + 7) // 8 * 8, (Cout + 7) // 8 * 8
    xd = torch.zeros(B, H, W, cin_pad, device=DEV)
    xd[..., :Cin] = nhwc(x.detach().float()).to(DEV)
    dyd = torch.zeros(B, H, W, cout_pad, device=DEV)
    dyd[..., :Cout] = nhwc(dy.float()).to(DEV)
    xs, dys = to_split(native, xd), to_split(native, dyd)
    try:
        native.set_conv_algo(algo)
        dwp = native.conv_wgrad(xs, dys, Cout, ks)
        dwp_f = native.conv_wgrad(xd, dyd, Cout, ks, operand=native.SPLIT_DTYPE)    # fp32 inputs converted by the wrapper
        dw = torch.empty(Cout, Cin, ks, ks, dtype=torch.float32, device=DEV)
        native.unpack_conv_wgrad(dwp.contiguous(), dw)
        assert rel_err(dw.cpu(), w.grad) < TOL
        assert rel_err(dwp_f, dwp) < 1e-6        # atomics: order of the fp32 sums may differ
        if Cin >= 8:
            wr = native.pack_conv_weight(w.detach().float().to(DEV), cout_pad, native.BF16X3, rot180=True)
            dx = native.conv_fwd(dys, wr, None, Cin, ks)
            assert rel_err(nchw(dx.cpu()), x.grad) < TOL
    finally:
        native.set_conv_algo(0)


@pytest.mark.parametrize("shape", [
    (2, 37, 75, 64, 128),
    (1, 20, 50, 32, 32),      # half-empty output-channel tile (64 per workgroup)
    (1, 33, 40, 128, 64),
    (2, 9, 13, 16, 96),
    (1, 70, 150, 48, 80),
    (3, 5, 6, 256, 256),
    (2, 30, 44, 72, 136),     # channel tails in both 64-wide blocks of the 64 x 64 kernel, tiles overhanging the map
    (1, 64, 96, 192, 64),
])
@pytest.mark.parametrize("pipe", [2, 1, 0])
def test_conv3x3_patch_wgrad(native, shape, pipe):
    """k_wgrad3x3_patch<4, SPLIT> (planes de-interleaved by the DMA, hi*lo + lo*hi + hi*hi per tap, four k-step slabs per
    pixel split) + the slab reduction against fp64 autograd; ``pipe`` (sfod_set_wgrad3x3_pipe): 2 = the 64 x 64-block kernel
    on 128-pixel tiles (k_wgrad3x3_w64, default; layers with Cin >= 64, otherwise it falls back to 1), 1 = the pipelined
    64 x 32-block loop, 0 = the round-2 loop.  0 and 1 issue the same MFMA sequence per accumulator (bit-equal); 2 groups
    the pixels differently (equal to fp32 summation order)."""
    B, H, W, Cin, Cout = shape
    native.set_wgrad3x3_pipe(pipe)
    g = torch.Generator().manual_seed(sum(shape) + 1)
    x = torch.randn(B, Cin, H, W, generator=g)
    dy = torch.randn(B, Cout, H, W, generator=g) * 1e-4
    w = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, None, padding=1).backward(dy.double())
    xd, dyd = to_split(native, nhwc(x).to(DEV)), to_split(native, nhwc(dy).to(DEV))
    try:
        native.set_conv_algo(2)
        assert native.query("sfod_conv_wgrad_ws_bytes", B, H, W, Cin, Cout, 3, Cout, native.BF16X3) >= 16 * Cout * 9 * Cin
        dwp = native.conv_wgrad(xd, dyd, Cout, 3)
        ran = {2: "k_wgrad3x3_w64" if Cin >= 64 else "k_wgrad3x3_patch<4,1,1>", 1: "k_wgrad3x3_patch<4,1,1>",
               0: "k_wgrad3x3_patch<4,1,0>"}[pipe]
        assert native.last_conv_kernel() == ran, native.last_conv_kernel()
        dwp2 = native.conv_wgrad(xd, dyd, Cout, 3)
        assert native.conv_wgrad_oihw_supported(xd, dyd, Cout, 3)
        direct = torch.full((Cout, Cin, 3, 3), float("nan"), dtype=torch.float32, device=DEV)
        native.conv_wgrad_oihw(xd, dyd, direct, accumulate=False)
        acc = torch.ones(Cout, Cin, 3, 3, dtype=torch.float32, device=DEV)
        native.conv_wgrad_oihw(xd, dyd, acc, accumulate=True)
        native.set_wgrad3x3_pipe((pipe + 1) % 3)
        other = native.conv_wgrad(xd, dyd, Cout, 3)
    finally:
        native.set_conv_algo(0)
        native.set_wgrad3x3_pipe(2)
    dw = torch.empty(Cout, Cin, 3, 3, dtype=torch.float32, device=DEV)
    native.unpack_conv_wgrad(dwp, dw)
    assert rel_err(dw.cpu(), w.grad) < TOL
    assert torch.equal(dwp, dwp2), "slab reduction must be deterministic"
    if {pipe, (pipe + 1) % 3} == {0, 1} or Cin < 64:
        assert torch.equal(dwp, other), "both 64 x 32 chunk loops issue the same MFMA sequence per accumulator"
    else:
        assert rel_err(other.cpu(), dwp.cpu()) < 2e-6, "same products, other pixel grouping: fp32 summation order only"
    assert torch.equal(direct, dw)
    torch.testing.assert_close(acc, dw + 1.0, rtol=0, atol=1e-6)


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("hw", [(8, 12), (7, 9), (37, 75)])
def test_bn_relu_pool_split_outputs_equal_fp32_kernels(native, pool, hw):
    """BatchNorm apply / backward writing (hi, lo) pairs == the fp32 kernels' outputs converted afterwards (the two
    instantiations may contract a*b+c differently: equal within one fp32 rounding + the 2^-16 of the pair format)."""
    H, W = hw
    B, C = 2, 64
    g = torch.Generator().manual_seed(5)
    y = torch.randn(B, H, W, C, generator=g).to(DEV)
    mean, var = y.mean(dim=(0, 1, 2)), y.var(dim=(0, 1, 2), unbiased=False)
    invstd = torch.rsqrt(var + 1e-5)
    gamma, beta = torch.rand(C, generator=g).to(DEV) + 0.5, torch.randn(C, generator=g).to(DEV) * 0.1
    z32 = native.bn_relu_pool_fwd(y, mean, invstd, gamma, beta, pool)
    zs = native.bn_relu_pool_fwd(y, mean, invstd, gamma, beta, pool, out_dtype=native.SPLIT_DTYPE)
    assert zs.dtype == native.SPLIT_DTYPE and zs.shape == z32.shape
    zb = native.cast(zs, torch.float32)
    assert ((zb - z32).abs() <= z32.abs() * 2.0 ** -16 + 1e-6).all()
    assert ((zb == 0) == (z32 == 0)).all()           # ReLU zeros stay exact zeros
    dz = torch.randn(z32.shape, generator=g).to(DEV) * 1e-4
    dy32, dg32, db32 = native.bn_relu_pool_bwd(dz, y, mean, invstd, gamma, beta, pool)
    dys, dgs, dbs = native.bn_relu_pool_bwd(dz, y, mean, invstd, gamma, beta, pool, out_dtype=native.SPLIT_DTYPE)
    assert torch.equal(dg32, dgs) and torch.equal(db32, dbs)
    assert ((native.cast(dys, torch.float32) - dy32).abs() <= dy32.abs() * 2.0 ** -16 + 1e-10).all()


def test_roi_align_fwd_split(native):
    g = torch.Generator().manual_seed(3)
    B, H, W, C, R = 2, 19, 38, 64, 200
    feat = torch.randn(B, H, W, C, generator=g).to(DEV)
    xy = torch.rand(R, 2, generator=g) * torch.tensor([W * 32.0, H * 32.0])
    wh = torch.rand(R, 2, generator=g) * 300 + 4
    rois = torch.cat([torch.randint(0, B, (R, 1), generator=g).float(), xy, xy + wh], dim=1)
    rois[7, 0] = -1          # padding row
    rois = rois.to(DEV)
    # reference: the fp32 kernel on the values the pairs hold
    fs = to_split(native, feat)
    ref = native.roi_align_fwd(native.cast(fs, torch.float32), rois, 7, 1.0 / 32)
    out = native.roi_align_fwd(fs, rois, 7, 1.0 / 32)
    assert out.dtype == native.SPLIT_DTYPE and out.shape == ref.shape
    got = native.cast(out, torch.float32)
    assert (got[7] == 0).all()
    assert rel_err(got.cpu(), ref.cpu()) < 2.0 ** -16


def test_preprocess_split(native):
    g = torch.Generator().manual_seed(1)
    imgs = [torch.randint(0, 256, (3, 20, 31), dtype=torch.uint8, generator=g).to(DEV),
            torch.randint(0, 256, (3, 17, 40), dtype=torch.uint8, generator=g).to(DEV)]
    mean, std = [103.53, 116.28, 123.675], [1.0, 57.0, 2.5]
    x32, _ = native.preprocess(imgs, 20, 40, 8, mean, std, native.F32)
    xs, _ = native.preprocess(imgs, 20, 40, 8, mean, std, native.BF16X3)
    assert xs.dtype == native.SPLIT_DTYPE and xs.shape == (2, 20, 40, 8)
    assert torch.equal(xs.view(torch.bfloat16), to_split(native, x32).view(torch.bfloat16))


def test_weight_packers_split(native):
    g = torch.Generator().manual_seed(2)
    w = torch.randn(40, 24, 3, 3, generator=g).to(DEV)
    for rot in (False, True):
        inner = 40 if rot else 24
        p32 = native.pack_conv_weight(w, inner, native.F32, rot180=rot)
        ps = native.pack_conv_weight(w, inner, native.BF16X3, rot180=rot)
        assert torch.equal(ps.view(torch.bfloat16), to_split(native, p32).view(torch.bfloat16))
    pk32 = native.ConvWeightPacker([(w, 24, False), (w, 40, True)], native.F32).pack()
    pks = native.ConvWeightPacker([(w, 24, False), (w, 40, True)], native.BF16X3).pack()
    for a, b in zip(pk32, pks):
        assert torch.equal(b.view(torch.bfloat16), to_split(native, a.contiguous()).view(torch.bfloat16))
    fc = torch.randn(1024, 512 * 49, generator=g).to(DEV)          # fc1-shaped: tiled (c, p) -> (p, c) path
    for tr in (False, True):
        a = native.pack_fc_weight(fc, native.F32, chw_c=512, transpose=tr)
        b = native.pack_fc_weight(fc, native.BF16X3, chw_c=512, transpose=tr)
        assert torch.equal(b.view(torch.bfloat16), to_split(native, a).view(torch.bfloat16))
    small = torch.randn(41, 1024, generator=g).to(DEV)
    a = native.pack_fc_weight(small, native.F32, transpose=True, ld=48)
    b = native.pack_fc_weight(small, native.BF16X3, transpose=True, ld=48)
    assert torch.equal(b.view(torch.bfloat16), to_split(native, a).view(torch.bfloat16))


@pytest.mark.parametrize("hw", [(50, 70), (64, 96), (9, 500)])
def test_conv_first_layer_kernel_split(native, hw):
    """The first-layer kernel in bf16x3 (pairs in, fp32 out + BatchNorm statistics): image edges, tiles hanging over
    the right / bottom border; against fp64 on the unrounded operands, and equal statistics from the store-free pass."""
    H, W = hw
    B, Cout = 2, 64
    g = torch.Generator().manual_seed(H * W)
    x = torch.zeros(B, H, W, 8)
    x[..., :3] = torch.randn(B, H, W, 3, generator=g) * 50
    w = torch.randn(Cout, 3, 3, 3, generator=g) / 5
    bias = torch.randn(Cout, generator=g)
    ref = conv_ref64(nchw(x)[:, :3], w, bias, padding=1)
    xd = to_split(native, x.to(DEV))
    wp = native.pack_conv_weight(w.to(DEV), 8, native.BF16X3)
    assert native.conv_first_supported(xd, 64)
    assert native.query("sfod_conv_fwd_algo", B, H, W, 8, Cout, 3, native.BF16X3) == 3
    y, st = native.conv_fwd(xd, wp, bias.to(DEV), Cout, 3, want_stats=True)
    assert y.dtype == torch.float32
    assert rel_err(nchw(y.cpu()), ref) < TOL
    y2 = native.conv_fwd(xd, wp, bias.to(DEV), Cout, 3)
    assert torch.equal(y, y2)
    st2 = native.conv_first_stats(xd, wp, bias.to(DEV))
    assert st.nblk == st2.nblk and torch.equal(st, st2)
    rm, rv = torch.zeros(Cout, device=DEV), torch.ones(Cout, device=DEV)
    mean, invstd = native.bn_finalize(st, B * H * W, Cout, rm, rv, 0.1, 1e-5)
    torch.testing.assert_close(mean.cpu().double(), ref.mean(dim=(0, 2, 3)), rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(invstd.cpu().double(), torch.rsqrt(ref.var(dim=(0, 2, 3), unbiased=False) + 1e-5),
                               rtol=2e-5, atol=1e-9)
    try:
        native.set_conv_algo(1)
        y_gen = native.conv_fwd(xd, wp, bias.to(DEV), Cout, 3)
    finally:
        native.set_conv_algo(0)
    assert rel_err(y.cpu(), y_gen.cpu()) < TOL
    # second pass of the forward-only (teacher) form: the next layer's operand pairs, written directly
    gamma, beta = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.2
    scale = gamma.to(DEV) * invstd
    shift = beta.to(DEV) - mean * scale
    z = native.conv_first_apply(xd, wp, bias.to(DEV), scale, shift, relu=True)
    assert z.dtype == native.SPLIT_DTYPE
    zref = F.relu(F.batch_norm(ref, None, None, gamma.double(), beta.double(), True, 0.1, 1e-5))
    zf = native.cast(z, torch.float32).cpu()
    assert rel_err(nchw(zf), zref) < TOL
    # the pairs are the exact split of an fp32 value: the unfused path (fp32 y -> BN kernel -> pairs) agrees to fp32 rounding
    z2 = native.bn_relu_pool_fwd(y, mean, invstd, gamma.to(DEV), beta.to(DEV), False, out_dtype=native.SPLIT_DTYPE)
    assert rel_err(zf, native.cast(z2, torch.float32).cpu()) < 1e-6


@pytest.mark.parametrize("wg", [2, 5, 6, 7, 9])      # (7, 9: the 64-channel tiles on 16x16x32; 256-pixel tiles like 2: same statistics blocks)
def test_conv3x3_pairs_under_load_is_deterministic(native, wg):
    """Full-chip launch on operand pairs (two workgroups per CU): the 32x32x16 kernel (2) and the 16x16x32 kernel (5) must
    each be run-to-run bit-identical -- guards the counted-wait DMA pipelines, whose hazards (a fragment read still queued
    when another wave's DMA overwrites its slot; a stage read before its DMA landed) only show under load -- and agree
    with each other to fp32 summation order."""
    B, H, W, Cin, Cout = 8, 150, 300, 256, 256
    g = torch.Generator(device=DEV).manual_seed(1)
    x = to_split(native, torch.randn(B, H, W, Cin, device=DEV, generator=g))
    w = to_split(native, torch.randn(Cout, 9, Cin, device=DEV, generator=g) / (3 * Cin ** 0.5))
    bias = torch.randn(Cout, device=DEV, generator=g)
    try:
        native.set_conv_algo(2)
        native.set_conv3x3_variant(2)
        ref, ref_stats = native.conv_fwd(x, w, bias, Cout, 3, want_stats=True)
        ran_forced(native, 2, Cin)
        native.set_conv3x3_variant(wg)
        outs = [native.conv_fwd(x, w, bias, Cout, 3, want_stats=True) for _ in range(6)]
        ran_forced(native, wg, Cin)     # the kernel under test, not a fallback: Cin = 256 takes every shape
        torch.cuda.synchronize()
    finally:
        native.set_conv_algo(0)
        native.set_conv3x3_variant(0)
    for y, st in outs[1:]:
        assert torch.equal(outs[0][0], y), "pair conv is not run-to-run deterministic"
        assert torch.equal(outs[0][1], st), "pair conv statistics are not run-to-run deterministic"
    assert rel_err(outs[0][0], ref) < 2e-6
    torch.testing.assert_close(outs[0][1], ref_stats, rtol=2e-4, atol=2e-3)


@pytest.mark.parametrize("shape", [(2, 37, 75, 64, 128), (1, 40, 64, 128, 64), (2, 18, 25, 256, 256), (1, 33, 31, 64, 64)])
@pytest.mark.parametrize("variant", [0, 1, 2, 4, 5, 6, 7, 8, 9])
def test_dgrad_with_fused_batchnorm_backward_reduction(native, shape, variant):
    """sfod_conv_dgrad_bnred: the data-gradient kernel's epilogue also makes the (dbeta, dgamma) partial sums of the layer
    below.  dz must be bit-identical to the plain kernel's, and BatchNorm backward fed with the pre-reduced workspace must
    give the dy / dgamma / dbeta of the unfused three-kernel form (different summation order: 1e-5)."""
    B, H, W, Cup, C = shape          # upper layer: C -> Cup channels; its data gradient has C channels
    g = torch.Generator().manual_seed(B * H + W + C)
    dy_up = torch.randn(B, H, W, Cup, generator=g) * 1e-3
    w = torch.randn(Cup, C, 3, 3, generator=g) / math.sqrt(9 * C)
    y = torch.randn(B, H, W, C, generator=g) * 2 + 0.3
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    yd = y.to(DEV)
    mean = yd.mean(dim=(0, 1, 2))
    invstd = torch.rsqrt(yd.var(dim=(0, 1, 2), unbiased=False) + 1e-5)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    dys = to_split(native, dy_up.to(DEV))
    wr = native.pack_conv_weight(w.to(DEV), Cup, native.BF16X3, rot180=True)
    try:
        native.set_conv3x3_variant(variant)
        # small maps / narrow layers may go to the generic kernel, which has no such epilogue: then the op must refuse
        served = native.query("sfod_conv_dgrad_bnred_blocks", B, H, W, Cup, C, native.BF16X3) > 0
        assert served or variant != 0 or shape == (1, 33, 31, 64, 64)
        dz_ref = native.conv_fwd(dys, wr, None, C, 3)
        if variant:     # the forced shape ran, or -- where the planner keeps this layer off the halo-patch kernel -- the generic one
            if native.query("sfod_conv_fwd_algo", B, H, W, Cup, C, 3, native.BF16X3) == 2:
                assert native.last_conv_kernel() == dc.expected_patch_kernel(variant, 2 * Cup, 1), native.last_conv_kernel()
            else:
                assert native.last_conv_kernel().startswith("k_conv_fwd<bf16_t,float,2,"), native.last_conv_kernel()
        fused = native.conv_dgrad_bnred(dys, wr, C, yd, mean, invstd, gd, bd)
        if fused is not None and variant:      # the same shape with the BatchNorm-backward epilogue
            assert native.last_conv_kernel() == dc.expected_patch_kernel(variant, 2 * Cup, 1, red=True), native.last_conv_kernel()
    finally:
        native.set_conv3x3_variant(0)
    if not served:
        assert fused is None
        return
    assert fused is not None
    dz, ws = fused
    assert torch.equal(dz, dz_ref)
    ref = native.bn_relu_pool_bwd(dz_ref, yd, mean, invstd, gd, bd, False, out_dtype=native.SPLIT_DTYPE)
    got = native.bn_relu_pool_bwd(dz, yd, mean, invstd, gd, bd, False, out_dtype=native.SPLIT_DTYPE, reduced=ws)
    for a, b, name in zip(got[1:], ref[1:], ("dgamma", "dbeta")):
        assert rel_err(a.cpu(), b.cpu()) < 1e-5, name
    assert rel_err(native.cast(got[0], torch.float32).cpu(), native.cast(ref[0], torch.float32).cpu()) < 1e-5
    # and against fp64 autograd of relu(bn(y)) with the same upstream gradient
    y64 = y.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z = F.relu(F.batch_norm(y64.permute(0, 3, 1, 2), None, None, g64, b64, True, 0.1, 1e-5))
    z.backward(dz_ref.cpu().double().permute(0, 3, 1, 2))
    assert rel_err(got[1].cpu(), g64.grad) < 2e-5 and rel_err(got[2].cpu(), b64.grad) < 2e-5
    assert rel_err(native.cast(got[0], torch.float32).cpu(), y64.grad) < 2e-5
    # shapes the halo-patch kernel does not serve are refused by the query, not silently mis-served
    assert native.query("sfod_conv_dgrad_bnred_blocks", B, H, W, Cup, C, native.BF16) == 0
    assert native.conv_dgrad_bnred(dys, wr, C, yd.bfloat16(), mean, invstd, gd, bd) is None


@pytest.mark.parametrize("shape", [(12900, 264, 1000), (17000, 1032, 520), (51300, 72, 256)])
def test_linear_wide_tile_kernel(native, shape):
    """k_conv_fwd<.., WN = 4, BKB = 64>: the 256 x 256 tile with 64-byte K stages that the long-K linear layers of the
    benchmark shapes select (teacher fc1: 16000 rows).  Ragged M, N and K tails; bias + ReLU epilogue, the BatchNorm
    statistics epilogue, and agreement with the 256 x 128 kernel (SFOD_GEMM_WIDE is read once per process, so the
    selection is checked through the tile count the rule uses: >= 200 wide tiles that fill their rounds)."""
    M, K, N = shape
    g = torch.Generator().manual_seed(M + K)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g)
    t256 = ((M + 255) // 256) * ((N + 255) // 256)
    t128 = ((M + 255) // 256) * ((N + 127) // 128)
    assert t256 >= 200 and ((t256 + 255) // 256) * 0.8 <= ((t128 + 255) // 256) * 0.5, "shape must select the wide tile"
    assert native.query("sfod_conv_fwd_algo", M, 1, 1, K, N, 1, native.BF16X3) == 4
    assert native.query("sfod_conv_fwd_algo", M // 2, 1, 1, K, N, 1, native.BF16X3) == 1
    xd = to_split(native, x.to(DEV))
    wp = native.pack_fc_weight(w.to(DEV), native.BF16X3)
    y, st = native.conv_fwd(xd.view(M, 1, 1, K), wp, bias.to(DEV), N, 1, act=0, want_stats=True)
    ref = x.double() @ w.double().t() + bias.double()
    assert rel_err(y.view(M, N).cpu(), ref) < TOL
    rm, rv = torch.zeros(N, device=DEV), torch.ones(N, device=DEV)
    mean, invstd = native.bn_finalize(st, M, N, rm, rv, 0.1, 1e-5)
    torch.testing.assert_close(mean.cpu().double(), ref.mean(0), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(invstd.cpu().double(), torch.rsqrt(ref.var(0, unbiased=False) + 1e-5), rtol=2e-5, atol=1e-9)
    yr = native.conv_fwd(xd.view(M, 1, 1, K), wp, bias.to(DEV), N, 1, act=1)
    assert rel_err(yr.view(M, N).cpu(), F.relu(ref)) < TOL
    # the same rows in two halves take the 256 x 128 kernel (fewer than 200 wide tiles): same values to fp32 rounding
    h = M // 2
    y2 = torch.cat([native.conv_fwd(xd[:h].contiguous().view(h, 1, 1, K), wp, bias.to(DEV), N, 1).view(h, N),
                    native.conv_fwd(xd[h:].contiguous().view(M - h, 1, 1, K), wp, bias.to(DEV), N, 1).view(M - h, N)])
    assert rel_err(y.view(M, N).cpu(), y2.cpu()) < 1e-6


@pytest.mark.parametrize("rows", [1, 700, 2049, 22800])
def test_bn_backward_with_a_prereduced_workspace_of_any_length(native, rows):
    """sfod_bn_relu_pool_bwd(reduced_blocks): the (dbeta | dgamma) partial rows of the fused data-gradient epilogue are summed
    by one kernel up to 2048 rows and in two stages (32 slices) beyond -- conv1_1 at B = 8, 600x1200 has 22 800 rows."""
    C, B, H, W = 64, 1, 8, 8
    g = torch.Generator().manual_seed(rows)
    part = torch.randn(rows + native.BN_BWD_SCRATCH_ROWS, 2 * C, generator=g)
    part[rows:] = float("nan")                       # scratch rows: must be overwritten before they are read
    y = torch.randn(B, H, W, C, generator=g).to(DEV)
    dz = torch.randn(B, H, W, C, generator=g).to(DEV)
    mean, invstd = y.mean(dim=(0, 1, 2)), torch.rsqrt(y.var(dim=(0, 1, 2), unbiased=False) + 1e-5)
    gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    dy, dgamma, dbeta = native.bn_relu_pool_bwd(dz, y, mean, invstd, gamma, beta, False, reduced=part.to(DEV))
    ref = part[:rows].double().sum(0)
    torch.testing.assert_close(dbeta.cpu().double(), ref[:C], rtol=1e-6, atol=1e-5)
    torch.testing.assert_close(dgamma.cpu().double(), ref[C:], rtol=1e-6, atol=1e-5)
    assert torch.isfinite(dy).all()


def test_conv3x3_patch_wgrad_pipelined_loop_under_load(native):
    """The pipelined chunk loop on a layer-sized problem (many tiles per workgroup, border and interior tiles, every CU
    busy): run-to-run identical and bit-equal to the round-2 loop -- an ordering hazard between the early fragment reads
    and the LDS-DMA would show as scattered wrong tiles."""
    B, H, W, Cin, Cout = 8, 75, 150, 256, 256
    g = torch.Generator(device=DEV).manual_seed(3)
    xd = native.cast(torch.randn(B, H, W, Cin, device=DEV, generator=g), native.SPLIT_DTYPE)
    dyd = native.cast(torch.randn(B, H, W, Cout, device=DEV, generator=g) * 1e-3, native.SPLIT_DTYPE)
    try:
        native.set_conv_algo(2)
        native.set_wgrad3x3_pipe(0)
        ref = native.conv_wgrad(xd, dyd, Cout, 3).clone()
        native.set_wgrad3x3_pipe(1)
        for _ in range(6):
            out = native.conv_wgrad(xd, dyd, Cout, 3)
            assert torch.equal(out, ref)
        native.set_wgrad3x3_pipe(2)          # 64 x 64 blocks on 128-pixel tiles: deterministic, fp32-summation-order equal
        first = native.conv_wgrad(xd, dyd, Cout, 3).clone()
        assert rel_err(first.cpu(), ref.cpu()) < 2e-6
        for _ in range(6):
            assert torch.equal(native.conv_wgrad(xd, dyd, Cout, 3), first)
    finally:
        native.set_conv_algo(0)
        native.set_wgrad3x3_pipe(2)


@pytest.mark.parametrize("shape,forced", [
    ((4, 150, 300, 256, 256), False),     # conv3_2 / conv3_3 of four 600 x 1200 frames: the planner's own choice
    ((4, 75, 150, 512, 512), False),      # conv4_x
    ((1, 300, 600, 128, 128), False),     # conv2_2, one frame
    ((6, 77, 149, 128, 256), False),      # ragged right / bottom tiles (tile overhang and the zero padding share patch rows)
    ((1, 150, 300, 256, 256), True),      # batch 1: the planner prefers another shape; the fold's own shape forced for both sides
    ((3, 41, 67, 64, 128), True),         # one 64-channel super-body: the prologue transform is the only slice-0 one
    ((2, 9, 13, 192, 64), True),          # three super-bodies, 64 output channels (half a channel tile), a map smaller than a tile
])
def test_conv3x3_with_batchnorm_folded_into_its_input(native, shape, forced):
    """sfod_conv_fwd_bnin: the convolution DMAs the producer's pre-BatchNorm fp32 tensor and turns it into relu(bn(.)) operand
    pairs inside its LDS patch.  Output and BatchNorm partial statistics must be bit-identical to the two-launch form
    (sfod_bn_relu_pool_fwd writing pairs, then sfod_conv_fwd on the same kernel shape): same arithmetic, operation for
    operation, and padding / tile-overhang rows stay zero (relu(beta - mean * scale) is not zero)."""
    B, H, W, Cin, Cout = shape
    g = torch.Generator(device=DEV).manual_seed(B + H + Cin)
    y_pre = torch.randn(B, H, W, Cin, device=DEV, generator=g) * 1.7 + 0.4
    gamma = torch.rand(Cin, device=DEV, generator=g) + 0.5
    beta = torch.rand(Cin, device=DEV, generator=g) + 0.2       # positive: a non-zero padding row would show
    mean = y_pre.mean(dim=(0, 1, 2))
    invstd = torch.rsqrt(y_pre.var(dim=(0, 1, 2), unbiased=False) + 1e-5)
    w = to_split(native, torch.randn(Cout, 9, Cin, device=DEV, generator=g) / (3 * Cin ** 0.5))
    bias = torch.randn(Cout, device=DEV, generator=g)
    if forced:
        assert not native.conv_fwd_bnin_supported(y_pre, w, Cout)        # (which is why it is forced)
        with pytest.raises(RuntimeError, match="not served"):
            native.conv_fwd_bnin(y_pre, mean, invstd, gamma, beta, w, bias, Cout)
    z = native.bn_relu_pool_fwd(y_pre, mean, invstd, gamma, beta, False, out_dtype=native.SPLIT_DTYPE)
    try:
        if forced:
            native.set_conv_algo(2)
            native.set_conv3x3_variant(6)
        assert native.conv_fwd_bnin_supported(y_pre, w, Cout), "a headline layer shape is not served"
        native.set_conv3x3_m16(2)           # the fold lives in the 4-wave shape: compare on the same accumulation order
        ref, ref_stats = native.conv_fwd(z, w, bias, Cout, 3, want_stats=True)
        outs = [native.conv_fwd_bnin(y_pre, mean, invstd, gamma, beta, w, bias, Cout, want_stats=True) for _ in range(3)]
        y1 = native.conv_fwd_bnin(y_pre, mean, invstd, gamma, beta, w, bias, Cout, act=1)
        native.set_conv3x3_m16(1)
        ref8, _ = native.conv_fwd(z, w, bias, Cout, 3, want_stats=True)
        torch.cuda.synchronize()
    finally:
        native.set_conv3x3_m16(1)
        native.set_conv3x3_variant(0)
        native.set_conv_algo(0)
    for y, st in outs:
        assert torch.equal(y, ref), "folded BatchNorm input differs from the two-launch form: max |d| = {}".format(
            (y - ref).abs().max().item())
        assert torch.equal(st, ref_stats)
    assert torch.equal(y1, torch.relu(ref))
    assert rel_err(outs[0][0], ref8) < 2e-6


def test_conv3x3_batchnorm_input_under_load_is_deterministic(native):
    """Full-chip launch of the fold (the in-LDS transform runs between the pipeline's barriers: a transform racing a DMA or a
    fragment read only shows under load)."""
    B, H, W, Cin, Cout = 8, 150, 300, 256, 256
    g = torch.Generator(device=DEV).manual_seed(5)
    y_pre = torch.randn(B, H, W, Cin, device=DEV, generator=g)
    gamma = torch.rand(Cin, device=DEV, generator=g) + 0.5
    beta = torch.rand(Cin, device=DEV, generator=g)
    mean = y_pre.mean(dim=(0, 1, 2))
    invstd = torch.rsqrt(y_pre.var(dim=(0, 1, 2), unbiased=False) + 1e-5)
    w = to_split(native, torch.randn(Cout, 9, Cin, device=DEV, generator=g) / (3 * Cin ** 0.5))
    bias = torch.randn(Cout, device=DEV, generator=g)
    z = native.bn_relu_pool_fwd(y_pre, mean, invstd, gamma, beta, False, out_dtype=native.SPLIT_DTYPE)
    try:
        native.set_conv3x3_m16(2)
        ref, ref_stats = native.conv_fwd(z, w, bias, Cout, 3, want_stats=True)
    finally:
        native.set_conv3x3_m16(1)
    outs = [native.conv_fwd_bnin(y_pre, mean, invstd, gamma, beta, w, bias, Cout, want_stats=True) for _ in range(6)]
    torch.cuda.synchronize()
    for y, st in outs:
        assert torch.equal(y, ref) and torch.equal(st, ref_stats)



@pytest.mark.parametrize("fmt", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("shape", [(22800, 256, 1024), (5000, 96, 200), (700, 1024, 256)])
@pytest.mark.parametrize("tile", [6, 7, 8])
def test_gemm_tiles_with_64_byte_stages_equal_the_planners_choice(native, shape, fmt, tile):
    """The round-6 tile shapes of the generic kernel (64-byte K stages: two / three workgroups per CU; sfod_set_gemm_tile 6 / 7 / 8)
    against the planner's own choice on the same operands: the same products in another summation order (fp32 rounding), the same
    BatchNorm statistics to their tolerance, and within the mode's tolerance of fp64.  Ragged M / N / K tails included."""
    M, K, N = shape
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g)
    if fmt == "bf16x3":
        xd, wp = to_split(native, x.to(DEV)), native.pack_fc_weight(w.to(DEV), native.BF16X3)
    else:
        xd, wp = native.cast(x.to(DEV), native.SPLITH_DTYPE), native.pack_fc_weight(w.to(DEV), native.F16X3)
    xd = xd.view(M, 1, 1, -1)
    try:
        native.set_gemm_tile(0)
        y0, st0 = native.conv_fwd(xd, wp, bias.to(DEV), N, 1, act=1, want_stats=True)
        native.set_gemm_tile(tile)
        y1, st1 = native.conv_fwd(xd, wp, bias.to(DEV), N, 1, act=1, want_stats=True)
        wn, wr, nst = {6: (2, 4, 3), 7: (2, 2, 3), 8: (2, 4, 4)}[tile]
        split = 1 if fmt == "bf16x3" else 2
        assert native.last_conv_kernel() == f"k_conv_fwd<bf16_t,float,2,{wn},1,{wr},{nst},{split},64>", native.last_conv_kernel()
        torch.cuda.synchronize()
    finally:
        native.set_gemm_tile(0)
    ref = x.double() @ w.double().t() + bias.double()
    assert rel_err(y1.view(M, N).cpu(), F.relu(ref)) < TOL and rel_err(y1, y0) < 2e-6
    rm, rv = torch.zeros(N, device=DEV), torch.ones(N, device=DEV)
    m0, i0 = native.bn_finalize(st0, M, N, rm.clone(), rv.clone(), 0.1, 1e-5)
    m1, i1 = native.bn_finalize(st1, M, N, rm.clone(), rv.clone(), 0.1, 1e-5)
    torch.testing.assert_close(m1, m0, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(i1, i0, rtol=1e-5, atol=1e-9)
