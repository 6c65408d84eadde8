"""The kernels between the convolutions against their DEFINITIONS, per element: BatchNorm (+ ReLU, + 2x2 max-pool) forward and
backward, the running statistics of sfod_bn_finalize, the bias gradient (fp64 definitions of oracle/pointwise_definitions.py,
bounds of tests/helpers/definition_check.py: counted roundings, nothing fitted), and the pointwise kernels (joins, gates,
dropout mask, stride-2 subsampling, 3x3 max-pool) bit for bit against single fp32 torch operations on the CPU.

The whole-tensor relative-L2 gates of tests/test_gpu_ops.py stay; they let one wrong channel vector, one leftover pixel of an
odd map or one workgroup's partial row through (tests/test_definition_checker.py plants those).  Shapes are the smallest that
reach each branch of the dispatch code; the comments say which.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import definition_check as dc
from helpers import pointwise_cases as pc
from oracle import pointwise_definitions as pd

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24

# (B, H, W, C), the modes it runs in.  Modes: fp32 / bf16 in and out; bf16x3 / f16x3: fp32 in, operand pairs out (f16x3 with
# the second, bf16-pair output of the dual kernel).
BN_SHAPES = [
    ((2, 7, 9, 64), ("fp32", "bf16", "bf16x3", "f16x3")),     # odd both ways: leftover row and column; grid stride % (C / V) == 0
    ((1, 8, 12, 72), ("fp32", "bf16", "bf16x3", "f16x3")),    # C / V does not divide 256: idle lanes in the reduce, the indexed walk
    ((1, 1, 1, 8), ("fp32", "bf16", "bf16x3", "f16x3")),      # no window at all (pooled output is empty, one leftover pixel)
    ((1, 33, 37, 1024), ("fp32",)),                           # one unit lane; more units than 1024 workgroups cover in one pass
    ((1, 5, 6, 2048), ("bf16",)),                             # C / V = 256
]
BN_CASES = [pytest.param(s, m, id=f"{'x'.join(map(str, s))}-{m}") for s, modes in BN_SHAPES for m in modes]


def _dev(c):
    return {k: (v.to(DEV) if v is not None else None) for k, v in c.items()}


def _in_dtype(mode):
    return torch.bfloat16 if mode == "bf16" else torch.float32


def _out_dtype(native, mode):
    return {"fp32": None, "bf16": None, "bf16x3": native.SPLIT_DTYPE, "f16x3": native.SPLITH_DTYPE}[mode]


def _f32(native, t):
    return native.cast(t, torch.float32) if native.is_pairs(t.dtype) else t


# ---- BatchNorm forward -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,mode", BN_CASES)
def test_batchnorm_forward_matches_its_definition(native, shape, mode):
    """bn_relu_pool_fwd / fwd2, pool and ReLU on and off, every output type: 5 u mag + the output rounding, per element."""
    for pool in (False, True):
        c = _dev(pc.bn_inputs(shape, _in_dtype(mode), pool, seed=1))
        z_pre, mag = pd.bn_affine(c["y"], c["mean"], c["invstd"], c["gamma"], c["beta"])
        if pool:
            z_pre, mag = pd.pool2x2(z_pre), pd.pool2x2(mag)
        for relu in (True, False):
            got = native.bn_relu_pool_fwd(c["y"], c["mean"], c["invstd"], c["gamma"], c["beta"], pool, relu=relu,
                                          out_dtype=_out_dtype(native, mode), with_grad_operand=mode == "f16x3")
            defined = torch.relu(z_pre) if relu else z_pre
            outs = [(got, mode)] if mode != "f16x3" else [(got[0], "f16x3"), (got[1], "bf16x3")]
            for z, out in outs:
                assert tuple(z.shape) == tuple(defined.shape)
                if defined.numel() == 0:             # a map without any 2x2 window pools to nothing
                    continue
                dc.assert_matches_definition(_f32(native, z), defined, mag, 1, mode, out=out,
                                             bnd=dc.bn_forward_bound(defined, mag, out), uniform=("block",),
                                             label=f"bn fwd {shape} pool={int(pool)} relu={int(relu)} -> {out}")


@pytest.mark.parametrize("shape,mode", BN_CASES)
def test_batchnorm_add_relu_forward_matches_its_definition(native, shape, mode):
    """relu(bn(y) + residual) in one pass, with the operand-pair copies of the dual kernel (both of its walks: the grid stride
    is a multiple of C / 8 at 64 channels and not at 72)."""
    c = _dev(pc.bn_inputs(shape, _in_dtype(mode), False, seed=2, residual=True))
    z_pre, mag = pd.bn_affine(c["y"], c["mean"], c["invstd"], c["gamma"], c["beta"], c["residual"])
    defined = torch.relu(z_pre)
    got = native.bn_add_relu_fwd(c["y"], c["mean"], c["invstd"], c["gamma"], c["beta"], c["residual"],
                                 with_operand=_out_dtype(native, mode), with_grad_operand=mode == "f16x3")
    base = "bf16" if mode == "bf16" else "fp32"
    outs = [(got, base)] if mode in ("fp32", "bf16") else [(got[0], "fp32"), (got[1], mode)]
    if mode == "f16x3":
        outs.append((got[2], "bf16x3"))
    for z, out in outs:
        dc.assert_matches_definition(_f32(native, z), defined, mag, 1, mode, out=out, bnd=dc.bn_forward_bound(defined, mag, out), uniform=("block",),
                                     label=f"bn add relu {shape} -> {out}")


# ---- BatchNorm backward ----------------------------------------------------------------------------------------------------
def _check_backward(native, c, shape, mode, pool, relu, expect_ties=None):
    out = {"fp32": "fp32", "bf16": "bf16", "bf16x3": "bf16x3"}[mode]
    defn, mag = pd.bn_backward(c["dz"], c["y"], c["mean"], c["invstd"], c["gamma"], c["beta"], pool, relu)
    # preconditions (not skips): no gate and no window maximum is decided by an fp32 rounding; nothing is left out
    zero, gap, ties = pd.bn_gate_margins(defn.z_pre, mag.z_pre, pool)
    assert zero >= 1.0 and gap >= 1.0, (zero, gap)
    assert ties == (expect_ties if expect_ties is not None else 0), ties
    C = shape[3]
    g = torch.Generator(device=DEV).manual_seed(5)
    acc_g0, acc_b0 = torch.randn(C, device=DEV, generator=g), torch.randn(C, device=DEV, generator=g)
    acc_g, acc_b = acc_g0.clone(), acc_b0.clone()
    dy, dgamma, dbeta = native.bn_relu_pool_bwd(c["dz"], c["y"], c["mean"], c["invstd"], c["gamma"], c["beta"], pool, relu=relu,
                                                dgamma_acc=acc_g, dbeta_acc=acc_b,
                                                out_dtype=native.SPLIT_DTYPE if mode == "bf16x3" else None)
    tol_db, tol_dg, bnd = dc.bn_backward_bounds(defn, mag, c["gamma"], c["invstd"], out)
    label = f"bn bwd {shape} pool={int(pool)} relu={int(relu)} {mode}"
    dc.assert_channels_within(dbeta, defn.dbeta, tol_db, f"{label} dbeta")
    dc.assert_channels_within(dgamma, defn.dgamma, tol_dg, f"{label} dgamma")
    # the accumulators: one more fp32 add
    dc.assert_channels_within(acc_b, acc_b0.double() + defn.dbeta, tol_db + U * (acc_b0.double().abs() + defn.dbeta.abs()),
                              f"{label} dbeta_acc")
    dc.assert_channels_within(acc_g, acc_g0.double() + defn.dgamma, tol_dg + U * (acc_g0.double().abs() + defn.dgamma.abs()),
                              f"{label} dgamma_acc")
    dc.assert_matches_definition(_f32(native, dy), defn.dy, defn.dy.abs(), 1, mode, out=out, bnd=bnd, uniform=("block",), label=f"{label} dy")


@pytest.mark.parametrize("shape,mode", [p for p in BN_CASES if p.values[1] != "f16x3"])     # dy: the input type or bf16 pairs
def test_batchnorm_backward_matches_its_definition(native, shape, mode):
    """dbeta, dgamma (and their accumulators) per channel, dy per element; M counts the leftover pixels of odd maps.  gamma
    = 0 / 1e-20 without pooling; with pooling gamma = 0 is an exact tie and runs in the dedicated case below (1e-20 ties in
    fp32 but not in fp64, which the gap precondition rules out)."""
    for pool in (False, True):
        c = _dev(pc.bn_inputs(shape, _in_dtype(mode), pool, seed=3, degenerate_gamma=not pool))
        for relu in (True, False):
            _check_backward(native, c, shape, mode, pool, relu)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_batchnorm_backward_routes_a_tie_to_the_first_maximum(native, mode):
    """Exact duplicates of y inside windows, on channels of positive and of negative gamma, and a channel with gamma exactly
    0 (all four members tie): the whole gradient goes to the first maximum in the order (0,0), (0,1), (1,0), (1,1)."""
    shape = (2, 7, 9, 64)
    cpu = pc.bn_inputs(shape, _in_dtype(mode), True, seed=4, degenerate_gamma=False, ties=True)
    z, zmag = pd.bn_affine(cpu["y"], cpu["mean"], cpu["invstd"], cpu["gamma"], cpu["beta"])
    w4 = pd._windows(z)
    tied = (torch.topk(w4, 2, dim=0).values.diff(dim=0) == 0)[0]
    assert tied[..., cpu["gamma"] > 0].any() and tied[..., cpu["gamma"] < 0].any() and tied[..., cpu["gamma"] == 0].all()
    g0 = pd.route(cpu["dz"], z, True, True)[..., 1]                  # gamma = 0: dz at member (0,0) of every window, gated by beta > 0
    want = cpu["dz"][..., 1].double() * float(cpu["beta"][1] > 0)
    assert torch.equal(g0[:, 0:6:2, 0:8:2], want) and g0.abs().sum() == want.abs().sum()
    _check_backward(native, _dev(cpu), shape, mode, True, True, expect_ties=int(tied.sum()))


# ---- running statistics ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 9, 11, 64), (1, 120, 128, 72)])      # one launch (<= 64 statistics blocks) / two launches
@pytest.mark.parametrize("k", [1, 3])
def test_bn_finalize_running_statistics_match_the_closed_form(native, shape, k):
    """running_mean / running_var after k momentum updates against (1 - m)^k r0 + (1 - (1 - m)^k) s in fp64, s the mean / the
    UNBIASED variance of the stored convolution output.  Allowance: the statistics' own tolerance (definition_check.
    stats_tolerances: an fp32 sum of M values) carried through the update + 4 k u of the magnitudes (k rounded updates)."""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(C + H)
    x = (torch.randn(B, H, W, 64, generator=g) * 3.0 + 0.7).to(DEV)
    wp = native.pack_conv_weight(torch.randn(C, 64, 1, 1, generator=g).to(DEV) * 0.2, 64, native.F32)
    y, stats = native.conv_fwd(x, wp, None, C, 1, want_stats=True)
    M = B * H * W
    rm0, rv0 = torch.linspace(-1, 1, C).to(DEV), torch.linspace(0.5, 2, C).to(DEV)
    rm, rv = rm0.clone(), rv0.clone()
    nbt = torch.tensor(7, dtype=torch.int64, device=DEV)
    mean, invstd = native.bn_finalize(stats, M, C, rm, rv, 0.1, 1e-5, k, num_batches_tracked=nbt)
    assert int(nbt) == 7 + k
    d = y[..., :C].double()
    mu, var, inv, tol_mu, tol_var, tol_inv = dc.stats_tolerances(d, torch.zeros_like(d), 1e-5)
    m = float(torch.tensor(0.1, dtype=torch.float32))            # the momentum the kernel receives
    keep = (1.0 - m) ** k
    unb = var * M / (M - 1)
    label = f"bn_finalize {shape} k={k}"
    dc.assert_channels_within(mean, mu, tol_mu, f"{label} mean")
    dc.assert_channels_within(invstd, inv, tol_inv, f"{label} invstd")
    dc.assert_channels_within(rm, keep * rm0.double() + (1 - keep) * mu,
                              (1 - keep) * tol_mu + 4 * k * U * (rm0.double().abs() + mu.abs()), f"{label} running_mean")
    dc.assert_channels_within(rv, keep * rv0.double() + (1 - keep) * unb,
                              (1 - keep) * tol_var * M / (M - 1) + 4 * k * U * (rv0.double().abs() + unb), f"{label} running_var")


# ---- bias gradient ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("M,N,ld", [(1, 8, 8), (3, 70, 72), (257, 64, 64), (5003, 81, 88)])
def test_bias_grad_is_the_column_sum(native, M, N, ld, dtype):
    """sfod_bias_grad against the fp64 column sums (so far pinned only to itself): LAMBDA sqrt(M) u sum |dy| per column, + u
    |db| when accumulating; sliced (atomic) and deterministic form; the pad columns of ld hold large values nobody may read."""
    g = torch.Generator().manual_seed(M + N)
    dy = torch.randn(M, ld, generator=g)
    dy[:, N:] = 1.0e6
    dy = dy.to(dtype).to(DEV)
    defined, mag = pd.bias_grad(dy, N)
    db0 = torch.randn(N, generator=g).to(DEV)
    before = native.set_deterministic(False)
    try:
        for det in (False, True):
            native.set_deterministic(det)
            for accumulate in (False, True):
                db = db0.clone()
                native.bias_grad(dy, N, db, accumulate=accumulate)
                want = defined + db0.double() if accumulate else defined
                dc.assert_channels_within(db, want, dc.bias_grad_bound(mag, M, db0 if accumulate else None),
                                          f"bias_grad {(M, N, ld)} det={int(det)} acc={int(accumulate)}")
    finally:
        native.set_deterministic(before)


# ---- pointwise kernels, bit for bit ----------------------------------------------------------------------------------------
SPECIALS = [0.0, -0.0, 1e-40, -1e-40, float("inf"), -float("inf"), float("nan"), 1.5]       # +-0, denormals, +-inf, NaN
FLAT_SIZES = [1, 257, 1048576 + 3 * 256 + 5]     # vectors: one; more than a workgroup; past ew_grid's 4096 x 256 threads (fp32)


def _flat_inputs(nvec, dtype, seed):
    """three tensors of nvec vectors; the first 64 elements pair every special value of a with every one of b (and of y)."""
    n = nvec * (4 if dtype == torch.float32 else 8)
    g = torch.Generator().manual_seed(seed)
    a, b, y = (torch.randn(n, generator=g) for _ in range(3))
    k = min(n, 64)
    idx = torch.arange(k)
    s = torch.tensor(SPECIALS)
    a[:k], b[:k], y[:k] = s[idx % 8], s[(idx // 8) % 8], s[(idx // 8) % 8]
    if n > 64:
        a[64:72], b[64:72] = 1.5, s             # ordinary values against every special gate / addend
        y[64:72] = s
    return a.to(dtype), b.to(dtype), y.to(dtype)


def _same_bits(got, want, label):
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, want.dtype, got.shape, want.shape)
    it = torch.int32 if got.dtype == torch.float32 else torch.int16
    ok = (got.view(it) == want.view(it)) | (torch.isnan(got) & torch.isnan(want))
    if not ok.all():
        i = int(torch.nonzero(~ok.flatten())[0])
        raise AssertionError(f"{label}: {int((~ok).sum())} of {ok.numel()} elements differ; first at {i}: got "
                             f"{float(got.flatten()[i])!r}, want {float(want.flatten()[i])!r}")
    print(f"[bit for bit {label}] {ok.numel()} elements equal")


def _relu(v):
    """the ReLU all activation kernels compute: v > 0 ? v : +0 -- a NaN gives 0 (fmaxf drops it), -0 gives +0."""
    return torch.where(v > 0, v, torch.zeros_like(v))


FLAT_CASES = [pytest.param(n, dt, id=f"{n}-{str(dt)[6:]}") for n in FLAT_SIZES for dt in (torch.float32, torch.bfloat16)
              if n <= 4096 * 256 or dt == torch.float32]       # the wrapped grid-stride loop: fp32, 4 * (1048576 + 3 * 256 + 5) elements


@pytest.mark.parametrize("nvec,dtype", FLAT_CASES)
def test_flat_pointwise_kernels_bit_for_bit(native, nvec, dtype):
    """add_act (act 0 / 1), add_, act_bwd_ (act 1; act 2: the fp32 slope 0.2), add_act_bwd_, mul_mask_: each a single fp32
    operation, rounded once to bf16 (nearest even) in bf16 mode -- against torch on the CPU."""
    a, b, y = _flat_inputs(nvec, dtype, nvec)
    ad, bd, yd = a.to(DEV), b.to(DEV), y.to(DEV)
    af, bf = a.float(), b.float()
    tag = f"{nvec} vectors {str(dtype)[6:]}"
    s = af + bf
    _same_bits(native.add_act(ad, bd, act=0), s.to(dtype), f"add_act act=0 {tag}")
    _same_bits(native.add_act(ad, bd, act=1), _relu(s).to(dtype), f"add_act act=1 {tag}")
    _same_bits(native.add_(ad.clone(), bd), s.to(dtype), f"add_ {tag}")
    zero = torch.zeros_like(af)
    _same_bits(native.act_bwd_(ad.clone(), yd, 1), torch.where(y.float() > 0, af, zero).to(dtype), f"act_bwd_ act=1 {tag}")
    slope = torch.tensor(0.2, dtype=torch.float32)
    _same_bits(native.act_bwd_(ad.clone(), yd, 2), torch.where(y.float() > 0, af, slope * af).to(dtype), f"act_bwd_ act=2 {tag}")
    _same_bits(native.add_act_bwd_(ad.clone(), bd, yd), torch.where(y.float() > 0, s, zero).to(dtype), f"add_act_bwd_ {tag}")
    mask = (torch.rand(a.numel(), generator=torch.Generator().manual_seed(3)) < 0.7).to(torch.uint8)
    scale = float(torch.tensor(1.0 / 0.7, dtype=torch.float32))
    _same_bits(native.mul_mask_(ad.clone(), mask.to(DEV), scale),
               torch.where(mask.bool(), af * torch.tensor(scale, dtype=torch.float32), zero).to(dtype), f"mul_mask_ {tag}")


MAPS = [(2, 7, 9, 8), (1, 1, 1, 8), (1, 2, 1, 16), (1, 8, 6, 40)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", MAPS, ids=lambda s: "x".join(map(str, s)))
def test_spatial_pointwise_kernels_bit_for_bit(native, shape, dtype):
    """subsample2 (even pixels), its adjoint (every destination pixel written: the destination is prefilled with a sentinel)
    and maxpool3s2 (3x3, stride 2, pad 1; a NaN is dropped like in the ReLU kernels, -inf is an ordinary value)."""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(H * 10 + W)
    x = torch.randn(B, H, W, C, generator=g)
    flat = x.view(-1)
    k = min(flat.numel(), 8)
    flat[:k] = torch.tensor(SPECIALS)[:k]
    if flat.numel() > 100:
        flat[torch.randperm(flat.numel(), generator=g)[:12]] = torch.tensor(SPECIALS + SPECIALS[4:])[:12]
    x = x.to(dtype)
    xd = x.to(DEV)
    tag = f"{shape} {str(dtype)[6:]}"
    sub = x[:, ::2, ::2].contiguous()
    _same_bits(native.subsample2(xd), sub, f"subsample2 {tag}")
    dx = torch.full(shape, 777.0, dtype=dtype, device=DEV)
    native.call("sfod_subsample2", sub.to(DEV), dx, B, H, W, C, 1, native.dt_of(dx))
    want = torch.zeros(shape, dtype=dtype)
    want[:, ::2, ::2] = sub
    _same_bits(dx, want, f"subsample2_bwd {tag}")
    _same_bits(native.subsample2_bwd(sub.to(DEV), shape), want, f"subsample2_bwd wrapper {tag}")
    xn = torch.where(torch.isnan(x), torch.full_like(x, -float("inf")), x).float()
    mp = F.max_pool2d(xn.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous().to(dtype)
    _same_bits(native.maxpool3s2(xd), mp, f"maxpool3s2 {tag}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_relu_kernels_agree_on_nan_and_signed_zero(native, dtype):
    """BatchNorm + ReLU (plain, pooled, with residual) and the join's ReLU all give +0 for a NaN and for -0 (fmaxf(v, 0)), and
    their backward gates (y > 0) pass no gradient there: pinned; torch's relu would propagate the NaN."""
    C = 16
    one, zero = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    y = torch.full((1, 2, 2, C), -1.0)
    y[0, 0, 0] = torch.tensor(SPECIALS + [2.0, -2.0] * 4)          # one pixel of specials in a window of -1
    y = y.to(dtype).to(DEV)
    want = _relu(y.float()).to(dtype)
    _same_bits(native.bn_relu_pool_fwd(y, zero, one, one, zero, False), want, "bn relu, identity affine")
    _same_bits(native.bn_add_relu_fwd(y, zero, one, one, zero, torch.zeros_like(y)), want, "bn add relu, identity affine")
    _same_bits(native.add_act(y, torch.zeros_like(y), act=1), want, "add_act")
    pooled = native.bn_relu_pool_fwd(y, zero, one, one, zero, True)
    yn = torch.where(torch.isnan(y.float()), torch.full_like(y.float(), -float("inf")), y.float())
    _same_bits(pooled, _relu(yn.amax(dim=(1, 2), keepdim=True)).to(dtype), "bn relu pool: the NaN is dropped from the window")
