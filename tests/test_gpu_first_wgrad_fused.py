"""conv1_1's weight gradient with the BatchNorm-backward apply pass fused in (sfod_conv_first_wgrad_bn, k_first_wgrad_bn).

The contract is bit identity: the fused kernel forms every dy pair in registers with the expression and the (hi, lo) split of
``k_bn_bwd_apply<float, 0, 1, split_t>`` and sums the products in the order of ``k_wgrad3x3_patch<4, true, .>``, so its dw
must be ``torch.equal`` to ``bn_relu_pool_bwd`` (dy as bf16 pairs) followed by ``conv_wgrad_oihw`` / ``conv_wgrad`` on every
served shape, and both must meet the weight gradient's definition on that dy.  The shapes are the smallest that reach every
path of the tile walk: one tile with all four borders, odd sizes with tiles overhanging the map, interior tiles, several
images, and 300 tiles (more than the 256 pixel splits, so that a split walks two tiles and both patch buffers are used).
"""
import pytest
import torch

from helpers import definition_check as dc
from test_gpu_conv_definition import nhwc, wgrad_def
from test_gpu_model import HOT_YAML

pytestmark = pytest.mark.gpu
DEV = "cuda"
CIN, COUT = 8, 64
SHAPES = [(1, 16, 16), (2, 17, 23), (1, 40, 70), (3, 33, 64), (2, 96, 400)]
OLD_KERNEL, NEW_KERNEL = "k_wgrad3x3_patch<4,1,1>", "k_first_wgrad_bn"
_cache = {}


def _case(native, shape):
    """inputs and the two-launch results of one shape (computed once, shared by the tests below, never modified)"""
    if shape in _cache:
        return _cache[shape]
    B, H, W = shape
    g = torch.Generator(device=DEV).manual_seed(1000 * B + 10 * H + W)
    x = torch.randn(B, CIN, H, W, device=DEV, generator=g)
    x[:, 3:] = 0                                                    # three image channels in one 8-channel group
    y = torch.randn(B, H, W, COUT, device=DEV, generator=g) * 1.5 + 0.3
    dz = torch.randn(B, H, W, COUT, device=DEV, generator=g) * 1e-3
    mean = y.mean(dim=(0, 1, 2))
    invstd = torch.rsqrt(y.var(dim=(0, 1, 2), unbiased=False) + 1e-5)
    gamma = torch.randn(COUT, device=DEV, generator=g)              # both signs: the ReLU mask is mixed either way
    beta = torch.randn(COUT, device=DEV, generator=g) * 0.5
    assert (gamma > 0).any() and (gamma < 0).any()
    xd = native.cast(nhwc(x), native.SPLIT_DTYPE)
    sink0 = torch.randn(COUT, CIN, 3, 3, device=DEV, generator=g)   # a non-zero accumulator
    c = dict(x=x, xd=xd, y=y, dz=dz, bn=(mean, invstd, gamma, beta), sink0=sink0)
    native.set_conv_algo(2)         # the halo-patch kernel also where the planner would leave a tiny map to the generic one
    try:
        dy, dgamma, dbeta = native.bn_relu_pool_bwd(dz, y, mean, invstd, gamma, beta, False, out_dtype=native.SPLIT_DTYPE)
        ref = sink0.clone()
        native.conv_wgrad_oihw(xd, dy, ref, accumulate=True)
        assert native.last_conv_kernel() == OLD_KERNEL
        ref_over = torch.full((COUT, CIN, 3, 3), float("nan"), device=DEV)
        native.conv_wgrad_oihw(xd, dy, ref_over, accumulate=False)
        ref_packed = native.conv_wgrad(xd, dy, COUT, 3)
    finally:
        native.set_conv_algo(0)
    zp = (y - mean) * (invstd * gamma) + beta
    assert 0.2 < (zp > 0).float().mean().item() < 0.8               # a mixed ReLU mask
    c.update(dy=dy, dgamma=dgamma, dbeta=dbeta, ref=ref, ref_over=ref_over, ref_packed=ref_packed)
    _cache[shape] = c
    return c


def _fused(native, c, dw, **kw):
    """finalize-only BatchNorm backward, then the fused weight gradient into ``dw``"""
    mean, invstd, gamma, beta = c["bn"]
    native.set_conv_algo(2)
    try:
        none, dgamma, dbeta = native.bn_relu_pool_bwd(c["dz"], c["y"], mean, invstd, gamma, beta, False,
                                                      out_dtype=native.SPLIT_DTYPE, apply=False)
        assert none is None
        assert native.conv_first_wgrad_bn_supported(c["xd"], c["y"], COUT, False)
        native.conv_first_wgrad_bn(c["xd"], c["dz"], c["y"], mean, invstd, gamma, beta, dgamma, dbeta, dw, **kw)
        assert native.last_conv_kernel() == NEW_KERNEL
    finally:
        native.set_conv_algo(0)
    return dgamma, dbeta


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_dw_is_bit_identical_to_the_two_launches(native, shape):
    c = _case(native, shape)
    got = c["sink0"].clone()
    dgamma, dbeta = _fused(native, c, got, accumulate=True)
    # the same finalize on the same sums, with or without the apply pass
    assert torch.equal(dgamma, c["dgamma"]) and torch.equal(dbeta, c["dbeta"])
    assert torch.equal(got, c["ref"]), f"max |diff| {(got - c['ref']).abs().max().item():.3e}"
    again = c["sink0"].clone()
    _fused(native, c, again, accumulate=True)
    assert torch.equal(again, c["ref"])
    # overwrite form and the packed form (what conv_weight_grad uses for a [64, 3, 3, 3] parameter)
    over = torch.full((COUT, CIN, 3, 3), float("nan"), device=DEV)
    _fused(native, c, over)
    assert torch.equal(over, c["ref_over"])
    packed = torch.zeros(COUT, 9, CIN, device=DEV)
    _fused(native, c, packed)
    assert torch.equal(packed, c["ref_packed"])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_both_paths_match_the_definition_on_the_defined_dy(native, shape):
    """the bound of test_gpu_conv_definition.py::test_patch_wgrad_matches_its_definition, on dy as the apply pass defines it"""
    c = _case(native, shape)
    B, H, W = shape
    dy32 = native.cast(c["dy"], torch.float32).permute(0, 3, 1, 2).contiguous()
    defined, mag = wgrad_def(c["x"], dy32, 3, "bf16x3")
    got = torch.full((COUT, CIN, 3, 3), float("nan"), device=DEV)
    _fused(native, c, got)
    dc.assert_matches_definition(got, defined, mag, B * H * W, "bf16x3", layout="oihw", label=f"fused first wgrad {shape}")
    dc.assert_matches_definition(c["ref_over"], defined, mag, B * H * W, "bf16x3", layout="oihw",
                                 label=f"two-launch first wgrad {shape}")


def test_query_refuses_what_the_kernel_does_not_reproduce(native):
    n = native

    def q(B=2, H=96, W=400, cin=CIN, cout=COUT, flags=0, dt=n.BF16X3, ydt=n.F32):
        return n.query("sfod_conv_first_wgrad_bn_supported", B, H, W, cin, cout, flags, dt, ydt)
    assert q() == 1
    assert q(B=8, H=600, W=1200) == 1                   # the benchmark's conv1_1
    assert q(cout=128) == 0 and q(cin=64) == 0 and q(cin=16) == 0
    assert q(flags=1) == 0 and q(flags=2) == 0 and q(flags=3) == 0       # pooled, no ReLU
    assert q(dt=n.F32) == 0 and q(dt=n.BF16) == 0 and q(dt=n.F16X3) == 0 and q(ydt=n.BF16) == 0
    assert q(B=8, H=1024, W=2048) == 0                  # 4 GiB of dz: the two-launch path walks it in sub-batches
    assert q(B=0) == 0 and q(H=-1) == 0
    assert q(B=1, H=16, W=16) == 0                      # one tile: the planner leaves it to the generic kernel
    try:
        n.set_first_wgrad_fused(0)
        assert q() == 0
    finally:
        n.set_first_wgrad_fused(1)
    assert q() == 1


def _backbone_grads(sfod, native, monkeypatch, mode, knob, sink):
    calls = [0]
    orig = native.conv_first_weight_grad

    def counted(*a, **k):
        calls[0] += 1
        return orig(*a, **k)
    monkeypatch.setattr(native, "conv_first_weight_grad", counted)
    native.set_first_wgrad_fused(knob)
    # the deep layers' maps are a few pixels at this size: their weight gradients run the generic kernel, whose float atomics
    # arrive in another order every run.  Deterministic mode fixes that order, so any difference left is the knob's.
    prev = native.set_deterministic(True)
    try:
        cfg = sfod.config.setup_cfg(HOT_YAML, ["OUTPUT_DIR", "", "SFOD.COMPUTE_DTYPE", mode])
        torch.manual_seed(5)
        bb = sfod.modeling.backbone_vgg.build_vgg_backbone(cfg, None).to(DEV).train()
        if sink:        # gradients accumulate straight into the parameters' buffers (grad_sink), as under the trainer
            for p in bb.parameters():
                p.grad = torch.full_like(p, 0.125)
        x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(3)).to(DEV)
        feats = bb(x)
        gr = torch.Generator().manual_seed(4)
        loss = sum((f * torch.randn(f.shape, generator=gr).to(DEV)).sum() for _, f in sorted(feats.items()))
        loss.backward()
        torch.cuda.synchronize()
    finally:
        native.set_first_wgrad_fused(1)
        native.set_deterministic(prev)
        monkeypatch.setattr(native, "conv_first_weight_grad", orig)
    return {k: p.grad.clone() for k, p in bb.named_parameters() if p.grad is not None}, calls[0]


@pytest.mark.parametrize("sink", [False, True], ids=["autograd", "sink"])
@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
def test_backbone_gradients_do_not_depend_on_the_knob(sfod, native, monkeypatch, mode, sink):
    """VGG trunk alone, B = 2, 64 x 96: every parameter gradient (BatchNorm's included) bit for bit, knob 1 against knob 0"""
    new, n_new = _backbone_grads(sfod, native, monkeypatch, mode, 1, sink)
    old, n_old = _backbone_grads(sfod, native, monkeypatch, mode, 0, sink)
    assert (n_new, n_old) == (1, 0)
    assert new.keys() == old.keys() and "vgg0.0.weight" in new and "vgg0.1.weight" in new and "vgg0.1.bias" in new
    for k in old:
        assert torch.equal(new[k], old[k]), k


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_other_modes_keep_the_two_launch_path(sfod, native, monkeypatch, mode):
    grads, n = _backbone_grads(sfod, native, monkeypatch, mode, 1, False)
    assert n == 0
    assert all(torch.isfinite(g).all() for g in grads.values()) and grads["vgg0.0.weight"].abs().max() > 0
