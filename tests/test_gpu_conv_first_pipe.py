"""The first-layer kernel's pipelined tile loop (SFOD_F1_PIPE) and the student's apply pass by recomputation
(sfod_conv_first_bn_apply, SFOD_FIRST_APPLY_RECOMPUTE).

The contract of both is bit identity, so every comparison is ``torch.equal`` and the plain loop (knob 0) is the reference:
the pipelined loop keeps the MFMA order of every accumulator, the epilogue arithmetic and the statistics formulas, and the
recomputing apply pass runs ``k_bn_relu_pool_fwd``'s expression on accumulators that equal pass 1's y.  The shapes are the
places the loop can go wrong: exactly one full tile, less than a tile, ragged in both directions, a mix of full and ragged
tiles, and -- with the persistent grid capped (SFOD_F1_GRID) -- a workgroup walking 9 full tiles (steady state of the
pipeline), 18 tiles over 5 workgroups (uneven counts: some workgroups end a tile earlier) and a cap above the tile count.
"""
import pytest
import torch

from test_gpu_model import HOT_YAML

pytestmark = pytest.mark.gpu
DEV = "cuda"
COUT = 64
# (B, H, W), grid cap
CASES = [((1, 8, 32), 0), ((1, 7, 31), 0), ((2, 9, 33), 0), ((1, 17, 70), 0),
         ((2, 24, 96), 2), ((2, 24, 96), 5), ((2, 24, 96), 64)]
IDS = ["x".join(map(str, s)) + (f"-grid{g}" if g else "") for s, g in CASES]
SENTINEL = 12345.0
_cache = {}


def _operands(native, shape, mode):
    """seeded normal image (3 channels in one 8-channel group), weights with a per-channel spread of scales"""
    key = (shape, mode)
    if key not in _cache:
        B, H, W = shape
        g = torch.Generator().manual_seed(100 * H + W + B)
        x = torch.zeros(B, H, W, 8)
        x[..., :3] = torch.randn(B, H, W, 3, generator=g) * 50
        w = torch.randn(COUT, 3, 3, 3, generator=g) / 5 * torch.exp2(torch.linspace(-6, 6, COUT)).view(COUT, 1, 1, 1)
        bias = torch.randn(COUT, generator=g)
        gamma = torch.randn(COUT, generator=g)
        gamma[3], gamma[17], gamma[40], gamma[41] = 0.0, -2.5, 300.0, -300.0      # zero, negative, large
        beta = torch.randn(COUT, generator=g) * 0.5
        assert (gamma < 0).any() and (gamma > 0).any() and (beta < 0).any() and (beta > 0).any()
        dt = native.SPLIT_DTYPE if mode == "bf16x3" else native.SPLITH_DTYPE
        code = native.BF16X3 if mode == "bf16x3" else native.F16X3
        _cache[key] = dict(xd=native.cast(x.to(DEV), dt), wp=native.pack_conv_weight(w.to(DEV), 8, code),
                           bias=bias.to(DEV), gamma=gamma.to(DEV), beta=beta.to(DEV))
    return _cache[key]


def _launch(native, c, shape, y=None, stats=False, scale=None, shift=None, act=0):
    """sfod_conv_first_fused_ws on the first-layer kernel's own statistics layout -> (y, stats)"""
    B, H, W = shape
    st = None
    if stats:
        nblk = native.query("sfod_conv_first_stats_blocks", B, H, W)
        assert nblk == B * ((H + 7) // 8) * ((W + 31) // 32)
        st = torch.full((nblk * 2 * COUT + nblk,), SENTINEL, device=DEV)
    xd, wp = c["xd"], c["wp"]
    native.call("sfod_conv_first_fused_ws", xd, wp, native.wscale_of(wp), c["bias"], scale, shift, y, st, B, H, W, COUT, act,
                native.dt_of(xd))
    assert native.last_conv_kernel() == ("k_conv_first_x3<1>" if xd.dtype == native.SPLIT_DTYPE else "k_conv_first_x3<2>")
    return y, st


def _three_launches(native, c, shape, with_z):
    """statistics only; fp32 y + statistics; the teacher's affine pass (z pairs as raw bytes)"""
    B, H, W = shape
    _, st_only = _launch(native, c, shape, stats=True)
    y, st_y = _launch(native, c, shape, y=torch.full((B, H, W, COUT), SENTINEL, device=DEV), stats=True)
    out = dict(st_only=st_only, y=y, st_y=st_y)
    if with_z:
        rm, rv = torch.zeros(COUT, device=DEV), torch.ones(COUT, device=DEV)
        mean, invstd = native.bn_finalize(_as_stats(native, st_y, shape), B * H * W, COUT, rm, rv, 0.1, 1e-5)
        scale = c["gamma"] * invstd
        shift = c["beta"] - mean * scale
        z = torch.zeros(B, H, W, COUT, dtype=c["xd"].dtype, device=DEV)
        _launch(native, c, shape, y=z, scale=scale, shift=shift, act=1)
        out.update(z=z.view(torch.uint8), mean=mean, invstd=invstd)
    return out


def _as_stats(native, flat, shape):
    """the flat statistics buffer in the form bn_finalize takes (what conv_fwd returns: the tensor carrying its block count)"""
    B, H, W = shape
    nblk = native.query("sfod_conv_first_stats_blocks", B, H, W)
    st = flat.clone()
    st.nblk = nblk
    return st


def _with_knobs(native, pipe, grid, fn):
    native.set_conv_first_pipe(pipe)
    native.set_conv_first_grid(grid)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    finally:
        native.set_conv_first_pipe(1)
        native.set_conv_first_grid(0)


@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pipelined_loop_is_bit_identical_to_the_plain_loop(native, case, mode):
    shape, grid = case
    c = _operands(native, shape, mode)
    with_z = True       # (f16x3: the affine pass as well, beyond the statistics and y launches)
    old = _with_knobs(native, 0, grid, lambda: _three_launches(native, c, shape, with_z))
    new = _with_knobs(native, 1, grid, lambda: _three_launches(native, c, shape, with_z))
    # the plain loop itself: the store-free pass gives the storing pass's statistics, every block and count written
    assert torch.equal(old["st_only"], old["st_y"]) and not (old["st_y"] == SENTINEL).any()
    assert not (old["y"] == SENTINEL).any()
    for k in ("st_only", "st_y", "y", "z"):
        assert torch.equal(new[k], old[k]), f"{k}: {(new[k].float() - old[k].float()).abs().max().item():.3e}"
    # and the grid cap changes nothing either (uncapped plain loop)
    if grid:
        base = _with_knobs(native, 0, 0, lambda: _three_launches(native, c, shape, with_z))
        for k in ("st_only", "st_y", "y", "z"):
            assert torch.equal(new[k], base[k]), k


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_recomputed_apply_is_bit_identical_to_the_elementwise_pass(native, case):
    shape, grid = case
    B, H, W = shape
    c = _operands(native, shape, "bf16x3")
    ref = _with_knobs(native, 0, 0, lambda: _three_launches(native, c, shape, True))       # y of the plain loop
    mean, invstd = ref["mean"], ref["invstd"]
    want = native.bn_relu_pool_fwd(ref["y"], mean, invstd, c["gamma"], c["beta"], False, out_dtype=native.SPLIT_DTYPE)
    got = _with_knobs(native, 1, grid, lambda: native.conv_first_bn_apply(c["xd"], c["wp"], c["bias"], mean, invstd,
                                                                         c["gamma"], c["beta"]))
    assert native.last_conv_kernel() == "k_conv_first_x3<1>"
    assert got.dtype == native.SPLIT_DTYPE and got.shape == want.shape
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    zf = native.cast(got, torch.float32)
    assert (zf[..., 3] == zf[0, 0, 0, 3]).all()                 # gamma = 0: the channel is the constant relu(beta)
    assert (zf > 0).any() and (zf == 0).any()                   # a mixed ReLU mask


def test_query_refuses_what_the_kernel_does_not_reproduce(native):
    n = native

    def q(B=2, H=96, W=400, cin=8, cout=COUT, flags=0, dt=n.BF16X3, ydt=n.F32):
        return n.query("sfod_conv_first_bn_apply_supported", B, H, W, cin, cout, flags, dt, ydt)
    assert q() == 1
    assert q(B=8, H=600, W=1200) == 1                   # the benchmark's conv1_1
    assert q(cout=128) == 0 and q(cin=64) == 0 and q(cin=16) == 0
    assert q(flags=1) == 0 and q(flags=2) == 0 and q(flags=3) == 0       # pooled, no ReLU
    assert q(dt=n.F32) == 0 and q(dt=n.BF16) == 0 and q(dt=n.F16X3) == 0 and q(ydt=n.BF16) == 0
    assert q(B=0) == 0 and q(H=-1) == 0
    assert q(B=1, H=8, W=32) == 0                       # conv_fwd leaves so small a map to another kernel: y would differ
    try:
        n.set_conv_algo(1)
        assert q() == 0                                 # ... as it does when the generic kernel is forced
    finally:
        n.set_conv_algo(0)
    try:
        n.set_first_apply_recompute(0)
        assert q() == 0
    finally:
        n.set_first_apply_recompute(1)
    assert q() == 1


def _trunk(sfod, native, monkeypatch, knob):
    calls = [0]
    orig = native.conv_first_bn_apply

    def counted(*a, **k):
        calls[0] += 1
        return orig(*a, **k)
    monkeypatch.setattr(native, "conv_first_bn_apply", counted)
    native.set_first_apply_recompute(knob)
    # (the deep layers' tiny maps run the generic weight gradient, whose float atomics are ordered in deterministic mode only)
    prev = native.set_deterministic(True)
    try:
        cfg = sfod.config.setup_cfg(HOT_YAML, ["OUTPUT_DIR", "", "SFOD.COMPUTE_DTYPE", "bf16x3"])
        torch.manual_seed(5)
        bb = sfod.modeling.backbone_vgg.build_vgg_backbone(cfg, None).to(DEV).train()
        with torch.no_grad():       # a BatchNorm with negative, zero and large weights and both signs of bias
            bn = bb._plan[0][1]
            bn.weight.copy_(torch.randn(COUT, generator=torch.Generator().manual_seed(6)))
            bn.weight[5], bn.weight[9] = 0.0, 40.0
            bn.bias.copy_(torch.randn(COUT, generator=torch.Generator().manual_seed(7)) * 0.3)
        x = torch.randn(2, 3, 40, 72, generator=torch.Generator().manual_seed(3)).to(DEV)
        feats = bb(x)
        gr = torch.Generator().manual_seed(4)
        loss = sum((f * torch.randn(f.shape, generator=gr).to(DEV)).sum() for _, f in sorted(feats.items()))
        loss.backward()
        torch.cuda.synchronize()
    finally:
        native.set_first_apply_recompute(1)
        native.set_deterministic(prev)
        monkeypatch.setattr(native, "conv_first_bn_apply", orig)
    grads = {k: p.grad.clone() for k, p in bb.named_parameters() if p.grad is not None}
    return {k: f.detach().clone() for k, f in feats.items()}, grads, calls[0]


def test_trunk_does_not_depend_on_the_knob(sfod, native, monkeypatch):
    """VGG trunk alone, 2 x 40 x 72: every stage output and every parameter gradient bit for bit, knob 1 against knob 0"""
    f_new, g_new, n_new = _trunk(sfod, native, monkeypatch, 1)
    f_old, g_old, n_old = _trunk(sfod, native, monkeypatch, 0)
    assert (n_new, n_old) == (1, 0)
    assert f_new.keys() == f_old.keys() and len(f_new) == 5
    for k in f_old:
        assert torch.equal(f_new[k], f_old[k]), k
    assert g_new.keys() == g_old.keys() and "vgg0.0.weight" in g_new and "vgg0.1.weight" in g_new
    for k in g_old:
        assert torch.equal(g_new[k], g_old[k]), k
