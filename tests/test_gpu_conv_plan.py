"""One launch per kind of forward-convolution plan (first layer, halo patch, every tile of the generic kernel, the wide
tile, split-K), on the smallest shape that reaches it: the kernel that ran is the one the queries announced, it wrote
exactly sfod_conv_stats_blocks rows of BatchNorm statistics and nothing behind them, and its output equals the generic
kernel's (sfod_set_conv_algo(1), the planner's tile, no scratch)."""
import math

import pytest
import torch

from helpers import definition_check as dc

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096          # floats behind the statistics buffer


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# Agreement of two kernels on the same operands, as the existing tests bound it for that pair:
PAIR_BF16 = 4e-3      # bf16 outputs, first-layer / halo-patch vs generic kernel (test_gpu_ops.py: test_conv3x3_patch_kernel,
#                       test_conv_first_layer_kernel)
PAIR_X3 = 3e-5        # operand pairs, fp32 outputs, the same two pairs (test_gpu_bf16x3.py: TOL)
PAIR_TILES = 2e-6     # two tile shapes of the generic kernel: the same products in another fp32 summation order
#                       (test_gpu_bf16x3.py: test_gemm_tiles_with_64_byte_stages_equal_the_planners_choice)


@pytest.fixture
def guarded_stats(native, monkeypatch):
    """native.conv_fwd(want_stats=True) gets its statistics buffer from here: NaN-filled, with a guard region behind it"""
    made = []

    def stats_buffer(B, H, W, cin, cout, ksize, dt, dev):
        nb = native.query("sfod_conv_stats_blocks", B, H, W, cin, cout, ksize, dt)
        whole = torch.full((nb * (2 * cout + 1) + GUARD,), float("nan"), dtype=torch.float32, device=dev)
        stats = whole[:nb * (2 * cout + 1)]
        stats.nblk = nb
        made.append((whole, nb, cout, B * H * W))
        return stats

    monkeypatch.setattr(native, "_stats_buffer", stats_buffer)
    return made


def check_stats(made):
    whole, nb, cout, rows = made[-1]
    torch.cuda.synchronize()
    used = nb * (2 * cout + 1)
    assert nb > 0 and torch.isfinite(whole[:used]).all(), "a promised statistics row was not written"
    assert torch.isnan(whole[used:]).all(), "the launch wrote behind the rows sfod_conv_stats_blocks announced"
    assert float(whole[nb * 2 * cout:used].sum()) == rows          # the blocks' row counts


def generic(native, fn):
    """fn() on the generic kernel with the planner's tile"""
    try:
        native.set_conv_algo(1)
        native.set_gemm_tile(0)
        return fn()
    finally:
        native.set_conv_algo(0)


def conv3_operands(native, dt, B, H, W, Cin, Cout, seed, real=None):
    """real: channels that carry data (the first layer's 3 in a chunk of 8; the weight packer pads)"""
    g = torch.Generator().manual_seed(seed)
    real = real or Cin
    x = torch.zeros(B, H, W, Cin)
    x[..., :real] = torch.randn(B, H, W, real, generator=g) + 0.3
    w = torch.randn(Cout, real, 3, 3, generator=g) / math.sqrt(9 * real)
    bias = torch.randn(Cout, generator=g).to(DEV)
    if dt == native.BF16:
        return x.to(DEV).bfloat16(), native.pack_conv_weight(w.to(DEV), Cin, dt), bias
    return native.cast(x.to(DEV), native.SPLIT_DTYPE), native.pack_conv_weight(w.to(DEV), Cin, dt), bias


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_first_layer_plan(native, guarded_stats, mode):
    dt = native.BF16 if mode == "bf16" else native.BF16X3
    B, H, W, Cout = 1, 64, 64, 64
    assert native.query("sfod_conv_fwd_algo", B, H, W, 8, Cout, 3, dt) == 3
    assert native.query("sfod_conv_fwd_algo", B, H, W - 1, 8, Cout, 3, dt) != 3         # fewer than 4096 pixels: not served
    x, wp, bias = conv3_operands(native, dt, B, H, W, 8, Cout, 1, real=3)
    y, _ = native.conv_fwd(x, wp, bias, Cout, 3, want_stats=True)
    assert native.last_conv_kernel() == ("k_conv_first" if mode == "bf16" else "k_conv_first_x3<1>")
    check_stats(guarded_stats)
    y_gen = generic(native, lambda: native.conv_fwd(x, wp, bias, Cout, 3))
    assert native.last_conv_kernel().startswith("k_conv_fwd<")
    assert rel_err(y.float(), y_gen.float()) < (PAIR_BF16 if mode == "bf16" else PAIR_X3)


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_halo_patch_plan(native, guarded_stats, mode):
    dt, cin_phys, split = (native.BF16, 64, 0) if mode == "bf16" else (native.BF16X3, 128, 1)
    B, Cin, Cout = 1, 64, 64
    algo = lambda s: native.query("sfod_conv_fwd_algo", B, s, s, Cin, Cout, 3, dt)
    side = next(s for s in range(1, 200) if algo(s) == 2)         # the smallest square map with >= 8 tiles
    assert algo(side - 1) == 1
    x, wp, bias = conv3_operands(native, dt, B, side, side, Cin, Cout, 2)
    y, _ = native.conv_fwd(x, wp, bias, Cout, 3, act=1, want_stats=True)
    assert native.last_conv_kernel() == dc.expected_patch_kernel(3, cin_phys, split), native.last_conv_kernel()
    check_stats(guarded_stats)
    assert guarded_stats[-1][1] == native.query("sfod_conv_stats_blocks", B, side, side, Cin, Cout, 3, dt) >= 8
    y_gen = generic(native, lambda: native.conv_fwd(x, wp, bias, Cout, 3, act=1))
    assert native.last_conv_kernel().startswith("k_conv_fwd<")
    assert rel_err(y.float(), y_gen.float()) < (PAIR_BF16 if mode == "bf16" else PAIR_X3)


def linear_operands(native, M, K, N, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(M, K, device=DEV, generator=g)
    w = torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)
    bias = torch.randn(N, device=DEV, generator=g)
    return native.cast(x, native.SPLIT_DTYPE).view(M, 1, 1, -1), native.pack_fc_weight(w, native.BF16X3), bias, (x, w)


TILE_KERNELS = {1: (1, 2, 2, 128), 2: (2, 2, 2, 128), 3: (2, 4, 3, 128), 4: (1, 4, 3, 128),           # WN, WR, NST, BKB
                5: (4, 4, 3, 64), 6: (2, 4, 3, 64), 7: (2, 2, 3, 64), 8: (2, 4, 4, 64)}


@pytest.fixture(scope="module")
def tile_case(native):
    """one 1x1 layer for all eight tiles: ragged M / N / K tails, two tile rows of the tallest shape; the generic reference once"""
    M, K, N = 300, 200, 136
    x, wp, bias, _ = linear_operands(native, M, K, N, 3)
    y_gen = generic(native, lambda: native.conv_fwd(x, wp, bias, N, 1, act=1))
    return M, K, N, x, wp, bias, y_gen, native.last_conv_kernel()


@pytest.mark.parametrize("tile", sorted(TILE_KERNELS))
def test_generic_tile_plan(native, guarded_stats, tile_case, tile):
    M, K, N, x, wp, bias, y_gen, gen_kernel = tile_case
    wn, wr, nst, bkb = TILE_KERNELS[tile]
    try:
        native.set_gemm_tile(tile)
        assert native.query("sfod_conv_fwd_algo", M, 1, 1, K, N, 1, native.BF16X3) == (4 if tile == 5 else 1)
        y, _ = native.conv_fwd(x, wp, bias, N, 1, act=1, want_stats=True)
        assert native.last_conv_kernel() == f"k_conv_fwd<bf16_t,float,2,{wn},1,{wr},{nst},1,{bkb}>", native.last_conv_kernel()
    finally:
        native.set_gemm_tile(0)
    check_stats(guarded_stats)
    assert gen_kernel == "k_conv_fwd<bf16_t,float,2,2,1,2,2,1,128>"      # the planner's own choice here: 128 x 128
    assert rel_err(y, y_gen) < PAIR_TILES


def test_wide_tile_plan(native, guarded_stats):
    M, K, N = 12900, 264, 1000             # test_gpu_bf16x3.py::test_linear_wide_tile_kernel's first shape
    assert native.query("sfod_conv_fwd_algo", M, 1, 1, K, N, 1, native.BF16X3) == 4
    x, wp, bias, _ = linear_operands(native, M, K, N, 4)
    y, _ = native.conv_fwd(x, wp, bias, N, 1, want_stats=True)
    assert native.last_conv_kernel() == "k_conv_fwd<bf16_t,float,2,4,1,4,3,1,64>"
    check_stats(guarded_stats)
    y_gen = generic(native, lambda: native.conv_fwd(x, wp, bias, N, 1))
    assert rel_err(y, y_gen) < PAIR_TILES


def test_split_k_plan(native):
    """the ROI head's fc1 at one frame per GPU; statistics forbid the split form, so none are asked for"""
    M, K, N = 512, 25088, 1024
    lib = native.load()
    nbytes = lib.sfod_conv_fwd_scratch_bytes(M, 1, 1, K, N, 1, native.BF16X3, native.F32, 0)
    assert nbytes > 0 and lib.sfod_conv_fwd_scratch_bytes(M, 1, 1, K, N, 1, native.BF16X3, native.F32, 1) == 0
    x, wp, bias, (x32, w32) = linear_operands(native, M, K, N, 5)
    y = native.conv_fwd(x, wp, bias, N, 1, act=1)
    assert native.last_conv_kernel() == "k_conv_fwd<bf16_t,float,2,1,1,4,3,1,128>+k_splitk_sum"
    y_gen = torch.empty(M, N, device=DEV)
    generic(native, lambda: native.call("sfod_conv_fwd_ws", x, wp, native.wscale_of(wp), bias, y_gen, M, 1, 1, K, N, 1, N, 1,
                                        None, native.BF16X3, native.F32))
    assert native.last_conv_kernel() == "k_conv_fwd<bf16_t,float,2,1,1,4,3,1,128>"       # unsplit: the tall 256 x 64 tile
    torch.cuda.synchronize()
    # the bound of test_gpu_ops.py::test_linear_split_k_for_few_rows for this pair: K = 25088 products carry summation-order
    # noise of their own, measured on the unsplit kernel against fp64
    exact = torch.relu(x32.double() @ w32.double().t() + bias.double())
    err_gen = rel_err(y_gen, exact)
    assert rel_err(y.view(M, N), y_gen) < max(PAIR_TILES, 3 * err_gen), err_gen
