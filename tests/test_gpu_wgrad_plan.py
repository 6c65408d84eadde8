"""One launch per kind of weight-gradient plan (both halo-patch kernels on bf16, the three loops on operand pairs, the
generic kernel in every operand type, its wide form, its deterministic slabs, the first layer's fused form, a batch walked
in sub-batches with a remainder), on the smallest shape that reaches it: the kernel that ran is the one the plan names, it
stayed inside the sfod_conv_wgrad_ws_bytes bytes it was given, and dw equals the generic kernel's (sfod_set_conv_algo(1))."""
import math

import pytest
import torch

from test_gpu_first_wgrad_fused import _case as first_case, _fused as first_fused

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 1 << 16       # bytes behind the workspace
SENTINEL = 0xA5


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# Agreement of two kernels on the same operands, as the existing tests bound it for that pair:
def pair_bf16(M):     # bf16 operands, halo-patch vs exact products (test_gpu_ops.py: test_conv3x3_patch_wgrad)
    return 2e-5 * math.sqrt(M) / 10 + 1e-4
PAIR_X3 = 3e-5        # operand pairs, any two weight-gradient kernels (test_gpu_bf16x3.py: TOL in test_conv3x3_patch_wgrad and
#                       test_conv_dgrad_and_wgrad, whose algo 4 / 0 / 1 cases are the wide, the planner's and the generic kernel)
GEN_F32, GEN_BF16 = 3e-5, 8e-3      # the generic kernel against exact products (test_gpu_ops.py: test_conv_dgrad_and_wgrad)


@pytest.fixture
def guarded_ws(native, monkeypatch):
    """native's weight-gradient wrappers get their workspace from here: exactly the queried bytes, a sentinel-filled guard
    region behind them"""
    made = []

    def workspace(dev, nbytes):
        whole = torch.full((int(nbytes) + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
        made.append((whole, int(nbytes)))
        return whole[:int(nbytes)]

    monkeypatch.setattr(native, "_workspace", workspace)
    return made


def check_guard(made, extents, native):
    """the last launch got sfod_conv_wgrad_ws_bytes(extents) bytes, wrote into them and nowhere behind them"""
    whole, nbytes = made[-1]
    torch.cuda.synchronize()
    assert nbytes == native.query("sfod_conv_wgrad_ws_bytes", *extents) > 0
    assert (whole[nbytes:] == SENTINEL).all(), "the launch wrote behind the bytes sfod_conv_wgrad_ws_bytes announced"
    assert (whole[:nbytes] != SENTINEL).any(), "the workspace was not used"


def generic(native, fn):
    try:
        native.set_conv_algo(1)
        return fn()
    finally:
        native.set_conv_algo(0)


def smallest_side(native, cin, cout, dt):
    """the smallest square map (B = 1) whose 3x3 weight gradient the planner gives to the halo-patch kernel"""
    served = lambda s: native.query("sfod_conv_wgrad_oihw_supported", 1, s, s, cin, cout, 3, cout, dt)
    side = next(s for s in range(1, 200) if served(s))
    assert not served(side - 1)
    return side


def conv3_operands(native, dt, side, cin, cout, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(1, side, side, cin, device=DEV, generator=g)
    dy = torch.randn(1, side, side, cout, device=DEV, generator=g) * 1e-4       # gradient-sized values
    if dt == native.BF16:
        return x.bfloat16(), dy.bfloat16()
    return native.cast(x, native.SPLIT_DTYPE), native.cast(dy, native.SPLIT_DTYPE)


@pytest.mark.parametrize("cout,kernel", [(32, "k_wgrad3x3_patch<2,0,0>"), (96, "k_wgrad3x3_patch<4,0,0>")])
def test_halo_patch_plan_bf16(native, guarded_ws, cout, kernel):
    cin = 32
    side = smallest_side(native, cin, cout, native.BF16)
    x, dy = conv3_operands(native, native.BF16, side, cin, cout, cout)
    dw = native.conv_wgrad(x, dy, cout, 3)
    assert native.last_conv_kernel() == kernel, native.last_conv_kernel()
    check_guard(guarded_ws, (1, side, side, cin, cout, 3, cout, native.BF16), native)
    dw_gen = generic(native, lambda: native.conv_wgrad(x, dy, cout, 3))
    assert native.last_conv_kernel() == "k_conv_wgrad<bf16_t,2,2,0>" and len(guarded_ws) == 1      # no workspace asked for
    assert rel_err(dw, dw_gen) < pair_bf16(side * side)


X3_CASES = [(2, 64, "k_wgrad3x3_w64"), (2, 8, "k_wgrad3x3_patch<4,1,1>"), (1, 64, "k_wgrad3x3_patch<4,1,1>"),
            (0, 64, "k_wgrad3x3_patch<4,1,0>")]          # sfod_set_wgrad3x3_pipe, Cin -> the kernel


@pytest.fixture(scope="module")
def x3_reference(native):
    """the 3x3 bf16x3 layer of each case below once through the generic kernel: {(pipe, cin): (side, x, dy, dw)}; the map is
    the smallest the planner gives to the halo-patch kernel under that setting (128- or 256-pixel tiles)"""
    out = {}
    for pipe, cin, _ in X3_CASES:
        try:
            native.set_wgrad3x3_pipe(pipe)
            side = smallest_side(native, cin, 64, native.BF16X3)
        finally:
            native.set_wgrad3x3_pipe(2)
        x, dy = conv3_operands(native, native.BF16X3, side, cin, 64, cin + pipe)
        dw = generic(native, lambda: native.conv_wgrad(x, dy, 64, 3))
        assert native.last_conv_kernel() == "k_conv_wgrad<bf16_t,2,2,1>"
        out[pipe, cin] = (side, x, dy, dw)
    return out


@pytest.mark.parametrize("pipe,cin,kernel", X3_CASES)
def test_halo_patch_plan_bf16x3(native, guarded_ws, x3_reference, pipe, cin, kernel):
    side, x, dy, dw_gen = x3_reference[pipe, cin]
    try:
        native.set_wgrad3x3_pipe(pipe)
        dw = native.conv_wgrad(x, dy, 64, 3)
        assert native.last_conv_kernel() == kernel, native.last_conv_kernel()
        check_guard(guarded_ws, (1, side, side, cin, 64, 3, 64, native.BF16X3), native)
    finally:
        native.set_wgrad3x3_pipe(2)
    assert rel_err(dw, dw_gen) < PAIR_X3


def linear_operands(native, mode, M, K, N, seed):
    """a 1x1 layer with ragged tails in every direction -> x, dy as operands, the exact gradient of what they hold"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(M, 1, 1, K, device=DEV, generator=g)
    dy = torch.randn(M, 1, 1, N, device=DEV, generator=g) * 1e-4
    if mode == "bf16":
        x, dy = x.bfloat16(), dy.bfloat16()
    exact = (dy.double().view(M, N).t() @ x.double().view(M, K)).view(N, 1, K)
    if mode == "bf16x3":
        x, dy = native.cast(x, native.SPLIT_DTYPE), native.cast(dy, native.SPLIT_DTYPE)
    return x, dy, exact


@pytest.mark.parametrize("mode,kernel,tol", [("fp32", "k_conv_wgrad<float,2,2,0>", GEN_F32),
                                             ("bf16", "k_conv_wgrad<bf16_t,2,2,0>", GEN_BF16),
                                             ("bf16x3", "k_conv_wgrad<bf16_t,2,2,1>", PAIR_X3)])
def test_generic_plan(native, guarded_ws, mode, kernel, tol):
    M, K, N = 300, 200, 136
    x, dy, exact = linear_operands(native, mode, M, K, N, 6)
    assert native.query("sfod_conv_wgrad_ws_bytes", M, 1, 1, K, N, 1, N, native.dt_of(x)) == 0
    dw = native.conv_wgrad(x, dy, N, 1)
    assert native.last_conv_kernel() == kernel, native.last_conv_kernel()
    assert not guarded_ws                   # the query said 0: the entry point got a NULL workspace
    assert rel_err(dw, exact) < tol


def test_wide_plan(native, guarded_ws):
    M, K, N = 300, 264, 136
    x, dy, _ = linear_operands(native, "bf16x3", M, K, N, 7)
    dw_gen = native.conv_wgrad(x, dy, N, 1)
    assert native.last_conv_kernel() == "k_conv_wgrad<bf16_t,2,2,1>"       # the planner's own choice: four wide tiles only
    try:
        native.set_conv_algo(4)
        dw = native.conv_wgrad(x, dy, N, 1)
        assert native.last_conv_kernel() == "k_conv_wgrad_x3w"
        native.set_conv_algo(3)
        dw64 = native.conv_wgrad(x, dy, N, 1)
        assert native.last_conv_kernel() == "k_conv_wgrad<bf16_t,2,2,1>"
    finally:
        native.set_conv_algo(0)
    assert not guarded_ws
    assert rel_err(dw, dw_gen) < PAIR_X3 and rel_err(dw64, dw_gen) < PAIR_X3


def test_deterministic_plan(native, guarded_ws):
    M, K, N = 300, 200, 136
    x, dy, _ = linear_operands(native, "bf16x3", M, K, N, 6)
    extents = (M, 1, 1, K, N, 1, N, native.BF16X3)
    dw_atomic = native.conv_wgrad(x, dy, N, 1)
    prev = native.set_deterministic(True)
    try:
        nbytes = native.query("sfod_conv_wgrad_ws_bytes", *extents)
        assert nbytes > 0 and nbytes % (N * K * 4) == 0
        dw = native.conv_wgrad(x, dy, N, 1)
        assert native.last_conv_kernel() == "k_conv_wgrad<bf16_t,2,2,1>"
        check_guard(guarded_ws, extents, native)
        again = native.conv_wgrad(x, dy, N, 1)
        check_guard(guarded_ws, extents, native)
    finally:
        native.set_deterministic(prev)
    assert torch.equal(dw, again)
    # the slab sum ran: dw is the slabs of the workspace added in split order
    slabs = guarded_ws[-1][0][:nbytes].view(torch.float32).view(-1, N, 1, K)
    assert slabs.shape[0] > 1
    want = torch.zeros_like(dw)
    for s in slabs:
        want += s
    assert torch.equal(dw, want)
    assert rel_err(dw, dw_atomic) < PAIR_X3


def test_first_layer_fused_plan(native, guarded_ws):
    shape = (2, 17, 23)
    c = first_case(native, shape)
    n_before = len(guarded_ws)
    over = torch.full((64, 8, 3, 3), float("nan"), device=DEV)
    first_fused(native, c, over)                # asserts the kernel name: k_first_wgrad_bn
    assert len(guarded_ws) == n_before + 1
    native.set_conv_algo(2)                     # the setting the fused launch ran under
    try:
        check_guard(guarded_ws, (*shape, 8, 64, 3, 64, native.BF16X3), native)
    finally:
        native.set_conv_algo(0)
    assert torch.equal(over, c["ref_over"])


def test_sub_batches_with_a_remainder(native):
    """conv1_1 of nine 750 x 1333 frames: dy holds 2.3 GB, past the 32-bit byte offsets of the halo-patch kernel, which walks
    the batch as 5 + 4 images -- and the 4 want more slabs than the 5 (18 800 640 against 18 726 912 bytes).  The workspace
    query covers both, and the one call equals the two calls a caller could have made itself, bit for bit."""
    B, H, W, cin, cout, dt = 9, 750, 1333, 8, 64, native.BF16X3
    nb = 5
    g = torch.Generator(device=DEV).manual_seed(9)
    x = native.cast(torch.randn(B, H, W, cin, device=DEV, generator=g), native.SPLIT_DTYPE)
    dy = native.cast(torch.randn(B, H, W, cout, device=DEV, generator=g) * 1e-4, native.SPLIT_DTYPE)
    need = lambda n: native.query("sfod_conv_wgrad_ws_bytes", n, H, W, cin, cout, 3, cout, dt)
    assert need(B) == max(need(nb), need(B - nb)) and need(B - nb) > need(nb)

    def run(xs, dys, dw):
        n = xs.shape[0]
        whole = torch.full((need(n) + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
        native.call("sfod_conv_wgrad", xs, dys, dw, n, H, W, cin, cout, 3, cout, dt, whole, need(n))
        assert native.last_conv_kernel() == "k_wgrad3x3_patch<4,1,1>"
        torch.cuda.synchronize()
        assert (whole[need(n):] == SENTINEL).all(), "the launch wrote behind the bytes sfod_conv_wgrad_ws_bytes announced"

    dw = torch.zeros(cout, 9, cin, device=DEV)
    run(x, dy, dw)
    parts = torch.zeros(cout, 9, cin, device=DEV)
    run(x[:nb], dy[:nb], parts)
    run(x[nb:], dy[nb:], parts)
    assert dw.abs().max() > 0 and torch.equal(dw, parts)
