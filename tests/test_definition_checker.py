"""CPU self-test of tests/helpers/definition_check.py: faults planted in a result at layer-like size.

A correct result is the definition of the bf16x3 mode (oracle/split_precision.py) accumulated in fp32 -- what a kernel
computes.  Each planted fault must fail the per-element checker.  The relative-L2 gate the GPU suite applied before
(tests/test_gpu_bf16x3.py: 3e-5 against the exact fp64 product) passes the tile and halo-row faults: the gap the checker
closes.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from helpers import definition_check as dc
from oracle import split_precision as sp

OLD_TOL = 3e-5          # tests/test_gpu_bf16x3.py TOL


@pytest.fixture(scope="module")
def layer():
    """8 frames of 75 x 150, 16 -> 128 channels (one 256-pixel x 128-channel tile is 0.3 % of the output).  Frame 1 is frame
    0 under a small photometric change (two augmentations of one frame, as in a teacher / student batch)."""
    g = torch.Generator().manual_seed(7)
    B, Cin, H, W, Cout = 8, 16, 75, 150, 128
    x = torch.randn(B, Cin, H, W, generator=g) + 0.3
    x[1] = x[0] * (1 + 3e-3 * torch.randn(Cin, H, W, generator=g))
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    ts, _ = sp.terms(x, w, "bf16x3")
    got = sum(F.conv2d(a.float(), b.float(), padding=1) for a, b in ts)       # fp32 accumulation of the defined products
    defined = sp.conv2d(x, w, "bf16x3")
    return dict(x=x, w=w, got=got, defined=defined, mag=sp.magnitude(x, w), K=Cin * 9,
                exact=F.conv2d(x.double(), w.double(), padding=1))


def check(layer, got):
    return dc.assert_matches_definition(got, layer["defined"], layer["mag"], layer["K"], "bf16x3", layout="nchw",
                                        label="planted", quiet=True)


def old_gate_passes(layer, got):
    return dc.rel_err(got, layer["exact"]) < OLD_TOL


def test_the_correct_result_passes(layer):
    worst = check(layer, layer["got"])
    print(f"correct fp32-accumulated result: worst error / bound {worst:.3g}")
    assert worst < 0.25
    assert old_gate_passes(layer, layer["got"])


def test_one_element_off(layer):
    got = layer["got"].clone()
    got[5, 77, 40, 111] *= 1 + 1e-4
    with pytest.raises(AssertionError, match=r"1 of .* elements exceed the bound; worst at \(b, y, x, c\) = \(5, 40, 111, 77\)"):
        check(layer, got)


def test_one_tile_without_a_lo_cross_term_in_one_k_slice(layer):
    """One 256-pixel x 128-channel tile (16 x 16 pixels) that drops the lo(x) * hi(w) cross term of one K slice (one tap, the
    first 8 input channels)."""
    x, w = layer["x"], layer["w"]
    got = layer["got"].clone()
    b, y0, x0 = 3, 32, 64
    xs = x[b:b + 1, :, y0 - 1:y0 + 17, x0 - 1:x0 + 17]
    w1 = torch.zeros_like(w)
    w1[:, :8, 1, 2] = w[:, :8, 1, 2]
    _, _, (xl, wh) = sp.terms(xs, w1, "bf16x3")[0]
    lost = F.conv2d(xl, wh)
    got[b:b + 1, :, y0:y0 + 16, x0:x0 + 16] -= lost.float()
    assert old_gate_passes(layer, got), dc.rel_err(got, layer["exact"])
    with pytest.raises(AssertionError, match=r"worst at \(b, y, x, c\) = \(3, (3[2-9]|4[0-7]), (6[4-9]|7[0-9]), \d+\)"):
        check(layer, got)


def test_one_channel_with_a_truncated_split(layer):
    """Output channel 70's weights split with lo rounded toward zero instead of to nearest."""
    x, w = layer["x"], layer["w"]
    got = layer["got"].clone()
    wc = w[70:71].float()
    hi = wc.bfloat16().float()
    r = wc - hi
    lo_t = (r.view(torch.int32) & ~0xFFFF).view(torch.float32)                        # bf16 by truncation
    xh, xl = sp.split_pairs(x, "bf16")
    yc = F.conv2d(xh.float(), hi, padding=1) + F.conv2d(xh.float(), lo_t, padding=1) + F.conv2d(xl.float(), hi, padding=1)
    got[:, 70:71] = yc
    with pytest.raises(AssertionError, match="worst channel 70"):
        check(layer, got)


def test_one_halo_row_from_the_wrong_image(layer):
    """The top halo row of one tile of frame 1 read from frame 0 (its near copy): one output row of 16 pixels x 128 channels."""
    x, w = layer["x"], layer["w"]
    got = layer["got"].clone()
    y0, x0 = 48, 96
    xf = x[1:2].clone()
    xf[:, :, y0 - 1] = x[0, :, y0 - 1]
    row = sum(F.conv2d(a.float(), b.float(), padding=1) for a, b in sp.terms(xf, w, "bf16x3")[0])[:, :, y0, x0:x0 + 16]
    got[1:2, :, y0, x0:x0 + 16] = row
    assert old_gate_passes(layer, got), dc.rel_err(got, layer["exact"])
    with pytest.raises(AssertionError, match=r"worst at \(b, y, x, c\) = \(1, 48, (9[6-9]|10\d|11[01]), \d+\)"):
        check(layer, got)


def test_relu_outputs_and_batchnorm_statistics(layer):
    d, got = layer["defined"], layer["got"]
    v = d.permute(0, 2, 3, 1).reshape(-1, d.shape[1])
    mean, invstd = v.mean(0), torch.rsqrt(v.var(0, unbiased=False) + 1e-5)
    dc.assert_matches_definition(torch.relu(got), d, layer["mag"], layer["K"], "bf16x3", layout="nchw", relu=True,
                                 stats=(mean.float(), invstd.float(), 1e-5), quiet=True)
    bad = mean.clone()
    bad[9] += 2e-3 * float(v[:, 9].abs().mean())
    with pytest.raises(AssertionError, match="BatchNorm mean of 1 channels off; channel 9"):
        dc.assert_matches_definition(got, d, layer["mag"], layer["K"], "bf16x3", layout="nchw", stats=(bad, invstd, 1e-5),
                                     quiet=True)


# ---- the kernels between the convolutions: BatchNorm, ROIAlign, bias gradient -----------------------------------------------
# An honest fp32 evaluation -- plain torch in fp32 with the operations in another order than the fp64 definition
# (oracle/pointwise_definitions.py), for ROIAlign the C oracle -- must pass every bound: the bounds are not too tight, before
# anything runs on a GPU.  Each planted fault must fail.  Every docstring says whether the whole-tensor relative-L2 gate the
# GPU suite applied at the SAME shape (tests/test_gpu_ops.py: 3e-5 BatchNorm, 1e-5 ROIAlign, fp32) would have caught it; at
# layer size (2500 ROIs, 600 x 1200 frames) the same faults are 10 - 100 x more diluted.
from helpers import pointwise_cases as pc
from oracle import pointwise_definitions as pd
from oracle import roi_align as ora

OLD_BN, OLD_ROI = 3e-5, 1e-5
BN_SHAPE = (2, 7, 9, 64)


def _bn_fwd32(c, pool, gamma=None):
    """fp32, shift form: y * sc - (mean * sc - beta), then the window maximum and ReLU."""
    gamma = c["gamma"] if gamma is None else gamma
    sc = c["invstd"] * gamma
    z = c["y"].float() * sc - (c["mean"] * sc - c["beta"])
    if pool:
        B, H, W, C = z.shape
        z = z[:, :H // 2 * 2, :W // 2 * 2].reshape(B, H // 2, 2, W // 2, 2, C).amax(dim=(2, 4))
    return torch.relu(z)


@pytest.fixture(scope="module")
def bn_case():
    c = pc.bn_inputs(BN_SHAPE, torch.float32, True, seed=1)
    z, mag = pd.bn_affine(c["y"], c["mean"], c["invstd"], c["gamma"], c["beta"])
    c["defined"], c["mag"] = torch.relu(pd.pool2x2(z)), pd.pool2x2(mag)
    return c


def _bn_fwd_check(c, got):
    return dc.assert_matches_definition(got, c["defined"], c["mag"], 1, "fp32", bnd=dc.bn_forward_bound(c["defined"], c["mag"]),
                                        uniform=("block",), label="bn fwd", quiet=True)


def test_batchnorm_forward_in_fp32_passes(bn_case):
    """every shape of the GPU module; the bf16 one computes in fp32 from bf16 data and rounds the result once."""
    for shape, pool, dtype in ((BN_SHAPE, True, torch.float32), ((1, 8, 12, 72), False, torch.float32), ((1, 1, 1, 8), False, torch.float32),
                               ((1, 33, 37, 1024), False, torch.float32), ((1, 33, 37, 1024), True, torch.float32),
                               ((1, 5, 6, 2048), False, torch.bfloat16), ((1, 5, 6, 2048), True, torch.bfloat16)):
        c = pc.bn_inputs(shape, dtype, pool, seed=1)
        out = "bf16" if dtype == torch.bfloat16 else "fp32"
        z, mag = pd.bn_affine(c["y"], c["mean"], c["invstd"], c["gamma"], c["beta"])
        if pool:
            z, mag = pd.pool2x2(z), pd.pool2x2(mag)
        worst = dc.assert_matches_definition(_bn_fwd32(c, pool).to(dtype), torch.relu(z), mag, 1, out, out=out,
                                             bnd=dc.bn_forward_bound(torch.relu(z), mag, out), uniform=("block",), label=f"bn fwd {out} {shape}")
        assert worst <= 1.0


def test_batchnorm_forward_one_channel_vector_with_the_neighbours_gamma(bn_case):
    """8 channels of one pixel scaled with the next channel group's gamma.  At this shape (8064 outputs) the old 3e-5 gate
    catches it too; of a 75 x 150 x 128 layer output the same 8 values are 5e-6 of the elements."""
    c = bn_case
    g2 = c["gamma"].clone()
    g2[8:16] = c["gamma"][16:24]
    yb = dict(c, y=c["y"].clone())
    got = _bn_fwd32(c, True)
    wrong = _bn_fwd32(yb, True, gamma=g2)
    got[1, 2, 3, 8:16] = wrong[1, 2, 3, 8:16]
    assert dc.rel_err(got, c["defined"]) > OLD_BN
    with pytest.raises(AssertionError, match=r"worst at \(b, y, x, c\) = \(1, 2, 3, (8|9|1[0-5])\)"):
        _bn_fwd_check(c, got)


def test_batchnorm_forward_last_column_of_an_odd_pooled_map_not_covered(bn_case):
    """W = 9 pools to 4 columns; the last one is left unwritten (zeros).  The old gate catches a whole column at any size; it
    is here because the loop bound is where an odd size goes wrong."""
    c = bn_case
    got = _bn_fwd32(c, True)
    got[:, :, -1] = 0
    assert dc.rel_err(got, c["defined"]) > OLD_BN
    with pytest.raises(AssertionError, match=r"worst at \(b, y, x, c\) = \(\d, \d, 3, \d+\)"):
        _bn_fwd_check(c, got)


def _bn_bwd32(c, pool, relu, g=None, dgamma_loss=None):
    """fp32 backward in another order: dy = sc g - (sc / M) dbeta - (sc / M) xhat dgamma, sums by torch (pairwise)."""
    y, mean, invstd, gamma, beta = c["y"].float(), c["mean"], c["invstd"], c["gamma"], c["beta"]
    sc = invstd * gamma
    z = (y - mean) * sc + beta
    if g is None:
        g = pd.route(c["dz"], z, pool, relu).float()
    xhat = (y - mean) * invstd
    M = y.numel() // y.shape[-1]
    dbeta, dgamma = g.sum(dim=(0, 1, 2)), (g * xhat).sum(dim=(0, 1, 2))
    if dgamma_loss is not None:
        dgamma = dgamma - dgamma_loss
    k = sc / M
    return sc * g - k * dbeta - k * xhat * dgamma, dgamma, dbeta


def _bn_bwd_check(c, defn, mag, dy, dgamma, dbeta, out="fp32"):
    tol_db, tol_dg, bnd = dc.bn_backward_bounds(defn, mag, c["gamma"], c["invstd"], out)
    w = [dc.assert_channels_within(dbeta, defn.dbeta, tol_db, "dbeta"), dc.assert_channels_within(dgamma, defn.dgamma, tol_dg, "dgamma"),
         dc.assert_matches_definition(dy, defn.dy, defn.dy.abs(), 1, "fp32", bnd=bnd, uniform=("block",), label="bn bwd dy", quiet=True)]
    return max(w)


@pytest.fixture(scope="module")
def bn_bwd_case():
    c = pc.bn_inputs(BN_SHAPE, torch.float32, True, seed=3, degenerate_gamma=False)
    defn, mag = pd.bn_backward(c["dz"], c["y"], c["mean"], c["invstd"], c["gamma"], c["beta"], True, True)
    zero, gap, ties = pd.bn_gate_margins(defn.z_pre, mag.z_pre, True)
    assert zero >= 1 and gap >= 1 and ties == 0
    return c, defn, mag


def test_batchnorm_backward_in_fp32_passes(bn_bwd_case):
    c, defn, mag = bn_bwd_case
    assert _bn_bwd_check(c, defn, mag, *_bn_bwd32(c, True, True)) <= 1.0
    for shape, pool, relu in (((1, 8, 12, 72), False, True), ((2, 7, 9, 64), True, False), ((1, 1, 1, 8), True, True)):
        c2 = pc.bn_inputs(shape, torch.float32, pool, seed=3, degenerate_gamma=not pool)
        d2, m2 = pd.bn_backward(c2["dz"], c2["y"], c2["mean"], c2["invstd"], c2["gamma"], c2["beta"], pool, relu)
        assert _bn_bwd_check(c2, d2, m2, *_bn_bwd32(c2, pool, relu)) <= 1.0
    for shape, pool, dtype in (((1, 33, 37, 1024), False, torch.float32), ((1, 33, 37, 1024), True, torch.float32),
                               ((1, 5, 6, 2048), False, torch.bfloat16), ((1, 5, 6, 2048), True, torch.bfloat16)):
        c2 = pc.bn_inputs(shape, dtype, pool, seed=3, degenerate_gamma=not pool)
        d2, m2 = pd.bn_backward(c2["dz"], c2["y"], c2["mean"], c2["invstd"], c2["gamma"], c2["beta"], pool, True)
        dy, dg, db = _bn_bwd32(c2, pool, True)
        assert _bn_bwd_check(c2, d2, m2, dy.to(dtype), dg, db, out="bf16" if dtype == torch.bfloat16 else "fp32") <= 1.0
    t = pc.bn_inputs(BN_SHAPE, torch.float32, True, seed=4, degenerate_gamma=False, ties=True)       # exact ties: first maximum
    dt, mt = pd.bn_backward(t["dz"], t["y"], t["mean"], t["invstd"], t["gamma"], t["beta"], True, True)
    assert pd.bn_gate_margins(dt.z_pre, mt.z_pre, True)[2] > 100
    assert _bn_bwd_check(t, dt, mt, *_bn_bwd32(t, True, True)) <= 1.0


def test_batchnorm_backward_one_window_routed_to_the_second_maximum(bn_bwd_case):
    """The gradient of one window (one channel) goes to the second largest member.  Two wrong values of 8064: at this shape
    the old 3e-5 gate on dy catches it too; at layer size (2 of 10^8 values) it does not."""
    c, defn, mag = bn_bwd_case
    g = defn.g.float().clone()
    win = g[0, 2:4, 4:6, 5]
    zwin = defn.z_pre[0, 2:4, 4:6, 5]
    first, second = torch.topk(zwin.flatten(), 2).indices.tolist()
    assert win.flatten()[first] != 0
    v = win.flatten().clone()
    v[second], v[first] = v[first], 0.0
    g[0, 2:4, 4:6, 5] = v.view(2, 2)
    dy, dgamma, dbeta = _bn_bwd32(c, True, True, g=g)
    with pytest.raises(AssertionError):
        _bn_bwd_check(c, defn, mag, dy, dgamma, dbeta)
    dy_ok, dg_ok, db_ok = _bn_bwd32(c, True, True)
    dy_ok[0, 2:4, 4:6, 5] = dy[0, 2:4, 4:6, 5]                      # the routing alone, correct sums
    with pytest.raises(AssertionError, match=r"4 of 8064 elements exceed the bound; worst at \(b, y, x, c\) = \(0, [23], [45], 5\)"):
        _bn_bwd_check(c, defn, mag, dy_ok, dg_ok, db_ok)


def test_batchnorm_backward_one_leftover_pixel_without_gradient(bn_bwd_case):
    """dy = 0 at one pixel of the leftover row of the odd map (its true dy is the -dbeta / M - xhat dgamma / M part).  Old gate
    figure at this shape: 1.0e-2 -- above the fp32 gate (3e-5), below the bf16 one (2e-2), and it falls with the map size."""
    c, defn, mag = bn_bwd_case
    dy, dgamma, dbeta = _bn_bwd32(c, True, True)
    dy[1, 6, 2] = 0
    assert OLD_BN < dc.rel_err(dy, defn.dy) < 2e-2
    with pytest.raises(AssertionError, match=r"worst at \(b, y, x, c\) = \(1, 6, 2, \d+\)"):
        _bn_bwd_check(c, defn, mag, dy, dgamma, dbeta)


def test_batchnorm_backward_dgamma_misses_one_partial_row(bn_bwd_case):
    """dgamma of channel 9 without the partial sum of one workgroup's units (here: the first 8 windows); dy is computed from
    that dgamma, as the kernel's third pass would.  Old gate figures at this shape: 4e-2 on dgamma (caught: one of 64 channels),
    3.5e-4 on dy (caught in fp32, passed by the bf16 gate of 2e-2)."""
    c, defn, mag = bn_bwd_case
    part = (defn.g * defn.xhat)[0, :2, :, 9].sum().float()
    loss = torch.zeros(64)
    loss[9] = part
    dy, dgamma, dbeta = _bn_bwd32(c, True, True, dgamma_loss=loss)
    assert dc.rel_err(dgamma, defn.dgamma) > OLD_BN and OLD_BN < dc.rel_err(dy, defn.dy) < 2e-2
    with pytest.raises(AssertionError, match="dgamma: 1 of 64 channels exceed the bound; worst channel 9"):
        _bn_bwd_check(c, defn, mag, dy, dgamma, dbeta)


# ---- ROIAlign ----------------------------------------------------------------------------------------------------------------
ROI_C = 256


@pytest.fixture(scope="module")
def roi_case():
    B, H, W = pc.ROI_MAP
    rois = pc.roi_set(300)
    m = pd.roi_align_matrices(rois, H, W, 7, pc.ROI_SCALE)
    coord, binm = pd.roi_precondition_margins(m)
    assert float(coord.min()) >= 1.0 and float(binm.min()) >= 1e-4
    feat = torch.randn(B, H, W, ROI_C, generator=torch.Generator().manual_seed(11)) + 0.3
    (defined, mag), aux = pd.roi_align_forward(feat, m)
    real = m.batch >= 0
    got = torch.zeros(300, 7, 7, ROI_C)
    got[real] = ora.roi_align(feat.permute(0, 3, 1, 2).contiguous(), rois[real], 7, pc.ROI_SCALE).permute(0, 2, 3, 1)
    return dict(rois=rois, m=m, feat=feat, defined=defined, mag=mag, aux=aux, got=got, real=real,
                bnd=dc.roi_align_bound(defined, mag, aux))


def _roi_check(c, got):
    return dc.assert_matches_definition(got, c["defined"], c["mag"], c["aux"].K, "fp32", bnd=c["bnd"], label="roi fwd", quiet=True)


def test_roi_align_definition_is_the_slow_python_one():
    """the matrix formulation against oracle.roi_align.roi_align_py (double loops), tiny cases incl. the degenerate ROIs."""
    feat = torch.randn(2, 5, 6, 4, generator=torch.Generator().manual_seed(2))
    rois = torch.tensor([[0, 3.0, 2.0, 60.0, 50.0], [1, -20.0, -9.0, 30.0, 33.0], [0, 40.0, 40.0, 40.0, 40.0], [1, 200.0, 10.0, 260.0, 40.0],
                         [1, -300.0, -200.0, 500.0, 400.0], [0, 70.0, 50.0, 96.0, 80.0], [1, 10.0, 10.0, 12.5, 11.0]])
    for P in (1, 2, 7):
        (d, _), _ = pd.roi_align_forward(feat, pd.roi_align_matrices(rois, 5, 6, P, 1 / 16))
        ref = ora.roi_align_py(feat.permute(0, 3, 1, 2), rois, P, 1 / 16).permute(0, 2, 3, 1).double()
        assert (d - ref).abs().max() < 2e-6 * ref.abs().max()
        assert (d[2] == 0).all() and (d[3] == 0).all()


def test_roi_align_forward_of_the_c_oracle_passes(roi_case):
    worst = _roi_check(roi_case, roi_case["got"])
    print(f"C oracle (fp32): worst error / bound {worst:.3g}; old gate figure {dc.rel_err(roi_case['got'], roi_case['defined']):.3g}")
    assert worst <= 1.0


def _regular_roi(c, min_grid=2):
    m = c["m"]
    ok = c["real"] & (m.grid_h >= min_grid) & (m.grid_w >= min_grid) & (m.Ay.sum((1, 2)) > 6.5 * m.grid_h) & (m.Ax.sum((1, 2)) > 6.5 * m.grid_w)
    return int(torch.nonzero(ok)[0])


def test_roi_align_forward_one_sample_dropped(roi_case):
    """One of the grid_h x grid_w samples of one bin is not added: 256 values of 3.8 million.  With 300 ROIs the old 1e-5
    gate still catches it (1.5e-3); the error falls with the number of ROIs and with the grid size, the per-element ratio
    does not."""
    c, m = roi_case, roi_case["m"]
    r = _regular_roi(c)
    b = int(m.batch[r])
    yy, xx = float(m.vy[r, 3, 0]), float(m.vx[r, 2, 0])
    yl, xl = int(yy), int(xx)
    ly, lx = yy - yl, xx - xl
    f = c["feat"][b]
    s = (1 - ly) * (1 - lx) * f[yl, xl] + (1 - ly) * lx * f[yl, xl + 1] + ly * (1 - lx) * f[yl + 1, xl] + ly * lx * f[yl + 1, xl + 1]
    got = c["got"].clone()
    got[r, 3, 2] -= s / float(m.count[r])
    assert dc.rel_err(got, c["defined"]) > OLD_ROI
    with pytest.raises(AssertionError, match=rf"worst at \(b, y, x, c\) = \({r}, 3, 2, \d+\)"):
        _roi_check(c, got)


def test_roi_align_forward_one_roi_reads_the_other_image(roi_case):
    """One ROI of 300 pooled from the wrong image: the old gate catches it at 300 ROIs (1 / 300 of the output is wrong by
    100 %), and still at 2500."""
    c = roi_case
    r = _regular_roi(c)
    swapped = c["rois"][r:r + 1].clone()
    swapped[0, 0] = 1 - swapped[0, 0]
    got = c["got"].clone()
    got[r] = ora.roi_align(c["feat"].permute(0, 3, 1, 2).contiguous(), swapped, 7, pc.ROI_SCALE).permute(0, 2, 3, 1)[0]
    assert dc.rel_err(got, c["defined"]) > OLD_ROI
    with pytest.raises(AssertionError, match=rf"worst at \(b, y, x, c\) = \({r}, "):
        _roi_check(c, got)


def test_roi_align_forward_one_channel_block_unwritten(roi_case):
    """The second 128-channel block of one ROI left as zeros.  Caught by the old gate as well (a block is 100 % wrong)."""
    c = roi_case
    r = _regular_roi(c)
    got = c["got"].clone()
    got[r, :, :, 128:] = 0
    assert dc.rel_err(got, c["defined"]) > OLD_ROI
    with pytest.raises(AssertionError, match=rf"worst at \(b, y, x, c\) = \({r}, \d, \d, (12[89]|1[3-9]\d|2\d\d)\)"):
        _roi_check(c, got)


def test_roi_align_forward_count_off_by_one_grid_row(roi_case):
    """The ROI with the largest grid (26 rows) divided by (grid_h + 1) * grid_w: every value of that ROI off by 1 / 27.  Old
    gate figure 9e-5: caught by the fp32 gate (1e-5) at 300 ROIs, passed by the bf16 one (8e-3) and at 2500 ROIs close to it."""
    c, m = roi_case, roi_case["m"]
    r = int(torch.argmax(torch.where(c["real"], m.grid_h * m.grid_w, torch.zeros_like(m.grid_h))))
    gh = int(m.grid_h[r])
    got = c["got"].clone()
    got[r] *= gh / (gh + 1.0)
    assert OLD_ROI < dc.rel_err(got, c["defined"]) < 8e-3
    with pytest.raises(AssertionError, match=rf"worst at \(b, y, x, c\) = \({r}, "):
        _roi_check(c, got)


def _roi_bwd_case(n, C):
    B, H, W = pc.ROI_MAP
    rois = pc.roi_set(n)
    m = pd.roi_align_matrices(rois, H, W, 7, pc.ROI_SCALE)
    coord, binm = pd.roi_precondition_margins(m)
    assert float(coord.min()) >= 1.0 and float(binm.min()) >= 1e-4
    dout = torch.randn(n, 7, 7, C, generator=torch.Generator().manual_seed(n))
    (defined, mag), aux = pd.roi_align_backward(dout, m, B)
    real = m.batch >= 0
    x = torch.zeros(B, C, H, W, requires_grad=True)
    ora.roi_align(x, rois[real], 7, pc.ROI_SCALE).backward(dout[real].permute(0, 3, 1, 2).contiguous())
    return dict(rois=rois, m=m, dout=dout, defined=defined, mag=mag, aux=aux, got=x.grad.permute(0, 2, 3, 1).contiguous(), B=B,
                bnd=dc.roi_align_bound(defined, mag, aux))


def _roi_bwd_check(c, got):
    return dc.assert_matches_definition(got, c["defined"], c["mag"], c["aux"].K, "fp32", bnd=c["bnd"], label="roi bwd", quiet=True)


@pytest.fixture(scope="module")
def roi_bwd_4500():
    return _roi_bwd_case(4500, 8)


def test_roi_align_backward_of_the_c_oracle_passes(roi_bwd_4500):
    assert _roi_bwd_check(roi_bwd_4500, roi_bwd_4500["got"]) <= 1.0
    small = _roi_bwd_case(300, 8)
    assert _roi_bwd_check(small, small["got"]) <= 1.0


def test_roi_align_backward_one_tile_misses_a_segment_of_rois(roi_bwd_4500):
    """The 8 x 8 tile at (8, 8) of image 0 without the ROIs 1024 .. 2047.  The old 1e-5 gate catches a tile that loses a
    quarter of its sum at this size; the per-block check names the tile.  (k_roi_align_bwd_tiled itself lists ROIs in passes
    of 4096 and ballots of 256; there is no 1024-ROI unit in it -- the fault stands for any run of ROIs one tile loses, e.g.
    four ballots whose prefix offsets went wrong.)"""
    c = roi_bwd_4500
    part = c["dout"].clone()
    part[:1024] = 0
    part[2048:] = 0
    (lost, _), _ = pd.roi_align_backward(part, c["m"], c["B"])
    got = c["got"].clone()
    got[0, 8:16, 8:16] -= lost[0, 8:16, 8:16].float()
    assert dc.rel_err(got, c["defined"]) > OLD_ROI
    with pytest.raises(AssertionError, match=r"worst at \(b, y, x, c\) = \(0, (8|9|1[0-5]), (8|9|1[0-5]), \d\)"):
        _roi_bwd_check(c, got)


def test_roi_align_backward_one_roi_clipped_a_pixel_early_at_the_right_border():
    """One ROI that hangs over the right border does not reach the last column: its share of that column is missing.  Old
    gate figure 2.5e-2 at 300 ROIs (caught); it falls as more ROIs share the column."""
    c = _roi_bwd_case(300, 8)
    m = c["m"]
    W = m.W
    over = (m.batch >= 0) & (m.Ax[:, :, W - 1].sum(1) > 1.0) & (m.vx.amax(dim=(1, 2)) > W) & (m.grid_w < 8)
    r = int(torch.nonzero(over)[0])
    part = torch.zeros_like(c["dout"])
    part[r] = c["dout"][r]
    (lost, _), _ = pd.roi_align_backward(part, m, c["B"])
    got = c["got"].clone()
    got[:, :, W - 1] -= lost[:, :, W - 1].float()
    assert dc.rel_err(got, c["defined"]) > OLD_ROI
    with pytest.raises(AssertionError, match=rf"worst at \(b, y, x, c\) = \({int(m.batch[r])}, \d+, {W - 1}, \d\)"):
        _roi_bwd_check(c, got)


# ---- bias gradient -----------------------------------------------------------------------------------------------------------
def test_bias_grad_column_sums_and_a_dropped_tail():
    """fp32 column sums pass; a sum without the last M % 4 = 3 rows of 5003 fails (the kernel adds rows four at a time).
    No test compared sfod_bias_grad with a sum before: it was pinned to itself."""
    M, N, ld = 5003, 81, 88
    dy = torch.randn(M, ld, generator=torch.Generator().manual_seed(5))
    defined, mag = pd.bias_grad(dy, N)
    tol = dc.bias_grad_bound(mag, M)
    assert dc.assert_channels_within(dy[:, :N].sum(0), defined, tol, "bias_grad fp32") <= 1.0
    db0 = torch.randn(N)
    acc = db0 + dy[:, :N].t().contiguous().sum(1)
    assert dc.assert_channels_within(acc, defined + db0.double(), dc.bias_grad_bound(mag, M, db0), "bias_grad fp32 accumulate") <= 1.0
    with pytest.raises(AssertionError, match="channels exceed the bound"):
        dc.assert_channels_within(dy[:M - M % 4, :N].sum(0), defined, tol, "bias_grad without the tail")
