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
