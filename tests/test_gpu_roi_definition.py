"""ROIAlign forward and backward against its DEFINITION, per element (oracle/pointwise_definitions.py: separable
interpolation matrices from sample coordinates computed in fp32 in torchvision's written order, contracted in fp64; bound:
tests/helpers/definition_check.roi_align_bound).  The pair modes are compared with the definition on the pairs' exact values,
not with the fp32 kernel.  One wrong ROI, bin row, channel block or 8x8 gradient tile fails here; the whole-tensor gates of
tests/test_gpu_ops.py (1e-5 / 8e-3) let them through (tests/test_definition_checker.py plants them).

Inputs (tests/helpers/pointwise_cases.roi_set): ~300 ROIs on a 2 x 21 x 30 map at scale 1/16 -- inside, over every border,
tiny, zero-sized, outside, far larger than the map, padding rows, images in random order -- drawn so that no sample coordinate
is within 4 eps_c of a validity edge and no bin size is within 1e-4 of an integer (asserted; nothing is excluded).
Only the default kernels are tested (SFOD_ROI_BWD_ATOMIC / SFOD_ROI_CBLK / SFOD_ROI_NT are A/B switches read at load).
"""
import pytest
import torch

from helpers import definition_check as dc
from helpers import pointwise_cases as pc
from oracle import pointwise_definitions as pd

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
B, H, W = pc.ROI_MAP
SCALE = pc.ROI_SCALE
_cache = {}


def rois_and_matrices(n, pooled):
    """the ROI set (device) and its interpolation matrices for one pooled size, computed once; the preconditions asserted."""
    if ("rois", n) not in _cache:
        _cache["rois", n] = pc.roi_set(n).to(DEV)
    rois = _cache["rois", n]
    if (n, pooled) not in _cache:
        m = pd.roi_align_matrices(rois, H, W, pooled, SCALE)
        coord, binm = pd.roi_precondition_margins(m)
        assert float(coord.min()) >= 1.0 and float(binm.min()) >= 1e-4, (float(coord.min()), float(binm.min()))
        assert int((m.batch < 0).sum()) >= 2 and int(((m.grid_h == 0) & (m.batch >= 0)).sum()) >= 2      # padding, zero-sized
        _cache[n, pooled] = m
    return rois, _cache[n, pooled]


def features(native, C, mode, seed):
    """-> (the kernel's feature tensor, its exact values in fp32)."""
    g = torch.Generator().manual_seed(seed)
    f = (torch.randn(B, H, W, C, generator=g) + 0.3).to(DEV)
    if mode == "bf16":
        f = f.bfloat16()
        return f, f.float()
    if mode in ("bf16x3", "f16x3"):
        p = native.cast(f, native.SPLIT_DTYPE if mode == "bf16x3" else native.SPLITH_DTYPE)
        return p, native.cast(p, torch.float32)
    return f, f


# pooled 7 (the separable kernel): C = 8: workgroup clamped to 64 threads; 40: one channel block; 136: C > 128, not a multiple
# of 128 (one block); 256: 2 blocks; 512: 4 blocks.  Outside fp32 the 16-byte vector needs C % 8.
FWD7 = [(C, m) for C in (8, 40, 136, 256, 512) for m in ("fp32", "bf16")] + [(C, m) for C in (136, 256) for m in ("bf16x3", "f16x3")]


def _check_forward(native, pooled, C, mode):
    rois, m = rois_and_matrices(300, pooled)
    feat, exact = features(native, C, mode, C + pooled)
    got = native.roi_align_fwd(feat, rois, pooled, SCALE)
    got = native.cast(got, torch.float32) if native.is_pairs(got.dtype) else got
    (defined, mag), aux = pd.roi_align_forward(exact, m)
    R = rois.shape[0]
    assert (got[m.batch < 0] == 0).all(), "padding rows are zeros"
    dc.assert_matches_definition(got.view(R, pooled, pooled, C), defined, mag, aux.K, mode, out=mode,
                                 bnd=dc.roi_align_bound(defined, mag, aux, mode), label=f"roi_align fwd P={pooled} C={C}")


@pytest.mark.parametrize("C,mode", FWD7, ids=[f"{C}-{m}" for C, m in FWD7])
def test_roi_align_forward_separable_matches_its_definition(native, C, mode):
    _check_forward(native, 7, C, mode)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("pooled", [1, 4, 14])
def test_roi_align_forward_sample_by_sample_matches_its_definition(native, pooled, mode):
    _check_forward(native, pooled, 40, mode)


def _check_backward(native, n, pooled, C, mode, accumulate):
    rois, m = rois_and_matrices(n, pooled)
    g = torch.Generator().manual_seed(n + C + pooled)
    dout = torch.randn(n, pooled * pooled, C, generator=g).to(DEV)
    if mode == "bf16":
        dout = dout.bfloat16()
    dfeat0 = torch.randn(B, H, W, C, generator=g).to(DEV) if accumulate else torch.zeros(B, H, W, C, device=DEV)
    got = native.roi_align_bwd(dout, rois, (B, H, W, C), pooled, SCALE, dfeat=dfeat0.clone())
    (defined, mag), aux = pd.roi_align_backward(dout.view(n, pooled, pooled, C), m, B)
    bnd = dc.roi_align_bound(defined, mag, aux, "fp32")
    if accumulate:                                  # one more fp32 add, onto the map's earlier content
        defined, mag = defined + dfeat0.double(), mag + dfeat0.double().abs()
        bnd = bnd + U * mag
    dc.assert_matches_definition(got, defined, mag, aux.K, "fp32", bnd=bnd,
                                 label=f"roi_align bwd R={n} P={pooled} C={C} {mode} acc={int(accumulate)}")


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("C", [40, 264])            # 264: a second 256-channel slab with a tail
def test_roi_align_backward_tiled_matches_its_definition(native, C, mode):
    """the tiled gather (pooled 7), accumulating onto a non-zero gradient map."""
    _check_backward(native, 300, 7, C, mode, True)


def test_roi_align_backward_tiled_with_more_rois_than_one_pass_lists(native):
    """4500 ROIs: more than one 4096-ROI pass of the tile's list, many 256-ROI ballots per pass."""
    _check_backward(native, 4500, 7, 8, "fp32", False)


@pytest.mark.parametrize("pooled", [2, 4])
def test_roi_align_backward_atomic_matches_its_definition(native, pooled):
    """pooled != 7: the separable scatter with one atomic add per footprint pixel and channel."""
    _check_backward(native, 300, pooled, 40, "fp32", False)
