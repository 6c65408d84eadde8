"""The kernels of csrc/cda_condition.hip (``sfod_cda_condition_fwd`` / ``_bwd``, ``sfod_da_bce_weighted``) against the float64
definitions of tests/helpers/cda_definitions.py.

Tolerance: the rule of tests/test_gpu_da_losses.py -- per compared quantity the same definition is also evaluated by torch in
fp32 and the gate is 4 x max(torch-fp32's distance from float64, 2^-24 * s), s = 1 for the probabilities, 2 for the entropy
weights (their ranges), the largest magnitude for x / df / dz, the weighted sum of absolute terms for the loss.  x in bf16 or
an operand-pair type is compared after decoding, against the float64 product rounded by the type's rule
(oracle/split_precision.py: to fp32, then bf16 or (hi, lo)); torch's fp32 product goes through the same rule.  No element is
excluded.  ``sfod_da_bce`` itself (csrc/da_losses.hip) is untouched by this file's kernels: the weighted form is a kernel of
its own, so the old prototype's values are the parent's by construction and there is no dump to compare with.
"""
import functools

import pytest
import torch

from helpers import cda_cases as C
from helpers import cda_definitions as CD
from helpers import da_definitions as D
from oracle import split_precision as SP

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 11
TYPES = ("fp32", "bf16", "bf16x3", "f16x3")
G = 0.7            # upstream scale, not 1


def dtype_of(native, name):
    return {"fp32": torch.float32, "bf16": torch.bfloat16, "bf16x3": native.SPLIT_DTYPE, "f16x3": native.SPLITH_DTYPE}[name]


def rounded(v, name):
    """the values storage type ``name`` holds for ``v``: float64 -> fp32 -> the type's rule, as float64"""
    v = v.float()
    if name == "fp32":
        return v.double()
    if name == "bf16":
        return v.bfloat16().double()
    hi, lo = SP.split_pairs(v, SP.PAIR_FORMAT[name])
    return hi + lo


def to_device(native, v32, name):
    """fp32 CPU tensor -> device tensor of storage type ``name`` (pairs through sfod_cast)"""
    if name == "fp32":
        return v32.to(DEV)
    if name == "bf16":
        return v32.bfloat16().to(DEV)
    return native.cast(v32.to(DEV), dtype_of(native, name))


def decoded(native, t):
    return (native.cast(t, torch.float32) if native.is_pairs(t.dtype) else t.float()).double().cpu()


def check(label, what, dev, ref64, ref32, s):
    gate, e32 = D.gate(ref64, ref32, s)
    dist = (dev.double().cpu() - ref64).abs().max().item() if ref64.numel() else 0.0
    print(f"{label}: {what} s={float(s):.6g} torch32={e32:.3e} device={dist:.3e} gate={gate:.3e}")
    assert dist <= gate, (label, what, dist, gate)


@functools.lru_cache(maxsize=None)
def case(ncls, dim):
    """inputs of one shape and the definitions of p and w in float64 and fp32 (computed once, never modified)"""
    f = C.hashed((C.N_ROWS, dim), SEED + dim, 2.0).float()
    scores = C.scores(C.N_ROWS, ncls, SEED + ncls, nan_padding=True)
    rois = C.roi_rows(SEED + 2)
    live = rois[:, 0] >= 0
    assert list(torch.nonzero(~live).flatten()) == list(C.PAD_ROWS) and torch.isnan(scores[~live]).all()
    assert scores[0].unique().numel() == 1 and float(scores[1].max() - scores[1].median()) > 78 and float(scores[2].max()) > 79 > -79 > float(scores[2].min())
    res = {}
    for dt in (torch.float64, torch.float32):
        p = torch.zeros(C.N_ROWS, ncls, dtype=dt)
        p[live] = CD.condition(scores[live].to(dt))
        w = torch.zeros(C.N_ROWS, dtype=dt)
        w[live] = CD.entropy_weight(p[live])
        res[dt] = (p, w)
    assert (res[torch.float32][0][2] == 0).any()          # exact zeros of p in fp32: log(0 + 1e-5) is exercised
    return {"f": f, "scores": scores, "rois": rois, "live": live, "defs": res}


def x_definitions(c, f_vals, out_type):
    """x of the live rows' definition at full height, in float64 and as torch computes it in fp32, both under ``out_type``'s rule"""
    (p64, _), (p32, _) = c["defs"][torch.float64], c["defs"][torch.float32]
    x64 = rounded(CD.conditioned(f_vals, p64), out_type)
    x32 = rounded(CD.conditioned(f_vals.float(), p32), out_type)
    return x64, x32


@pytest.mark.parametrize("out_type", TYPES)
@pytest.mark.parametrize("shape", C.KERNEL_SHAPES, ids=lambda s: "C{}-D{}".format(*s))
def test_condition_forward(native, shape, out_type):
    ncls, dim = shape
    c = case(ncls, dim)
    live, rd, sd = c["live"], c["rois"].to(DEV), c["scores"].to(DEV)
    (p64, w64), (p32, w32) = c["defs"][torch.float64], c["defs"][torch.float32]
    for in_type in TYPES:
        name = f"condition C={ncls} D={dim} f={in_type} x={out_type}"
        f_vals = rounded(c["f"].double(), in_type)
        fd = to_device(native, c["f"], in_type)
        assert torch.equal(decoded(native, fd), f_vals)
        x, xg, p, w = native.cda_condition_fwd(fd, sd, ncls, rd, entropy=True, out_dtype=dtype_of(native, out_type),
                                               with_grad_operand=True)
        assert x.dtype == dtype_of(native, out_type) and tuple(x.shape) == (C.N_ROWS, ncls * dim)
        check(name, "p", p, p64, p32, 1.0)
        check(name, "w", w, w64, w32, 2.0)
        x64, x32 = x_definitions(c, f_vals, out_type)
        xd = decoded(native, x)
        check(name, "x", xd, x64, x32, x64.abs().max())
        # padding rows: exact zeros whatever their (NaN) logits hold
        assert (xd[~live] == 0).all() and (p.cpu()[~live] == 0).all() and (w.cpu()[~live] == 0).all()
        assert torch.isfinite(xd).all() and (w.cpu()[live] > 1).all()
        if out_type == "f16x3":      # the weight gradient's bf16 pairs, from the same registers
            assert xg.dtype == native.SPLIT_DTYPE and xg is not x
            g64, g32 = x_definitions(c, f_vals, "bf16x3")
            check(name, "x (bf16 pairs)", decoded(native, xg), g64, g32, g64.abs().max())
        else:
            assert xg is x
        # without the entropy switch the live weights are exactly 1, everything else the same bits
        x1, none, p1, w1 = native.cda_condition_fwd(fd, sd, ncls, rd, out_dtype=dtype_of(native, out_type))
        assert none is None and torch.equal(p1, p) and torch.equal(w1.cpu(), live.float())
        assert torch.equal(decoded(native, x1), xd)


def test_condition_reports_values_beyond_the_half_range(native):
    c = case(2, 8)
    f = c["f"].clone()
    f[0, 3] = 3.0e5                      # row 0: uniform p = 0.5 -> 1.5e5, beyond half's 65504
    rd, sd = c["rois"].to(DEV), c["scores"].to(DEV)
    native.check_f16x3_range(DEV)
    x, _, _, _ = native.cda_condition_fwd(f.to(DEV), sd, 2, rd, out_dtype=native.SPLIT_DTYPE)
    native.check_f16x3_range(DEV)        # bf16 pairs hold it: nothing to report
    assert decoded(native, x)[0, 3].item() == rounded(torch.tensor(1.5e5, dtype=torch.float64), "bf16x3").item()
    x, xg, _, _ = native.cda_condition_fwd(f.to(DEV), sd, 2, rd, out_dtype=native.SPLITH_DTYPE, with_grad_operand=True)
    assert decoded(native, x)[0, 3].item() == 65504.0 and decoded(native, x)[0, 8 + 3].item() == 65504.0
    assert decoded(native, xg)[0, 3].item() == rounded(torch.tensor(1.5e5, dtype=torch.float64), "bf16x3").item()
    with pytest.raises(FloatingPointError):
        native.check_f16x3_range(DEV)
    native.check_f16x3_range(DEV)        # the flag was cleared


@pytest.mark.parametrize("shape", C.KERNEL_SHAPES, ids=lambda s: "C{}-D{}".format(*s))
def test_condition_without_a_live_row_and_without_rows(native, shape):
    ncls, dim = shape
    c = case(ncls, dim)
    rois = c["rois"].clone()
    rois[:, 0] = -1.0
    for t in TYPES:
        x, xg, p, w = native.cda_condition_fwd(to_device(native, c["f"], t), c["scores"].to(DEV), ncls, rois.to(DEV), entropy=True,
                                               out_dtype=dtype_of(native, t), with_grad_operand=True)
        assert (decoded(native, x) == 0).all() and (decoded(native, xg) == 0).all() and (p == 0).all() and (w == 0).all()
        loss, dz = native.da_bce_weighted(torch.zeros(C.N_ROWS, 8, device=DEV), 1.0, w, rois=rois.to(DEV),
                                          grad_scale=torch.tensor([G], device=DEV))
        assert loss[0].item() == 0.0 and loss[1].item() == 0.0 and (dz == 0).all()
        df = native.cda_condition_bwd(torch.ones(C.N_ROWS, ncls * dim, device=DEV), p, rois.to(DEV))
        assert (df == 0).all()
        # R = 0: nothing is launched, empty outputs
        x, xg, p, w = native.cda_condition_fwd(to_device(native, c["f"][:0], t), c["scores"][:0].to(DEV), ncls, rois[:0].to(DEV),
                                               entropy=True, out_dtype=dtype_of(native, t), with_grad_operand=True)
        assert tuple(x.shape) == (0, ncls * dim) and tuple(p.shape) == (0, ncls) and tuple(w.shape) == (0,)
    df = native.cda_condition_bwd(torch.empty(0, ncls * dim, device=DEV), torch.empty(0, ncls, device=DEV), rois[:0].to(DEV))
    assert tuple(df.shape) == (0, dim)


def test_condition_refuses_bad_shapes(native):
    c = case(2, 8)
    rd, sd = c["rois"].to(DEV), c["scores"].to(DEV)
    with pytest.raises(native.NativeLibraryError, match="multiple of 8"):
        native.cda_condition_fwd(torch.zeros(C.N_ROWS, 12, device=DEV), sd, 2, rd)
    with pytest.raises(native.NativeLibraryError, match="C >= 2"):
        native.cda_condition_fwd(c["f"].to(DEV), sd, 1, rd)
    with pytest.raises(native.NativeLibraryError, match="ld"):
        native.cda_condition_fwd(c["f"].to(DEV), sd, 3, rd)                  # more classes than the score rows hold
    with pytest.raises(native.NativeLibraryError, match="fp32 or bf16"):
        native.cda_condition_bwd(native.cast(torch.zeros(C.N_ROWS, 16, device=DEV), native.SPLIT_DTYPE), torch.zeros(C.N_ROWS, 2, device=DEV), rd)


@pytest.mark.parametrize("dx_type", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", C.KERNEL_SHAPES, ids=lambda s: "C{}-D{}".format(*s))
def test_condition_backward(native, shape, dx_type):
    ncls, dim = shape
    c = case(ncls, dim)
    live, rd = c["live"], c["rois"].to(DEV)
    _, _, p, _ = native.cda_condition_fwd(c["f"].to(DEV), c["scores"].to(DEV), ncls, rd)
    dx_vals = rounded(C.hashed((C.N_ROWS, ncls * dim), SEED + 5, 3.0), dx_type)
    dx_vals[C.PAD_ROWS[0]] = float("nan")                # a padding row's gradient is never read
    dxd = to_device(native, dx_vals.float(), dx_type)
    pv = p.double().cpu()
    df = native.cda_condition_bwd(dxd, p, rd)
    assert df.dtype == dxd.dtype and tuple(df.shape) == (C.N_ROWS, dim)
    ref64 = torch.zeros(C.N_ROWS, dim, dtype=torch.float64)
    ref64[live] = CD.contraction(dx_vals[live], pv[live])
    ref32 = torch.zeros(C.N_ROWS, dim)
    ref32[live] = CD.contraction(dx_vals[live].float(), pv[live].float())
    check(f"condition bwd C={ncls} D={dim} {dx_type}", "df", df.float(), rounded(ref64, dx_type), rounded(ref32.double(), dx_type),
          ref64.abs().max())
    assert (df.float().cpu()[~live] == 0).all() and float(df.float().abs().max()) > 0
    # one owner per element, a fixed order: the same bits again
    assert torch.equal(native.cda_condition_bwd(dxd, p, rd), df)


# ---- the weighted BCE ------------------------------------------------------------------------------------------------------------
def run_weighted_bce(native, name, z, w, label, rois):
    """z, w [n] float64 holding fp32 values; rois [n, 5] or None"""
    live = (rois[:, 0] >= 0) if rois is not None else None
    res = {}
    for dt in (torch.float64, torch.float32):
        zz = z.to(dt).clone().requires_grad_(True)
        loss, s = CD.weighted_bce(zz, label, w.to(dt), live)
        (grad,) = torch.autograd.grad(loss * G, zz)
        res[dt] = (loss.detach(), s.detach(), grad)
    zc = torch.zeros(z.numel(), 8)
    zc[:, 0] = z.float()
    zc, wd = zc.to(DEV), w.float().to(DEV)
    rd = rois.to(DEV) if rois is not None else None
    loss, dz = native.da_bce_weighted(zc, label, wd, rois=rd, grad_scale=torch.tensor([G], device=DEV))
    loss_only, none = native.da_bce_weighted(zc, label, wd, rois=rd)
    assert none is None and torch.equal(loss_only, loss)
    assert loss[1].item() == (int(live.sum()) if live is not None else z.numel())
    l64, s64, g64 = res[torch.float64]
    l32, _, g32 = res[torch.float32]
    check(name, "loss", loss[0], l64, l32, s64)
    check(name, "grad", dz[:, 0], g64, g32, g64.abs().max())
    assert (dz[:, 1:] == 0).all()
    if live is not None:
        assert (dz[:, 0].cpu()[~live] == 0).all()
    loss2, dz2 = native.da_bce_weighted(zc, label, wd, rois=rd, grad_scale=torch.tensor([G], device=DEV))
    assert torch.equal(loss2, loss) and torch.equal(dz2, dz)
    return loss, dz


def masked_rows(n, pad):
    rois = torch.zeros(n, 5)
    rois[:, 0] = (torch.arange(n) % 2).float()
    rois[pad, 0] = -1.0
    return rois


@pytest.mark.parametrize("label", [0.0, 1.0])
def test_weighted_bce(native, label):
    """80 rows with the interleaved padding, entropy-like weights in (1, 2]; 300 rows (two blocks), every 7th padding, logits
    over the log1p branch; no mask at all"""
    z = C.as_f32_values(C.hashed((80,), SEED + 1, 6.0))
    w = C.as_f32_values(1.5 + 0.5 * C.hashed((80,), SEED + 2))
    run_weighted_bce(native, f"weighted bce n=80 label={label:g}", z, w, label, C.roi_rows(SEED + 2))
    z = C.as_f32_values(C.hashed((300,), SEED + 3, 30.0))
    w = C.as_f32_values(1.5 + 0.5 * C.hashed((300,), SEED + 4))
    run_weighted_bce(native, f"weighted bce n=300 label={label:g}", z, w, label, masked_rows(300, list(range(2, 300, 7))))
    run_weighted_bce(native, f"weighted bce n=300 unmasked label={label:g}", z, w, label, None)


def test_weighted_bce_with_equal_weights_is_the_plain_mean(native):
    """uniform p gives equal entropy weights: after the normalisation they are all 1 and the weighted loss is sfod_da_bce's,
    to the fp32 gate of the plain loss"""
    z = C.as_f32_values(C.hashed((80,), SEED + 1, 6.0))
    rois = C.roi_rows(SEED + 2)
    live = rois[:, 0] >= 0
    sd = torch.full((80, 9), 0.75, device=DEV)
    _, _, p, w = native.cda_condition_fwd(torch.zeros(80, 8, device=DEV), sd, 9, rois.to(DEV), entropy=True)
    assert w[live.to(DEV)].unique().numel() == 1 and torch.equal(p[live.to(DEV)], torch.full((70, 9), 1.0 / 9, device=DEV))
    zc = torch.zeros(80, 8)
    zc[:, 0] = z.float()
    gs = torch.tensor([G], device=DEV)
    lw, dzw = native.da_bce_weighted(zc.to(DEV), 1.0, w, rois=rois.to(DEV), grad_scale=gs)
    lp, dzp = native.da_bce(zc.to(DEV), 1.0, rois=rois.to(DEV), grad_scale=gs)
    l64, s64 = D.bce(z, 1.0, live)
    l32, _ = D.bce(z.float(), 1.0, live)
    check("equal weights", "weighted loss", lw[0], l64, l32, s64)
    check("equal weights", "plain loss", lp[0], l64, l32, s64)
    assert lw[1].item() == lp[1].item() == 70
    assert float((dzw - dzp).abs().max()) <= 4 * 2.0 ** -24 * float(dzp.abs().max())
