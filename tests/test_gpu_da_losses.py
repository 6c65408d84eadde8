"""The domain-loss kernels of csrc/da_losses.hip (``sfod_da_bce``, ``sfod_da_consistency_fwd`` / ``_bwd``) against the float64
definitions of tests/helpers/da_definitions.py (``pool="matrices"``: float64 throughout), gradients by autograd.

Tolerance as in tests/test_gpu_box_reg_options.py: nothing fixed in advance -- per compared quantity the same definition is also
evaluated by torch in fp32 and the gate is 4 x max(torch-fp32's distance from float64, 2^-24 * s), s = the sum of absolute
terms (a loss) or the largest magnitude (a gradient tensor).  The consistency cases assert a tie margin in float64 before
anything is compared: |p_img - p_ins| >= 1e-4 for every live ROI (SEED: the first seed from 1 upwards that keeps it for both
pooler settings).  No element is excluded.  Every case prints its figures; with SFOD_DA_REPORT=<file> they are appended there
(profiles/da_faster.txt holds such a run).
"""
import os

import pytest
import torch

from helpers import da_cases as C
from helpers import da_definitions as D

pytestmark = pytest.mark.gpu
DEV = "cuda"
LD = 8
SEED = 1
G_BCE, G_CONS = 0.7, 1.3            # upstream scales, not 1


def report(line):
    print(line)
    path = os.environ.get("SFOD_DA_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def column(z, ld=LD):
    """logits [..] -> fp32 [.., ld] with the values in column 0 and junk-free padding (what the GEMM writes under ldy)"""
    out = torch.zeros(*z.shape, ld, dtype=torch.float32)
    out[..., 0] = z.float()
    return out


def definition_bce(z, label, live, g):
    res = {}
    for dt in (torch.float64, torch.float32):
        zz = z.to(dt).clone().requires_grad_(True)
        loss, s = D.bce(zz, label, live)
        (grad,) = torch.autograd.grad(loss * g, zz)
        res[dt] = (loss.detach(), s.detach(), grad)
    return res


def check(label, what, dev, ref64, ref32, s):
    gate, e32 = D.gate(ref64, ref32, s)
    dist = (dev.double().cpu() - ref64).abs().max().item()
    report(f"{label}: {what} s={float(s):.6g} torch32={e32:.3e} device={dist:.3e} gate={gate:.3e}")
    assert dist <= gate, (label, what, dist, gate)


def run_bce(native, name, z, label, rois):
    """z [n] float64 holding fp32 values; rois [n, 5] or None"""
    live = (rois[:, 0] >= 0) if rois is not None else None
    res = definition_bce(z, label, live, G_BCE)
    zc = column(z).to(DEV)
    rd = rois.to(DEV) if rois is not None else None
    gs = torch.tensor([G_BCE], device=DEV)
    loss, dz = native.da_bce(zc, label, rois=rd, grad_scale=gs)
    loss_only, none = native.da_bce(zc, label, rois=rd)
    assert none is None and torch.equal(loss_only, loss)
    n_live = int(live.sum()) if live is not None else z.numel()
    assert loss[1].item() == n_live
    l64, s64, g64 = res[torch.float64]
    l32, _, g32 = res[torch.float32]
    check(name, "loss", loss[0], l64, l32, s64)
    check(name, "grad", dz[:, 0], g64, g32, g64.abs().max() if g64.numel() else 0.0)
    assert (dz[:, 1:] == 0).all()
    if live is not None:
        assert (dz[:, 0].cpu()[~live] == 0).all()
    return loss, dz


@pytest.mark.parametrize("label", [0.0, 1.0])
def test_bce_on_a_map_with_logits_spanning_the_log1p_branch(native, label):
    n = 2 * 5 * 7
    z = C.as_f32_values(C.hashed((n,), SEED, 30.0))
    z[:4] = torch.tensor([-30.0, 30.0, 0.0, -0.0], dtype=torch.float64)
    assert z.min() <= -29 and z.max() >= 29
    run_bce(native, f"bce map n={n} label={label:g}", z, label, None)


def masked_rows(n, pad):
    rois = torch.zeros(n, 5)
    rois[:, 0] = (torch.arange(n) % 2).float()
    rois[pad, 0] = -1.0
    return rois


@pytest.mark.parametrize("label", [0.0, 1.0])
def test_bce_masks_padding_rows(native, label):
    """80 rows: 4 padding rows at the tail and 6 at scattered positions; 300 rows (two blocks): every 7th row padding"""
    z = C.as_f32_values(C.hashed((80,), SEED + 1, 6.0))
    run_bce(native, f"bce rows n=80 pad=10 label={label:g}", z, label, masked_rows(80, [3, 17, 18, 40, 63, 70, 76, 77, 78, 79]))
    z = C.as_f32_values(C.hashed((300,), SEED + 2, 6.0))
    run_bce(native, f"bce rows n=300 label={label:g}", z, label, masked_rows(300, list(range(2, 300, 7))))


def test_bce_of_all_padding_rows_is_zero(native):
    z = C.as_f32_values(C.hashed((80,), SEED + 3, 6.0))
    loss, dz = run_bce(native, "bce rows n=80 all padding", z, 1.0, masked_rows(80, list(range(80))))
    assert loss[0].item() == 0.0 and loss[1].item() == 0.0 and (dz == 0).all()


# ---- consistency ---------------------------------------------------------------------------------------------------------------
def consistency_case(seed):
    B, Hf, Wf = C.MAP
    return {"z_img": C.as_f32_values(C.hashed((B, Hf, Wf), seed, 3.0)), "z_ins": C.as_f32_values(C.hashed((C.N_ROWS,), seed + 1, 3.0)),
            "rois": C.roi_rows(seed + 2)}


def definition_consistency(c, pooler, g):
    pooled, sr, aligned = pooler
    res = {}
    for dt in (torch.float64, torch.float32):
        zi, zn = c["z_img"].to(dt).clone().requires_grad_(True), c["z_ins"].to(dt).clone().requires_grad_(True)
        loss, s, d = D.consistency(zi, zn, c["rois"].to(dt), pooled, 1.0 / C.STRIDE, sr, aligned)
        gi, gn = torch.autograd.grad(loss * g, [zi, zn])
        res[dt] = (loss.detach(), s, d.detach(), gi, gn)
    return res


def test_seed_is_the_first_that_keeps_the_tie_margin():
    def keeps(seed):
        c = consistency_case(seed)
        return all(float(definition_consistency(c, p, 1.0)[torch.float64][2].abs().min()) >= 1e-4 for p in C.POOLERS)
    assert keeps(SEED) and not any(keeps(s) for s in range(1, SEED))


@pytest.mark.parametrize("pooler", C.POOLERS, ids=lambda p: "p{}-s{}-a{}".format(p[0], p[1], int(p[2])))
def test_consistency_forward_and_backward(native, pooler):
    pooled, sr, aligned = pooler
    c = consistency_case(SEED)
    rois = c["rois"]
    live = rois[:, 0] >= 0
    assert int(live.sum()) == 70 and set(rois[live, 0].tolist()) == {0.0, 1.0}
    res = definition_consistency(c, pooler, G_CONS)
    l64, s64, d64, gi64, gn64 = res[torch.float64]
    l32, _, d32, gi32, gn32 = res[torch.float32]
    margin = float(d64.abs().min())
    name = f"consistency pooled={pooled} sampling={sr} aligned={int(aligned)}"
    report(f"{name}: live={int(live.sum())} tie margin min|p_img - p_ins|={margin:.3e}")
    assert margin >= 1e-4
    zi, zn, rd = column(c["z_img"]).to(DEV), column(c["z_ins"]).to(DEV), rois.to(DEV)
    loss, st = native.da_consistency_fwd(zi, zn, rd, pooled, 1.0 / C.STRIDE, sampling_ratio=sr, aligned=aligned)
    assert loss[1].item() == 70
    check(name, "loss", loss[0], l64, l32, s64)
    # p_img of the live rows: against the definition's p_img = d + p_ins, a probability (s = 1)
    p64 = d64 + torch.sigmoid(c["z_ins"][live])
    p32 = d32.double() + torch.sigmoid(c["z_ins"][live].float()).double()
    check(name, "p_img", st["p_img"].cpu()[live], p64, p32, 1.0)
    assert (st["p_img"].cpu()[~live] == 0).all()
    assert torch.equal(st["sgn"][: C.N_ROWS].cpu()[live].double(), torch.sign(d64)) and (st["sgn"][: C.N_ROWS].cpu()[~live] == 0).all()
    assert st["p_img"][4].item() == 0.0 or not aligned          # x2 == x1 under the adaptive aligned grid pools nothing
    gs = torch.tensor([G_CONS], device=DEV)
    dzi, dzn = native.da_consistency_bwd(zi, zn, rd, st, gs)
    check(name, "dz_img", dzi[..., 0], gi64, gi32, gi64.abs().max())
    check(name, "dz_ins", dzn[:, 0], gn64, gn32, gn64.abs().max())
    assert (dzi[..., 1:] == 0).all() and (dzn[:, 1:] == 0).all() and (dzn[:, 0].cpu()[~live] == 0).all()
    assert float(gi64.abs().max()) > 0 and float(gn64.abs().max()) > 0
    # no float atomics: a second backward gives the same bits
    dzi2, dzn2 = native.da_consistency_bwd(zi, zn, rd, st, gs)
    assert torch.equal(dzi, dzi2) and torch.equal(dzn, dzn2)
    loss2, st2 = native.da_consistency_fwd(zi, zn, rd, pooled, 1.0 / C.STRIDE, sampling_ratio=sr, aligned=aligned)
    assert torch.equal(loss, loss2) and torch.equal(st["wts"], st2["wts"])


def test_consistency_without_a_live_roi_is_zero(native):
    c = consistency_case(SEED)
    rois = c["rois"].clone()
    rois[:, 0] = -1.0
    zi, zn, rd = column(c["z_img"]).to(DEV), column(c["z_ins"]).to(DEV), rois.to(DEV)
    loss, st = native.da_consistency_fwd(zi, zn, rd, 7, 1.0 / C.STRIDE)
    assert loss[0].item() == 0.0 and loss[1].item() == 0.0
    dzi, dzn = native.da_consistency_bwd(zi, zn, rd, st, torch.tensor([G_CONS], device=DEV))
    assert (dzi == 0).all() and (dzn == 0).all()
