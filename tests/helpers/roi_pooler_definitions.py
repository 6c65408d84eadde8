"""ROIAlign's definition under the pooler options (``sampling_ratio``, ``aligned``): the interpolation matrices of
oracle/pointwise_definitions.py with the two options, in the same namespace, so that ``pd.roi_align_forward``,
``pd.roi_align_backward``, ``pd.roi_precondition_margins`` and ``definition_check.roi_align_bound`` work on it unchanged.

    aligned=True:   start = coord * scale - 0.5, length = end - start                 (pd.roi_align_matrices)
    aligned=False:  start = coord * scale,       length = max(end - start, 1)
    sampling_ratio = 0: grid = ceil(length / pooled) per ROI and axis (pd._axis);  > 0: grid = sampling_ratio (_axis_fixed)

Sample coordinates in fp32 in torchvision's written order, one rounded op per step; weights summed in fp64.
Only tests/ import this module.
"""
import types

import torch

from oracle import pointwise_definitions as pd

U32 = 2.0 ** -24


def _axis_fixed(start, length, L, pooled, grid_n):
    """pd._axis with the grid of every ROI fixed at ``grid_n`` (its twin: pd._axis computes ceil(bin)); same returns."""
    f32 = torch.float32
    R, dev = start.shape[0], start.device
    P = torch.tensor(float(pooled), dtype=f32, device=dev)
    bin_ = length / P
    grid = torch.full((R,), int(grid_n), dtype=torch.long, device=dev)
    G = int(grid_n)
    p = torch.arange(pooled, dtype=f32, device=dev).view(1, -1, 1)
    i = torch.arange(G, dtype=f32, device=dev).view(1, 1, -1)
    gn = torch.tensor(float(grid_n), dtype=f32, device=dev)
    b3, s3 = bin_.view(-1, 1, 1), start.view(-1, 1, 1)
    t1 = p * b3
    t2 = s3 + t1
    t3 = (i + 0.5) * b3
    t4 = t3 / gn
    v = t2 + t4                                                              # [R, P, G] fp32
    valid = ~((v < -1.0) | (v > float(L)))
    c = torch.where(v <= 0, torch.zeros_like(v), v)
    lo = c.to(torch.long).clamp_max(10 * L + 10)
    edge = lo >= L - 1
    lo = torch.where(edge, torch.full_like(lo, L - 1), lo)
    hi = torch.where(edge, lo, lo + 1)
    c = torch.where(edge, lo.to(f32), c)
    lw = c - lo.to(f32)
    hw = 1.0 - lw
    vd = valid.double()
    eps = 4 * U32 * (v.double().abs() + 1.0) * vd
    lo, hi = torch.where(valid, lo, torch.zeros_like(lo)), torch.where(valid, hi, torch.zeros_like(hi))

    def scatter(wl, wh):
        out = torch.zeros(R, pooled, L, dtype=torch.float64, device=dev)
        out.scatter_add_(2, lo, wl)
        out.scatter_add_(2, hi, wh)
        return out

    A = scatter(hw.double() * vd, lw.double() * vd)
    S = scatter(vd, vd)
    E = scatter(eps, eps)
    return A, S, E, grid, v, valid, bin_


def roi_align_matrices_opt(rois, H, W, pooled, scale, sampling_ratio=0, aligned=True):
    """pd.roi_align_matrices' namespace for any (sampling_ratio, aligned); (0, True) returns tensors equal to it.
    More fields: ``clamped`` [R] (aligned=False: a raw length below 1 on either axis, so the clamp acts; else all False),
    ``sampling_ratio``, and ``start_h`` / ``start_w`` [R] fp32."""
    f32 = torch.float32
    r = rois.detach().to(f32)
    s = torch.tensor(scale, dtype=f32, device=r.device)
    off = torch.tensor(0.5 if aligned else 0.0, dtype=f32, device=r.device)
    one = torch.tensor(1.0, dtype=f32, device=r.device)
    x1, y1, x2, y2 = ((r[:, k] * s) - off for k in (1, 2, 3, 4))
    lw, lh = x2 - x1, y2 - y1
    clamped = torch.zeros_like(lw, dtype=torch.bool)
    if not aligned:
        clamped = (lw < 1.0) | (lh < 1.0)
        lw, lh = torch.maximum(lw, one), torch.maximum(lh, one)
    axis = (lambda st, ln, L: pd._axis(st, ln, L, pooled)) if sampling_ratio == 0 else \
        (lambda st, ln, L: _axis_fixed(st, ln, L, pooled, sampling_ratio))
    Ax, Sx, Ex, gw, vx, okx, bw = axis(x1, lw, W)
    Ay, Sy, Ey, gh, vy, oky, bh = axis(y1, lh, H)
    batch = r[:, 0].to(torch.long)
    batch = torch.where(r[:, 0] < 0, torch.full_like(batch, -1), batch)
    pad = (batch < 0).view(-1, 1, 1)
    Ay, Ax, Sy, Sx, Ey, Ex = (torch.where(pad, torch.zeros_like(t), t) for t in (Ay, Ax, Sy, Sx, Ey, Ex))
    count = (gh * gw).clamp_min(1).double()
    return types.SimpleNamespace(Ay=Ay, Ax=Ax, count=count, batch=batch, Sy=Sy, Sx=Sx, Ey=Ey, Ex=Ex, grid_h=gh, grid_w=gw,
                                 vy=vy, vx=vx, valid_y=oky, valid_x=okx, bin_h=bh, bin_w=bw, H=H, W=W, pooled=pooled,
                                 clamped=clamped & (batch >= 0), sampling_ratio=sampling_ratio, start_h=y1, start_w=x1)


def precondition_margins(m):
    """pd.roi_precondition_margins; with a fixed grid the bin-integer margin is void (the grid does not depend on the bin
    size): inf."""
    coord, binm = pd.roi_precondition_margins(m)
    if m.sampling_ratio > 0:
        binm = torch.full_like(binm, float("inf"))
    return coord, binm


def degenerate(m, aligned):
    """[R] bool: aligned=True: a live ROI whose adaptive grid ceil(bin) is 0 on an axis (zero-sized; under a fixed grid its
    samples all fall on one point); aligned=False: one whose raw length is below 1, so the clamp acts."""
    if not aligned:
        return m.clamped
    return ((torch.ceil(m.bin_h) <= 0) | (torch.ceil(m.bin_w) <= 0)) & (m.batch >= 0)


def vet(rois, H, W, pooled, scale, sampling_ratio, aligned, coord_min=1.0, bin_min=1e-4):
    """roi_set vets its preconditions for the default geometry only: recompute them for this combination and turn the
    offending rows into padding rows.  -> (rois, matrices of the vetted set, number of rows replaced)."""
    m = roi_align_matrices_opt(rois, H, W, pooled, scale, sampling_ratio, aligned)
    coord, binm = precondition_margins(m)
    bad = (coord < coord_min) | (binm < bin_min)
    n = int(bad.sum())
    if n:
        rois = rois.clone()
        rois[bad, 0] = -1.0
        m = roi_align_matrices_opt(rois, H, W, pooled, scale, sampling_ratio, aligned)
    return rois, m, n
