"""Oracle (test infrastructure): fp64 definitions of the kernels between the convolutions -- BatchNorm (+ ReLU, + 2x2
max-pool) forward and backward, ROIAlign forward and backward, the bias gradient -- written with torch ops only, on CPU or
device tensors.  Like oracle/split_precision.py every function returns ``(defined, mag)`` in fp64: ``mag`` is the same
expression evaluated on absolute values, the scale of the fp32 rounding error of an honest kernel
(tests/helpers/definition_check.py turns it into a bound).  Only tests/ may import this module.

Activations are NHWC [B, H, W, C] (the kernels' layout); per-channel vectors are [C].
"""
import types

import torch

U32 = 2.0 ** -24


def _d(t):
    return t.detach().double()


# ---- BatchNorm ------------------------------------------------------------------------------------------------------
def bn_affine(y, mean, invstd, gamma, beta, residual=None):
    """z = (y - mean) * (invstd * gamma) + beta (+ residual); ReLU and the 2x2 max (floor sizes) are the caller's."""
    y, mean, invstd, gamma, beta = _d(y), _d(mean), _d(invstd), _d(gamma), _d(beta)
    sc = invstd * gamma
    z = (y - mean) * sc + beta
    mag = (y.abs() + mean.abs()) * sc.abs() + beta.abs()
    if residual is not None:
        z = z + _d(residual)
        mag = mag + _d(residual).abs()
    return z, mag


def pool2x2(z):
    """2x2 / 2 max over an NHWC tensor, floor sizes (H // 2 by W // 2); leftover pixels of odd H / W are not covered."""
    B, H, W, C = z.shape
    Ho, Wo = H // 2, W // 2
    if Ho == 0 or Wo == 0:
        return z.new_zeros(B, Ho, Wo, C)
    w = z[:, :2 * Ho, :2 * Wo].reshape(B, Ho, 2, Wo, 2, C)
    return w.amax(dim=(2, 4))


def _windows(t):
    """NHWC -> [4, B, Ho, Wo, C]: the window members in the order (0,0), (0,1), (1,0), (1,1)."""
    B, H, W, C = t.shape
    Ho, Wo = H // 2, W // 2
    w = t[:, :2 * Ho, :2 * Wo].reshape(B, Ho, 2, Wo, 2, C)
    return torch.stack([w[:, :, 0, :, 0], w[:, :, 0, :, 1], w[:, :, 1, :, 0], w[:, :, 1, :, 1]])


def _unwindows(w4, H, W):
    """inverse of _windows; pixels no window covers are 0."""
    _, B, Ho, Wo, C = w4.shape
    out = torch.zeros(B, H, W, C, dtype=w4.dtype, device=w4.device)
    v = out[:, :2 * Ho, :2 * Wo].view(B, Ho, 2, Wo, 2, C)
    v[:, :, 0, :, 0], v[:, :, 0, :, 1], v[:, :, 1, :, 0], v[:, :, 1, :, 1] = w4[0], w4[1], w4[2], w4[3]
    return out


def route(dz, z_pre, pool, relu):
    """g [B, H, W, C]: dz routed to the FIRST maximum of its 2x2 window in the order (0,0), (0,1), (1,0), (1,1) (pool) or to
    its own pixel, gated by z_pre > 0 at that maximum (relu).  Leftover pixels of odd H / W get 0."""
    dz, z_pre = _d(dz), _d(z_pre)
    if not pool:
        return torch.where(z_pre > 0, dz, torch.zeros_like(dz)) if relu else dz.clone()
    B, H, W, C = z_pre.shape
    w4 = _windows(z_pre)
    best, arg = w4[0].clone(), torch.zeros_like(w4[0], dtype=torch.long)
    for k in range(1, 4):
        gt = w4[k] > best                      # strictly greater: ties stay with the earlier member
        best = torch.where(gt, w4[k], best)
        arg = torch.where(gt, torch.full_like(arg, k), arg)
    gate = (best > 0) if relu else torch.ones_like(best, dtype=torch.bool)
    g4 = torch.stack([torch.where((arg == k) & gate, dz, torch.zeros_like(dz)) for k in range(4)])
    return _unwindows(g4, H, W)


def bn_backward(dz, y, mean, invstd, gamma, beta, pool, relu):
    """The formulas above bn_unit_grad (csrc/elementwise.hip):
        g = route(dz) ; dbeta = sum g ; dgamma = sum g * xhat ; dy = gamma * invstd * (g - dbeta / M - xhat * dgamma / M)
    with xhat = (y - mean) * invstd and M = B * H * W -- the leftover pixels of odd H / W included (their g is 0).
    -> (defined, mag): defined has dy, dgamma, dbeta, g, xhat, z_pre, M; mag has the absolute-value sums ``dbeta`` = sum |g|
    and ``dgamma`` = sum |g| |xhat| with |xhat| taken as (|y| + |mean|) * invstd (``xhat``), and ``z_pre`` (bn_affine's)."""
    z_pre, zmag = bn_affine(y, mean, invstd, gamma, beta)
    y, mean, invstd, gamma = _d(y), _d(mean), _d(invstd), _d(gamma)
    B, H, W, C = y.shape
    M = B * H * W
    g = route(dz, z_pre, pool, relu)
    xhat = (y - mean) * invstd
    xabs = (y.abs() + mean.abs()) * invstd.abs()
    dbeta = g.sum(dim=(0, 1, 2))
    dgamma = (g * xhat).sum(dim=(0, 1, 2))
    dy = gamma * invstd * (g - dbeta / M - xhat * dgamma / M)
    defined = types.SimpleNamespace(dy=dy, dgamma=dgamma, dbeta=dbeta, g=g, xhat=xhat, z_pre=z_pre, M=M)
    mag = types.SimpleNamespace(dbeta=g.abs().sum(dim=(0, 1, 2)), dgamma=(g.abs() * xabs).sum(dim=(0, 1, 2)), xhat=xabs,
                                z_pre=zmag)
    return defined, mag


def bn_gate_margins(z_pre, zmag, pool):
    """How far the discontinuous parts of the backward are from the data, in units of delta = 2^-12 * mag (4096 x the fp32
    error of z_pre): -> (min |z_pre| / delta, min over windows of (largest - second largest) / delta, inf without pool;
    exact ties -- bitwise equal z_pre -- are reported separately as their count)."""
    delta = 2.0 ** -12 * zmag
    zero = float((z_pre.abs() / delta.clamp_min(1e-300)).min())
    if not pool or z_pre.shape[1] < 2 or z_pre.shape[2] < 2:
        return zero, float("inf"), 0
    w4, d4 = _windows(z_pre), _windows(delta)
    top = torch.topk(w4, 2, dim=0).values
    gap = top[0] - top[1]
    ties = gap == 0
    ratio = gap / d4.amax(dim=0).clamp_min(1e-300)
    ratio = torch.where(ties, torch.full_like(ratio, float("inf")), ratio)
    return zero, float(ratio.min()), int(ties.sum())


# ---- ROIAlign (torchvision semantics, aligned=True, adaptive grid) --------------------------------------------------
def _axis(start, length, L, pooled):
    """One axis of every ROI.  start, length: fp32 [R].  The sample coordinates are computed in fp32 in torchvision's
    written order, one rounded op per step, no contraction; the interpolation weights are summed in fp64.
    -> A [R, P, L] weights, S [R, P, L] how many sample corners touch the pixel (the 0/1 support counted with multiplicity),
    E [R, P, L] the same weighted with each sample's coordinate allowance eps_c = 4u (|v| + 1), grid [R] (long),
    v [R, P, G] the coordinates, valid [R, P, G], bin [R]."""
    f32 = torch.float32
    R, dev = start.shape[0], start.device
    P = torch.tensor(float(pooled), dtype=f32, device=dev)
    bin_ = length / P
    grid = torch.ceil(bin_).to(torch.long)
    G = max(int(grid.max()) if R else 0, 1)
    p = torch.arange(pooled, dtype=f32, device=dev).view(1, -1, 1)
    i = torch.arange(G, dtype=f32, device=dev).view(1, 1, -1)
    gn = grid.clamp_min(1).to(f32).view(-1, 1, 1)
    b3, s3 = bin_.view(-1, 1, 1), start.view(-1, 1, 1)
    t1 = p * b3
    t2 = s3 + t1
    t3 = (i + 0.5) * b3
    t4 = t3 / gn
    v = t2 + t4                                                              # [R, P, G] fp32
    live = torch.arange(G, device=dev).view(1, 1, -1) < grid.view(-1, 1, 1)
    valid = live & ~((v < -1.0) | (v > float(L)))
    c = torch.where(v <= 0, torch.zeros_like(v), v)
    lo = c.to(torch.long).clamp_max(10 * L + 10)                             # (int) of a non-negative float: floor
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


def roi_align_matrices(rois, H, W, pooled, scale):
    """rois [R, 5] (batch index, x1, y1, x2, y2).  -> Ay [R, P, H], Ax [R, P, W], count [R], batch [R] (long; < 0: a padding
    row) and what the bound needs: Sy / Sx, Ey / Ex (see _axis), grid_h / grid_w, the coordinates and their validity.
        forward:  out[r, ph, pw, c] = sum_{py, px} Ay[r, ph, py] * Ax[r, pw, px] * feat[b_r, py, px, c] / count_r
    (the validity test of a sample factorises over the axes, so the sum over the grid does too)."""
    f32 = torch.float32
    r = rois.detach().to(f32)
    s = torch.tensor(scale, dtype=f32, device=r.device)
    half = torch.tensor(0.5, dtype=f32, device=r.device)
    x1, y1, x2, y2 = ((r[:, k] * s) - half for k in (1, 2, 3, 4))
    Ax, Sx, Ex, gw, vx, okx, bw = _axis(x1, x2 - x1, W, pooled)
    Ay, Sy, Ey, gh, vy, oky, bh = _axis(y1, y2 - y1, H, pooled)
    batch = r[:, 0].to(torch.long)
    batch = torch.where(r[:, 0] < 0, torch.full_like(batch, -1), batch)
    pad = (batch < 0).view(-1, 1, 1)
    Ay, Ax, Sy, Sx, Ey, Ex = (torch.where(pad, torch.zeros_like(t), t) for t in (Ay, Ax, Sy, Sx, Ey, Ex))
    count = (gh * gw).clamp_min(1).double()
    return types.SimpleNamespace(Ay=Ay, Ax=Ax, count=count, batch=batch, Sy=Sy, Sx=Sx, Ey=Ey, Ex=Ex, grid_h=gh, grid_w=gw,
                                 vy=vy, vx=vx, valid_y=oky, valid_x=okx, bin_h=bh, bin_w=bw, H=H, W=W, pooled=pooled)


def roi_precondition_margins(m):
    """The discontinuities of ROIAlign against the inputs, per ROI: -> (the smallest distance of a live sample coordinate from
    -1 or from H / W in units of 4 * eps_c, the smallest distance of roi_len / pooled from an integer), both [R], inf for
    padding rows.  An exactly zero-sized axis is left out of the second figure: its length is exactly 0 however the
    expression is contracted, so its grid is 0."""
    R = m.batch.shape[0]
    inf = torch.full((R,), float("inf"), dtype=torch.float64, device=m.batch.device)
    coord, binm = inf.clone(), inf.clone()
    for v, grid, L, bin_ in ((m.vy, m.grid_h, m.H, m.bin_h), (m.vx, m.grid_w, m.W, m.bin_w)):
        live = torch.arange(v.shape[2], device=v.device).view(1, 1, -1) < grid.view(-1, 1, 1)
        vd = v.double()
        dist = torch.minimum((vd + 1.0).abs(), (vd - L).abs()) / (16 * U32 * (vd.abs() + 1.0))
        dist = torch.where(live.expand_as(dist), dist, torch.full_like(dist, float("inf")))
        coord = torch.minimum(coord, dist.amin(dim=(1, 2)))
        b = bin_.double()
        binm = torch.minimum(binm, torch.where(b == 0, inf, (b - b.round()).abs()))
    pad = m.batch < 0
    return torch.where(pad, inf, coord), torch.where(pad, inf, binm)


def _per_image(m, B, fn):
    for b in range(B):
        rows = torch.nonzero(m.batch == b).flatten()
        if rows.numel():
            fn(b, rows)


def _fwd(My, Mx, feat, m, out):
    def one(b, rows):
        t = torch.einsum("rph,hwc->rpwc", My[rows], feat[b])
        out[rows] += torch.einsum("rqw,rpwc->rpqc", Mx[rows], t)
    _per_image(m, feat.shape[0], one)


def _adj(My, Mx, dout, m, out):
    def one(b, rows):
        t = torch.einsum("rqw,rpqc->rpwc", Mx[rows], dout[rows])
        out[b] += torch.einsum("rph,rpwc->hwc", My[rows], t)
    _per_image(m, out.shape[0], one)


def roi_align_forward(feat, m):
    """feat [B, H, W, C] -> (defined, mag) [R, P, P, C] fp64, and the bound's other inputs: K [R, P, P, 1] = nnz(Ay row) *
    nnz(Ax row), coord [R, P, P, C] = sum over the bin's samples of (eps_y + eps_x) * (|f11| + |f12| + |f21| + |f22|) / count,
    gsum [R, 1, 1, 1] = grid_h + grid_w.  Padding rows are zeros."""
    f = _d(feat)
    R, P, C = m.Ay.shape[0], m.pooled, f.shape[-1]
    z = lambda: torch.zeros(R, P, P, C, dtype=torch.float64, device=f.device)
    out, mag, coord = z(), z(), z()
    inv = (1.0 / m.count).view(-1, 1, 1, 1)
    _fwd(m.Ay, m.Ax, f, m, out)
    _fwd(m.Ay, m.Ax, f.abs(), m, mag)
    _fwd(m.Ey, m.Sx, f.abs(), m, coord)
    _fwd(m.Sy, m.Ex, f.abs(), m, coord)
    K = ((m.Ay != 0).sum(2).view(R, P, 1, 1) * (m.Ax != 0).sum(2).view(R, 1, P, 1)).double()
    gsum = (m.grid_h + m.grid_w).double().view(-1, 1, 1, 1)
    return (out * inv, mag * inv), types.SimpleNamespace(K=K, coord=coord * inv, gsum=gsum)


def roi_align_backward(dout, m, B):
    """dout [R, P, P, C] -> (defined, mag) [B, H, W, C] fp64: the adjoint of the forward (padding rows ignored), and K
    [B, H, W, 1] the adjoint of ones through the 0/1 support, coord the adjoint of the forward's coordinate allowance, gsum
    [B, H, W, 1] the largest grid_h + grid_w over the ROIs that touch the pixel."""
    g = _d(dout)
    C = g.shape[-1]
    inv = (1.0 / m.count).view(-1, 1, 1, 1)
    gi, ga = g * inv, g.abs() * inv
    z = lambda c=C: torch.zeros(B, m.H, m.W, c, dtype=torch.float64, device=g.device)
    out, mag, coord, K, gsum = z(), z(), z(), z(1), z(1)
    _adj(m.Ay, m.Ax, gi, m, out)
    _adj(m.Ay, m.Ax, ga, m, mag)
    _adj(m.Ey, m.Sx, ga, m, coord)
    _adj(m.Sy, m.Ex, ga, m, coord)
    ny, nx = (m.Ay != 0).double(), (m.Ax != 0).double()
    ones = torch.ones(g.shape[0], m.pooled, m.pooled, 1, dtype=torch.float64, device=g.device)
    _adj(ny, nx, ones, m, K)
    gs = (m.grid_h + m.grid_w).double()

    def one(b, rows):
        touch = ny[rows].amax(1).unsqueeze(2) * nx[rows].amax(1).unsqueeze(1)            # [r, H, W]
        gsum[b, :, :, 0] = (touch * gs[rows].view(-1, 1, 1)).amax(0)
    _per_image(m, B, one)
    return (out, mag), types.SimpleNamespace(K=K, coord=coord, gsum=gsum)


# ---- bias gradient --------------------------------------------------------------------------------------------------
def bias_grad(dy, n):
    """dy [M, ld] (the first n columns count) -> (column sums, column sums of |dy|) fp64."""
    d = _d(dy)[:, :n]
    return d.sum(0), d.abs().sum(0)
