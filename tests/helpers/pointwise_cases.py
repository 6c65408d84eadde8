"""Inputs of the per-element checks of BatchNorm and ROIAlign (tests/test_definition_checker.py on the CPU,
tests/test_gpu_pointwise_definition.py and tests/test_gpu_roi_definition.py on the device): fixed seeds, nudged so that the
discontinuous parts of the operations (ReLU gate, window maximum, sample validity, adaptive grid size) are not decided by an
fp32 rounding.  The tests ASSERT those preconditions on the fp64 reference; nothing is excluded from a comparison."""
import torch

from oracle import pointwise_definitions as pd


# ---- BatchNorm ------------------------------------------------------------------------------------------------------
def bn_inputs(shape, dtype=torch.float32, pool=False, seed=0, degenerate_gamma=True, ties=False, residual=False):
    """-> dict of CPU tensors: y [B, H, W, C] (dtype), mean / invstd / gamma / beta [C] fp32 (free inputs: invstd in [0.05, 20]
    log-uniform, |mean| up to 10 x the data's spread, gamma of both signs and -- degenerate_gamma -- exactly 0 on channel 1 and
    1e-20 on channel 2), dz [B, Ho, Wo, C] (dtype), residual (dtype) or None.  y is nudged (then rounded to dtype) until every
    z_pre is >= 2 delta from 0 and, with pool, the two largest z_pre of every window are >= 2 delta apart (delta = 2^-12 mag).
    ties: afterwards the maximum of every other window is duplicated onto another member of the window (exact ties), and
    gamma is exactly 0 on channel 1 (all four members tie: the gradient goes to (0,0))."""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(1000 + seed)
    invstd = torch.exp(torch.empty(C).uniform_(-3.0, 3.0, generator=g)).clamp(0.05, 20.0)
    spread = 1.0 / invstd
    mean = torch.empty(C).uniform_(-10.0, 10.0, generator=g) * spread
    gamma = (0.3 + 1.7 * torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.4, -1.0, 1.0)
    gamma[0], gamma[3] = 1.25, -0.75
    if degenerate_gamma:
        gamma[1], gamma[2] = 0.0, 1e-20
    if ties:
        gamma[1] = 0.0               # z_pre = beta at every pixel, in fp32 and in fp64: every window of the channel is an exact tie
    beta = torch.randn(C, generator=g) * 0.5
    beta = torch.where(beta.abs() < 0.01, torch.full_like(beta, 0.25), beta)
    y = (mean + spread * torch.randn(B, H, W, C, generator=g)).to(dtype)
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    dz = torch.randn(B, Ho, Wo, C, generator=g).to(dtype)
    res = torch.randn(B, H, W, C, generator=g).to(dtype) if residual else None
    sc = (invstd * gamma).double()
    for _ in range(200):
        z, zmag = pd.bn_affine(y, mean, invstd, gamma, beta)
        delta = 2.0 ** -12 * zmag
        move = torch.zeros_like(z)                                   # desired change of z_pre, in units of its sign
        near0 = z.abs() < 2 * delta
        move = torch.where(near0, torch.where(z >= 0, 1.0, -1.0).double(), move)
        if pool and H >= 2 and W >= 2:
            w4, d4 = pd._windows(z), pd._windows(delta).amax(dim=0)
            top = torch.topk(w4, 2, dim=0)
            close = (top.values[0] - top.values[1]) < 2 * d4           # exact ties (bf16 data has them) too
            second = torch.zeros_like(w4).scatter_(0, top.indices[1:2], close.double().unsqueeze(0))
            move = torch.where(pd._unwindows(second, H, W) > 0, torch.full_like(move, -3.0), move)    # through the zero band
        move = torch.where(gamma.abs() < 1e-6, torch.zeros_like(move), move)      # z_pre does not depend on y there
        if not (move != 0).any():
            break
        step = 8 * delta / sc.abs().clamp_min(1e-300)
        if dtype == torch.bfloat16:
            step = torch.maximum(step, y.double().abs() * 2.0 ** -7)
        y = (y.double() + move * torch.sign(sc) * step).to(dtype)
    if ties:
        assert pool
        z, _ = pd.bn_affine(y, mean, invstd, gamma, beta)
        w4 = pd._windows(z)                                          # [4, B, Ho, Wo, C]
        y4 = pd._windows(y.double())
        arg = w4.argmax(dim=0, keepdim=True)
        ymax = y4.gather(0, arg)
        other = (arg + 1 + torch.randint(0, 3, arg.shape, generator=g)) % 4
        pick = (torch.rand(arg.shape, generator=g) < 0.5)
        y4 = torch.where(torch.zeros_like(y4, dtype=torch.bool).scatter_(0, other, pick), ymax.expand_as(y4), y4)
        rest = y.double().clone()
        rest[:, :2 * Ho, :2 * Wo] = pd._unwindows(y4, H, W)[:, :2 * Ho, :2 * Wo]
        y = rest.to(dtype)
    return dict(y=y, mean=mean, invstd=invstd, gamma=gamma, beta=beta, dz=dz, residual=res)


# ---- ROIAlign -------------------------------------------------------------------------------------------------------
ROI_MAP = (2, 21, 30)            # B, H, W
ROI_SCALE = 1.0 / 16
ROI_POOLED = (1, 2, 4, 7, 14)    # every pooled size a test uses: the preconditions hold for all of them


def _roi_ok(rois, H, W, scale, pooled_sizes):
    ok = torch.ones(rois.shape[0], dtype=torch.bool)
    for P in pooled_sizes:
        c, b = pd.roi_precondition_margins(pd.roi_align_matrices(rois, H, W, P, scale))
        ok &= (c >= 1.0) & (b >= 1e-4)
    return ok


def roi_set(n=300, seed=0, B=ROI_MAP[0], H=ROI_MAP[1], W=ROI_MAP[2], scale=ROI_SCALE, pooled_sizes=ROI_POOLED):
    """-> rois [n, 5] fp32 (CPU), images in random order: boxes inside the map, over every border, tiny, zero-sized,
    entirely outside, far larger than the map, and padding rows (batch index -1).  Candidates that break a precondition
    (oracle.pointwise_definitions.roi_precondition_margins) for any pooled size are redrawn."""
    g = torch.Generator().manual_seed(2000 + seed)
    Wp, Hp = W / scale, H / scale

    def draw(kind, k):
        u = lambda lo, hi: torch.empty(k).uniform_(lo, hi, generator=g)
        if kind == "inside":
            w, h = u(8, 0.7 * Wp), u(8, 0.7 * Hp)
            x1, y1 = u(0, 1) * (Wp - w), u(0, 1) * (Hp - h)
        elif kind == "border":
            w, h = u(20, 0.5 * Wp), u(20, 0.5 * Hp)
            side = torch.randint(0, 8, (k,), generator=g)
            x1, y1 = u(0, 1) * (Wp - w), u(0, 1) * (Hp - h)
            x1 = torch.where((side == 0) | (side == 4) | (side == 6), -u(0.1, 0.9) * w, x1)           # over the left border
            x1 = torch.where((side == 1) | (side == 5) | (side == 7), Wp - u(0.1, 0.9) * w, x1)       # right
            y1 = torch.where((side == 2) | (side == 4) | (side == 5), -u(0.1, 0.9) * h, y1)           # top
            y1 = torch.where((side == 3) | (side == 6) | (side == 7), Hp - u(0.1, 0.9) * h, y1)       # bottom
        elif kind == "tiny":
            w, h = u(0.3, 6.0), u(0.3, 6.0)
            x1, y1 = u(-4, Wp + 2), u(-4, Hp + 2)
        elif kind == "outside":
            w, h = u(10, 100), u(10, 100)
            side = torch.randint(0, 4, (k,), generator=g)
            x1, y1 = u(0, Wp), u(0, Hp)
            x1 = torch.where(side == 0, -w - u(40, 400), x1)
            x1 = torch.where(side == 1, Wp + u(40, 400), x1)
            y1 = torch.where(side == 2, -h - u(40, 400), y1)
            y1 = torch.where(side == 3, Hp + u(40, 400), y1)
        elif kind == "huge":
            w, h = u(3 * Wp, 12 * Wp), u(3 * Hp, 12 * Hp)
            x1, y1 = -u(0.2, 0.6) * w, -u(0.2, 0.6) * h
        else:
            raise ValueError(kind)
        b = torch.randint(0, B, (k,), generator=g).float()
        return torch.stack([b, x1, y1, x1 + w, y1 + h], 1)

    def accepted(kind, k):
        out = torch.zeros(0, 5)
        for _ in range(100):
            c = draw(kind, 2 * k + 8)
            out = torch.cat([out, c[_roi_ok(c, H, W, scale, pooled_sizes)]])
            if out.shape[0] >= k:
                return out[:k]
        raise RuntimeError(f"could not draw {k} {kind} ROIs that keep the preconditions")

    n_pad, n_zero, n_out, n_huge = max(n // 30, 2), 4, max(n // 60, 4), max(n // 100, 3)
    n_tiny, n_border = n // 12, n // 5
    zero = draw("inside", n_zero)
    zero[:, 3], zero[:, 4] = zero[:, 1], zero[:, 2]                 # zero-sized: grid 0, count 1, output 0
    zero[1, 4] = zero[1, 2] + 40.0                                  # zero width only
    pad = draw("inside", n_pad)
    pad[:, 0] = -1.0
    parts = [accepted("border", n_border), accepted("tiny", n_tiny), accepted("outside", n_out), accepted("huge", n_huge),
             zero, pad]
    parts.insert(0, accepted("inside", n - sum(p.shape[0] for p in parts)))
    rois = torch.cat(parts)
    return rois[torch.randperm(n, generator=g)].contiguous()
