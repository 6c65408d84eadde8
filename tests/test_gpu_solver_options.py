"""Solver options of the fused optimiser on the GPU: per-tensor gradient clipping (sfod_grad_clip_coef), the table-driven
update (sfod_sgd_ema_seg: per-tensor weight decay / lr factor / clip coefficient, Nesterov) and the public surface
(build_optimizer / build_lr_scheduler).

The reference everywhere is torch on the CPU: ``torch.optim.SGD`` over plain fp32 tensors with one param group per
distinct hyper-parameter set, ``clip_grad_norm_`` / ``clip_grad_value_`` called once per tensor, the teacher blended
with ``_update_teacher_model``'s expression  student * (1 - k) + teacher * k.

Gates
  * "value", ("norm", inf) and every tensor that does not clip: the arithmetic is elementwise (a max does not depend on
    the order) -> test_sgd_ema_fused's tolerances for this kernel family, rtol 1e-6 / atol 1e-7, on parameters, momentum
    and teacher.
  * ("norm", 2.0): the clip coefficient of a tensor depends on a summation order.  Yardstick: the relative distance of
    torch's own fp32 ``clip_grad_norm_`` coefficient from the float64 one on the same data; the device is gated at FOUR
    times the largest such distance over the tensors (another order may land on the other side), never below 1e-6.
    A relative error e of a coefficient moves the clipped gradient g' by e * |g'|; through three steps of momentum mu
    the parameter moves by at most  lr * lr_factor * e * max|g'| * K  with  K = (1 + mu) * (1 + (1 + mu) + (1 + mu + mu^2))
    = 10.66 (the (1 + mu) covers Nesterov's look-ahead), the momentum buffer by  e * max|g'| * (1 + mu + mu^2); these are
    added to the elementwise atol per tensor.  (The weight-decay feedback of that error is lr * wd times smaller.)
    Measured relative distances from float64 on test_clip_kernels_match_torch's data (12 tensors x 3 steps; printed
    by the test under -s, recorded in DESIGN.md): grad_scale 1.0: torch fp32 4.6e-7, the device 4.9e-8, gate 1.84e-6;
    grad_scale 0.5: torch 3.5e-7, the device 6.1e-8, gate 1.41e-6.  Max-norm: both 4.8e-8 / 3.6e-8 (the same bits).
"""
import math
import os

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
HOT_YAML = os.path.join(ROOT, "configs", "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free.yaml")
INF = float("inf")
MOM, KEEP, LR = 0.9, 0.9996, 0.02
K_PARAM = (1 + MOM) * (1 + (1 + MOM) + (1 + MOM + MOM * MOM))
K_MOM = 1 + MOM + MOM * MOM

# a segment smaller than a float4, several segments inside one 4096-element chunk, one segment over many chunks, a
# one-element segment between two large ones, a last segment that ends off a chunk boundary
LENS = [1, 3, 4, 5, 64, 255, 256, 257, 4099, 70001, 1, 262147]


def pad4(n):
    return (n + 3) // 4 * 4


def offsets(lens):
    offs, o = [], 0
    for k in lens:
        offs.append(o)
        o += pad4(k)
    return offs, o


def pack(tensors, lens):
    offs, n = offsets(lens)
    flat = torch.zeros(n)
    for t, o, k in zip(tensors, offs, lens):
        flat[o:o + k] = t.flatten()
    return flat


def unpack(flat, lens):
    offs, _ = offsets(lens)
    return [flat[o:o + k] for o, k in zip(offs, lens)]


def padding_mask(lens):
    offs, n = offsets(lens)
    mask = torch.ones(n, dtype=torch.bool)
    for o, k in zip(offs, lens):
        mask[o:o + k] = False
    return mask


def seg_norm(g, norm_type):
    return g.double().abs().max() if norm_type == INF else g.double().pow(2).sum().sqrt()


def planted_gradients(shapes, norm_type, seed, steps=3):
    """[step][tensor]: randn, each tensor scaled so that its norm is 4.0 or 0.25, alternating over tensors and steps: with
    CLIP_VALUE 1.0 and grad_scale 1.0 or 0.5 half of the tensors clip (norm 4 / 2) and half do not (0.25 / 0.125)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for step in range(steps):
        row = []
        for i, shp in enumerate(shapes):
            x = torch.randn(shp, generator=g)
            target = 4.0 if (i + step) % 2 == 0 else 0.25
            row.append((x * (target / seg_norm(x, norm_type))).float())
        out.append(row)
    return out


def torch_reference(p0, t0, grads, wd, lf, lrs, mode, norm_type, clip_value, nesterov, gs):
    """-> dict: p / m / t (lists of tensors), c32 / c64 [step][tensor] (torch's fp32 coefficient, the float64 one),
    gmax [tensor] (largest |clipped gradient| over the steps)"""
    params = [x.clone().requires_grad_(True) for x in p0]
    groups = {}
    for p, w, f in zip(params, wd, lf):
        groups.setdefault((w, f), []).append(p)
    opt = torch.optim.SGD([{"params": ps, "weight_decay": w, "lf": f} for (w, f), ps in groups.items()], lr=lrs[0],
                          momentum=MOM, nesterov=nesterov)
    t = [x.clone() for x in t0]
    c32, c64, gmax = [], [], [0.0] * len(params)
    for step, row in enumerate(grads):
        for grp in opt.param_groups:
            grp["lr"] = lrs[step] * grp["lf"]
        c32.append([]), c64.append([])
        for i, (p, g) in enumerate(zip(params, row)):
            p.grad = g * gs
            if mode == "norm":
                c64[-1].append(min(1.0, clip_value / (seg_norm(p.grad, norm_type).item() + 1e-6)))
                n32 = torch.nn.utils.clip_grad_norm_(p, clip_value, norm_type)        # once per tensor
                c32[-1].append(torch.clamp(clip_value / (n32 + 1e-6), max=1.0).item())
            elif mode == "value":
                torch.nn.utils.clip_grad_value_(p, clip_value)
            gmax[i] = max(gmax[i], p.grad.abs().max().item())
        opt.step()
        with torch.no_grad():
            for s, ts in zip(params, t):
                ts.copy_(s * (1 - KEEP) + ts * KEEP)
    return {"p": [p.detach() for p in params], "m": [opt.state[p]["momentum_buffer"] for p in params], "t": t,
            "c32": c32, "c64": c64, "gmax": gmax}


def device_run(native, lens, p0, t0, grads, wd, lf, lrs, mode, norm_type, clip_value, nesterov, gs):
    """the same steps through sfod_grad_clip_coef + sfod_sgd_ema_seg -> flat p, m, t on the CPU, coef [step] tensors"""
    offs, n = offsets(lens)
    p, t = pack(p0, lens).to(DEV), pack(t0, lens).to(DEV)
    m = torch.zeros_like(p)
    seg_off = torch.tensor(offs, dtype=torch.int64, device=DEV)
    seg_len = torch.tensor(lens, dtype=torch.int64, device=DEV)
    seg_hp = torch.tensor(list(zip(wd, lf)), dtype=torch.float32, device=DEV)
    coef = torch.ones(len(lens), device=DEV) if mode == "norm" else None
    ws = native.grad_clip_ws(n, len(lens), DEV)
    lr = torch.zeros(1, device=DEV)
    coefs = []
    for step, row in enumerate(grads):
        g = pack(row, lens).to(DEV)
        lr.fill_(lrs[step])
        if mode == "norm":
            ws.fill_(float("nan"))                  # the workspace need not be initialised: no stale slot is read
            native.grad_clip_coef_(coef, g, seg_off, seg_len, gs, clip_value, norm_type, ws)
            coefs.append(coef.cpu().clone())
        native.sgd_ema_seg_(p, g, m, t, seg_off, seg_hp, coef, lr, MOM, gs, mode, clip_value, nesterov, KEEP, step == 0)
    return p.cpu(), m.cpu(), t.cpu(), coefs


def check_against_reference(ref, got, lens, lf, lr_max, mode, norm_type, label=""):
    """the gates of the module docstring; -> (torch's, the device's) largest relative coefficient distance from float64"""
    p, m, t, coefs = got
    d_torch = d_dev = 0.0
    gate = 0.0
    clipped = [False] * len(lens)
    if mode == "norm":
        for step, c in enumerate(coefs):
            for i in range(len(lens)):
                c64 = ref["c64"][step][i]
                clipped[i] = clipped[i] or c64 < 1.0
                d_torch = max(d_torch, abs(ref["c32"][step][i] - c64) / c64)
                d_dev = max(d_dev, abs(c[i].item() - c64) / c64)
        gate = max(4 * d_torch, 1e-6) if norm_type == 2.0 else 1e-6
        print("%s coefficient distance from float64: torch fp32 %.3g, device %.3g, gate %.3g" % (label, d_torch, d_dev, gate))
        for step, c in enumerate(coefs):
            for i in range(len(lens)):
                c64 = ref["c64"][step][i]
                if c64 == 1.0:
                    assert c[i].item() == 1.0, (step, i)          # a tensor that does not clip: exactly 1
                else:
                    assert abs(c[i].item() - c64) <= gate * c64, (step, i, c[i].item(), c64)
    order_dependent = mode == "norm" and norm_type == 2.0
    for name, flat, k in (("p", p, K_PARAM * lr_max), ("m", m, K_MOM), ("t", t, K_PARAM * lr_max)):
        for i, (a, b) in enumerate(zip(unpack(flat, lens), ref[name])):
            extra = gate * ref["gmax"][i] * k * (lf[i] if name != "m" else 1.0) if order_dependent and clipped[i] else 0.0
            torch.testing.assert_close(a, b.flatten(), rtol=1e-6, atol=1e-7 + extra, msg=lambda s: f"{name}[{i}]: {s}")
        assert (flat[padding_mask(lens)] == 0).all(), name      # padding lanes hold zeros and keep them
    return d_torch, d_dev


def segment_case(norm_type, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    p0 = [torch.randn(k, generator=g) for k in LENS]
    t0 = [torch.randn(k, generator=g) for k in LENS]
    wd = [(1e-4, 0.0, 5e-4)[i % 3] for i in range(len(LENS))]
    lf = [(1.0, 2.0)[(i // 2) % 2] for i in range(len(LENS))]
    return p0, t0, planted_gradients([(k,) for k in LENS], norm_type, seed), wd, lf


_cases = {}


def cached_case(norm_type):
    if norm_type not in _cases:
        _cases[norm_type] = segment_case(norm_type)
    return _cases[norm_type]


@pytest.mark.parametrize("gs", [1.0, 0.5])
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("mode,norm_type", [("norm", 2.0), ("norm", INF), ("value", None)])
def test_clip_kernels_match_torch(native, mode, norm_type, nesterov, gs):
    """Three steps, fresh gradient each, teacher attached, per-tensor weight decay and lr factor, on segments chosen to
    break a segmented reduction (LENS).  Gates: module docstring."""
    p0, t0, grads, wd, lf = cached_case(INF if mode == "value" else norm_type)
    # the split the data was built for, verified here: both kinds of tensor are present at every step
    for row in grads:
        if mode == "value":
            clips = [bool(((g * gs).abs() > 1.0).any()) for g in row]
        else:
            clips = [seg_norm(g * gs, norm_type).item() > 1.0 for g in row]
        assert 4 <= sum(clips) <= len(LENS) - 4, clips
    lrs = [LR, LR * 0.5, LR * 0.25]
    ref = torch_reference(p0, t0, grads, wd, lf, lrs, mode, norm_type, 1.0, nesterov, gs)
    got = device_run(native, LENS, p0, t0, grads, wd, lf, lrs, mode, norm_type, 1.0, nesterov, gs)
    check_against_reference(ref, got, LENS, lf, LR, mode, norm_type, label=f"[{mode}-{norm_type}-{nesterov}-{gs}]")


def test_clip_reduction_is_deterministic(native):
    """Two runs from the same inputs give identical bytes: coefficients, parameters, momentum, teacher."""
    p0, t0, grads, wd, lf = cached_case(2.0)
    runs = [device_run(native, LENS, p0, t0, grads, wd, lf, [LR] * 3, "norm", 2.0, 1.0, False, 1.0) for _ in range(2)]
    for a, b in zip(runs[0][:3], runs[1][:3]):
        assert torch.equal(a, b)
    for a, b in zip(runs[0][3], runs[1][3]):
        assert torch.equal(a, b)


def test_table_kernel_equals_the_two_group_kernel_bit_for_bit(native):
    """(a) "norm" with a CLIP_VALUE no tensor reaches (every coefficient exactly 1.0f) == the table kernel without
    clipping; (c) the table kernel fed only the two weight-decay groups == today's sgd_ema_ on the two ranges; all bit for
    bit over three steps, with a grad_scale that is no power of two."""
    p0, t0, grads, _, _ = cached_case(2.0)
    split = 8                                               # tensors [0, 8): decayed, [8, 12): not
    wd = [1e-4] * split + [0.0] * (len(LENS) - split)
    lf = [1.0] * len(LENS)
    gs, lrs = 0.37, [LR, LR * 0.5, LR * 0.25]
    plain = device_run(native, LENS, p0, t0, grads, wd, lf, lrs, None, None, 0.0, False, gs)
    huge = device_run(native, LENS, p0, t0, grads, wd, lf, lrs, "norm", 2.0, 1e30, False, gs)
    for c in huge[3]:
        assert (c == 1.0).all()
    offs, n = offsets(LENS)
    b = offs[split]
    p, t = pack(p0, LENS).to(DEV), pack(t0, LENS).to(DEV)
    m = torch.zeros_like(p)
    lr = torch.zeros(1, device=DEV)
    for step, row in enumerate(grads):
        g = pack(row, LENS).to(DEV)
        lr.fill_(lrs[step])
        native.sgd_ema_(p[:b], g[:b], m[:b], t[:b], lr, MOM, 1e-4, gs, KEEP, step == 0)
        native.sgd_ema_(p[b:], g[b:], m[b:], t[b:], lr, MOM, 0.0, gs, KEEP, step == 0)
    for old, a, c in zip((p.cpu(), m.cpu(), t.cpu()), plain[:3], huge[:3]):
        assert torch.equal(old, a) and torch.equal(a, c)
    assert not torch.equal(p.cpu(), pack(p0, LENS))         # (the steps did move the parameters)


def _small_net(seed):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 6, 3), torch.nn.BatchNorm2d(6), torch.nn.Conv2d(6, 4, 1),
                              torch.nn.BatchNorm2d(4), torch.nn.Linear(5, 3))
    for p in net[2].parameters():       # a frozen layer: laid out, EMA'd, never stepped
        p.requires_grad_(False)
    return net.to(DEV)


def _record_calls(monkeypatch, native):
    names, orig = [], native.call

    def call(name, *a, **k):
        names.append(name)
        return orig(name, *a, **k)
    monkeypatch.setattr(native, "call", call)
    return names


def test_default_options_take_the_existing_kernels(sfod, native, monkeypatch):
    """(b) every new option off: FusedSGD.step is today's sequence of sgd_ema_ / ema_ calls, bit for bit, and launches
    nothing else."""
    cfg = sfod.config.setup_cfg(HOT_YAML, ["SOLVER.BASE_LR", "0.02", "SOLVER.WARMUP_ITERS", "0"])
    E = sfod.engine
    student, teacher = _small_net(1), _small_net(2)
    opt = E.build_optimizer(cfg, student)
    tflat = E.FlatModelState(teacher, with_grad=False)
    opt.attach_teacher(tflat, KEEP)
    opt.grad_scale = 0.5
    assert not opt.table_driven
    f = opt.flat
    p, t, m = f.param.clone(), tflat.param.clone(), torch.zeros_like(f.param)
    fb, ib = tflat.fbuf.clone(), tflat.ibuf.clone()
    g = torch.Generator().manual_seed(5)
    grads = [torch.randn(f.n_total, generator=g).to(DEV) for _ in range(3)]
    names = _record_calls(monkeypatch, native)
    for step in range(3):
        f.grad.copy_(grads[step])
        opt.step(ema=True)
    assert names == ["sfod_sgd_ema", "sfod_sgd_ema", "sfod_ema", "sfod_ema", "sfod_ema_i64"] * 3
    a, b, n = f.n_decay, f.n_norm_end, f.n_total
    assert 0 < a < b < n
    for step in range(3):
        native.sgd_ema_(p[:a], grads[step][:a], m[:a], t[:a], opt.lr_dev, MOM, 1e-4, 0.5, KEEP, step == 0)
        native.sgd_ema_(p[a:b], grads[step][a:b], m[a:b], t[a:b], opt.lr_dev, MOM, 0.0, 0.5, KEEP, step == 0)
        native.ema_(t[b:n], p[b:n], KEEP)
        native.ema_(fb, f.fbuf, KEEP)
        native.ema_i64_(ib, f.ibuf, KEEP)
    assert torch.equal(f.param, p) and torch.equal(opt.mom, m) and torch.equal(tflat.param, t)
    assert torch.equal(tflat.fbuf, fb) and torch.equal(tflat.ibuf, ib)


def test_non_finite_gradient_propagates_like_torch(native):
    """One inf in a 5-element tensor under ("norm", 2.0): torch's coefficient is 0 and the clipped gradient
    [nan, 0, 0, 0, 0]; the device gives the same pattern and leaves the neighbours alone (a value check).  Read back as
    the step of lr 1 without momentum or decay from p = 0:  p = -g'."""
    lens = [7, 5, 9]
    g = torch.Generator().manual_seed(9)
    grads = [torch.randn(7, generator=g) * 3, torch.randn(5, generator=g), torch.randn(9, generator=g) * 0.1]
    grads[1][0] = INF
    ref = []
    for x in grads:
        p = torch.zeros_like(x).requires_grad_(True)
        p.grad = x.clone()
        torch.nn.utils.clip_grad_norm_(p, 1.0, 2.0)
        ref.append(p.grad)
    assert math.isnan(ref[1][0].item()) and ref[1][1:].tolist() == [0.0] * 4
    assert seg_norm(grads[0], 2.0) > 1 > seg_norm(grads[2], 2.0)        # one neighbour clips, the other does not
    offs, n = offsets(lens)
    seg_off = torch.tensor(offs, dtype=torch.int64, device=DEV)
    seg_len = torch.tensor(lens, dtype=torch.int64, device=DEV)
    seg_hp = torch.tensor([[0.0, 1.0]] * 3, dtype=torch.float32, device=DEV)
    coef = torch.ones(3, device=DEV)
    gd = pack(grads, lens).to(DEV)
    p, m = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    native.grad_clip_coef_(coef, gd, seg_off, seg_len, 1.0, 1.0, 2.0, native.grad_clip_ws(n, 3, DEV))
    native.sgd_ema_seg_(p, gd, m, None, seg_off, seg_hp, coef, torch.ones(1, device=DEV), 0.0, 1.0, "norm", 1.0, False, 0.0, True)
    assert coef[1].item() == 0.0 and coef[2].item() == 1.0 and 0 < coef[0].item() < 1
    got = unpack(-p.cpu(), lens)
    assert math.isnan(got[1][0].item()) and got[1][1:].tolist() == [0.0] * 4
    torch.testing.assert_close(got[0], ref[0], rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(got[2], ref[2], rtol=0, atol=0)
    # a NaN gradient: NaN norm, NaN coefficient (the clamp keeps it), under both norms
    gd[offs[1]] = float("nan")
    for norm_type in (2.0, INF):
        native.grad_clip_coef_(coef, gd, seg_off, seg_len, 1.0, 1.0, norm_type, native.grad_clip_ws(n, 3, DEV))
        assert math.isnan(coef[1].item()) and not math.isnan(coef[0].item()) and coef[2].item() == 1.0


def test_solver_options_through_build_optimizer(sfod, native, monkeypatch):
    """The VGG detector with small heads (the model test_host_logic's solver test builds), CLIP_GRADIENTS norm + NESTEROV
    + BIAS_LR_FACTOR 2 + WEIGHT_DECAY_BIAS 0 + WarmupCosineLR: three optimizer.step() + scheduler.step() on planted
    gradients against torch SGD on the CPU with Detectron2's grouping rule restated here; every parameter and the EMA
    teacher under the module docstring's gates.  Per step: two launches for the coefficients, one for the update."""
    cfg = sfod.config.setup_cfg(HOT_YAML, [
        "OUTPUT_DIR", "", "MODEL.ROI_BOX_HEAD.FC_DIM", "64", "SOLVER.CLIP_GRADIENTS.ENABLED", "True",
        "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "norm", "SOLVER.NESTEROV", "True", "SOLVER.BIAS_LR_FACTOR", "2.0",
        "SOLVER.WEIGHT_DECAY_BIAS", "0.0", "SOLVER.LR_SCHEDULER_NAME", "WarmupCosineLR", "SOLVER.BASE_LR", "0.02",
        "SOLVER.WARMUP_ITERS", "2", "SOLVER.WARMUP_FACTOR", "0.1", "SOLVER.MAX_ITER", "10"])
    E = sfod.engine
    torch.manual_seed(3)
    student = sfod.modeling.build_model(cfg)
    torch.manual_seed(4)
    teacher = sfod.modeling.build_model(cfg)
    frozen = ("DC_img.", "DC_ins.") if ("DOMAIN_CLASSIFIER" in cfg and not cfg.DOMAIN_CLASSIFIER.ENABLED) else ()
    opt = E.build_optimizer(cfg, student, frozen=frozen)
    sched = E.build_lr_scheduler(cfg, opt)
    tflat = E.FlatModelState(teacher, frozen_prefixes=frozen, with_grad=False)
    opt.attach_teacher(tflat, KEEP)
    assert opt.table_driven and isinstance(sched, E.WarmupCosineLR)
    # Detectron2's get_default_optimizer_params, restated
    norm_owned = {id(p) for mod in student.modules() if isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d, torch.nn.GroupNorm, torch.nn.LayerNorm))
                  for p in mod.parameters(recurse=False)}
    names, wd, lf, p0, t0 = [], [], [], [], []
    tparams = dict(teacher.named_parameters())
    for n, p in student.named_parameters():
        if not p.requires_grad or n.startswith(frozen):
            continue
        w, f = (cfg.SOLVER.WEIGHT_DECAY_NORM if id(p) in norm_owned else cfg.SOLVER.WEIGHT_DECAY), 1.0
        if n.rsplit(".", 1)[-1] == "bias":
            w, f = 0.0, 2.0
        names.append(n), wd.append(w), lf.append(f)
        p0.append(p.detach().cpu().clone()), t0.append(tparams[n].detach().cpu().clone())
    assert len(names) > 50 and sum(f == 2.0 for f in lf) > 20
    assert set(zip(wd, lf)) == {(1e-4, 1.0), (0.0, 1.0), (0.0, 2.0)}      # weights, BatchNorm weights, every bias
    grads = planted_gradients([tuple(p.shape) for p in p0], 2.0, seed=11)
    lrs = []
    for it in range(3):
        warm = 1.0 if it >= 2 else 0.1 * (1 - it / 2) + it / 2
        lrs.append(0.02 * warm * 0.5 * (1 + math.cos(math.pi * it / 10)))
    ref = torch_reference(p0, t0, grads, wd, lf, lrs, "norm", 2.0, 1.0, True, 1.0)
    f = opt.flat
    index = {r[0]: i for i, r in enumerate(opt.hyper)}
    assert sorted(index) == sorted(names)
    calls = _record_calls(monkeypatch, native)
    before = f.param.clone()
    coefs = []
    for step in range(3):
        assert abs(opt.param_groups[0]["lr"] - lrs[step]) < 1e-15
        opt.zero_grad()
        for n, g in zip(names, grads[step]):
            o, k, _ = f.offsets[n]
            f.grad[o:o + k].copy_(g.flatten())
        opt.step(ema=True)
        sched.step()
        coefs.append(opt.clip_coef.cpu()[[index[n] for n in names]])
    per_step = ["sfod_grad_clip_coef", "sfod_sgd_ema_seg"]
    assert [c for c in calls if "sgd" in c or "clip" in c] == per_step * 3 and calls[:2] == per_step
    lens = [p.numel() for p in p0]
    got = tuple(pack([x[f.offsets[n][0]:f.offsets[n][0] + f.offsets[n][1]].cpu() for n in names], lens)
                for x in (f.param, opt.mom, tflat.param)) + (coefs,)
    check_against_reference(ref, got, lens, lf, max(lrs), "norm", 2.0, label="[build_optimizer]")
    assert sum(c < 1.0 for c in ref["c64"][0]) > 20 and sum(c == 1.0 for c in ref["c64"][0]) > 20
    for n in f.offsets:                            # what is not optimised stayed where it was
        if n not in index:
            o, k, _ = f.offsets[n]
            assert torch.equal(before[o:o + k], f.param[o:o + k]), n
