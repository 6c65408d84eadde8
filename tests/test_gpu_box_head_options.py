"""Box-head architecture options on the device: MODEL.ROI_BOX_HEAD.{NUM_CONV, CONV_DIM, NUM_FC, FC_DIM, NORM}.

GroupNorm + ReLU (sfod_group_norm_relu_fwd / _bwd) per element against torch float64 (``F.group_norm`` and autograd,
tests/helpers/box_head_definitions.py) under that helper's derived bounds -- no free tolerance; the bounds are validated
against an honest fp32 evaluation on the CPU by tests/test_box_head_options_host.py, never against the kernels.  Cases: C 32
(one channel per group), 96 (groups of 3 straddle the 8-channel pair groups), 256; PP 1, 49, 196; R 3 and 300 (the last two
ROIs of the 300 all zero: padding rows); fp32 and bf16 everywhere, bf16x3 and f16x3 at C 96 and 256.  The uniformity checks
of ``assert_matches_definition`` are off: a GroupNorm's error is dominated by its (ROI, group) mean, ONE random draw per group
whose bound is ~LAMBDA sqrt(n) times its typical size, so error / bound is not uniform over blocks or channels by construction.

Module level: ``StandardROIHeads`` on a 2 x 21 x 30 map with 40 channels for four heads, losses and every parameter gradient
against the float64 composition on the pass's own sampled ROIs.  Gates: fp32 -- a loss within 4 x max(torch-fp32's distance
from float64, 2^-24 x loss) (box_reg_definitions.gate, the gate of the other module-level option tests); bf16x3 / f16x3 -- a loss
within 1e-4 relative (tests/test_gpu_model.py's gate for every arithmetic mode); gradients 2e-3 relative L2 in every mode.
What a trainer step adds to the head's gradients -- the ROI losses and the instance-level domain loss, two backward passes into
preallocated non-zero ``.grad`` sinks -- against float64 for a GN head and a head without a norm.  Step level: two deterministic
trainer steps with the GN head, run twice.
"""
import importlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from helpers import box_head_definitions as bd
from helpers import box_reg_definitions as D
from helpers import definition_check as dc
from oracle import model as om

pytestmark = pytest.mark.gpu
DEV = "cuda"
HOT_YAML = os.path.join(os.path.dirname(GOLDEN), "..", "configs",
                        "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free.yaml")
H = "MODEL.ROI_BOX_HEAD."
SHAPES = [(R, PP, C) for C in (32, 96, 256) for PP in (1, 49, 196) for R in (3, 300)]
CASES = [(s, m) for s in SHAPES for m in (("fp32",) + (("bf16x3", "f16x3") if s[2] != 32 else ()) + ("bf16",))]
IDS = [f"R{s[0]}-PP{s[1]}-C{s[2]}-{m}" for s, m in CASES]
_last = {}


def _defn(shape, mode, backward=False):
    """the case's inputs and float64 definition, computed once per (shape, input rounding) -- the cases run shape-major, so
    only the latest is kept"""
    R, PP, C = shape
    key = (shape, mode == "bf16")
    if _last.get("key") != key:
        y, dz, gamma, beta = bd.gn_case(R, PP, C, seed=R + PP + C, pad_rows=2 if R == 300 else 0)
        if mode == "bf16":
            y, dz = y.bfloat16().float(), dz.bfloat16().float()
        _last.clear()
        _last.update(key=key, y=y, dz=dz, gamma=gamma, beta=beta, defn=bd.gn_forward(y, gamma, beta))
    if backward and "bw" not in _last:
        _last["bw"] = bd.gn_backward(_last["defn"], _last["y"], _last["dz"])
    return _last


def _pair_dtype(native, mode):
    return {"bf16x3": native.SPLIT_DTYPE, "f16x3": native.SPLITH_DTYPE}.get(mode)


def _f32(native, t):
    return native.cast(t, torch.float32) if native.is_pairs(t.dtype) else t.float()


def _as(t, R, PP, C):       # [R, PP, C] -> the checker's NHWC: one ROI = one "image", its pixels a column
    return t.reshape(R, PP, 1, C)


@pytest.mark.parametrize("shape,mode", CASES, ids=IDS)
def test_group_norm_forward_matches_its_definition(native, shape, mode):
    R, PP, C = shape
    c = _defn(shape, mode)
    defn = c["defn"]
    y = c["y"].to(DEV)
    y = y.bfloat16() if mode == "bf16" else y
    gamma, beta = c["gamma"].to(DEV), c["beta"].to(DEV)
    z, zg, mean, rstd = native.group_norm_relu_fwd(y, gamma, beta, 32, 1e-5, out_dtype=_pair_dtype(native, mode),
                                                   with_grad_operand=mode == "f16x3")
    got = _f32(native, z)
    dc.assert_matches_definition(_as(got.cpu(), R, PP, C), _as(defn.z, R, PP, C), _as(defn.z.abs(), R, PP, C), 1, mode, out=mode,
                                 bnd=_as(bd.gn_forward_bound(defn, mode), R, PP, C), uniform=(),
                                 label=f"group_norm fwd R={R} PP={PP} C={C}")
    dc.assert_channels_within(mean, defn.mean, defn.tol_mean, label=f"group_norm mean R={R} PP={PP} C={C} {mode}")
    dc.assert_channels_within(rstd, defn.rstd, defn.tol_rstd, label=f"group_norm rstd R={R} PP={PP} C={C} {mode}")
    rb = torch.relu(beta)            # what an all-zero ROI, or a group of one element, gives: exactly, in the output type
    want = rb.bfloat16().float() if mode == "bf16" else rb
    if _pair_dtype(native, mode) is not None:
        want = native.cast(native.cast(rb.contiguous(), _pair_dtype(native, mode)), torch.float32)
    if R == 300:
        assert torch.equal(got[-2:], want.expand(2, PP, C)), "padding rows are exactly relu(beta)"
    if C == 32 and PP == 1:
        assert torch.equal(got, want.expand(R, PP, C)), "zero variance: exactly relu(beta)"
    if mode == "f16x3":              # the producer-writes-both convention: each output has the bits of its own single-output run
        zh = native.group_norm_relu_fwd(y, gamma, beta, out_dtype=native.SPLITH_DTYPE)[0]
        zb = native.group_norm_relu_fwd(y, gamma, beta, out_dtype=native.SPLIT_DTYPE)[0]
        assert z.dtype == native.SPLITH_DTYPE and zg.dtype == native.SPLIT_DTYPE
        assert torch.equal(z.view(torch.float16), zh.view(torch.float16))
        assert torch.equal(zg.view(torch.bfloat16), zb.view(torch.bfloat16))
    elif mode == "bf16x3":
        assert zg is None
        z1, zg1, _, _ = native.group_norm_relu_fwd(y, gamma, beta, out_dtype=native.SPLIT_DTYPE, with_grad_operand=True)
        assert zg1 is z1


@pytest.mark.parametrize("shape,mode", CASES, ids=IDS)
def test_group_norm_backward_matches_autograd(native, shape, mode):
    R, PP, C = shape
    c = _defn(shape, mode, backward=True)
    defn, bw = c["defn"], c["bw"]
    y, dz = c["y"].to(DEV), c["dz"].to(DEV)
    if mode == "bf16":
        y, dz = y.bfloat16(), dz.bfloat16()
    gamma, beta = c["gamma"].to(DEV), c["beta"].to(DEV)
    _, _, mean, rstd = native.group_norm_relu_fwd(y, gamma, beta)
    odt = native.SPLIT_DTYPE if mode in ("bf16x3", "f16x3") else None          # the backward products' operand: bf16 pairs
    out = "bf16x3" if odt is not None else mode
    dy, dgamma, dbeta = native.group_norm_relu_bwd(dz, y, mean, rstd, gamma, beta, out_dtype=odt)
    tol_db, tol_dg, bnd = bd.gn_backward_bounds(defn, bw, out)
    near = bd.near_gate(defn)
    share = float(near.double().mean())
    print(f"[group_norm bwd R={R} PP={PP} C={C} {mode}] elements within their forward bound of the gate: {share:.2e}")
    assert share <= 1e-3
    got = _f32(native, dy).cpu().double()
    got = torch.where(near, bw.dy, got)                      # left out of the comparison
    dc.assert_matches_definition(_as(got, R, PP, C), _as(bw.dy, R, PP, C), _as(bw.dy.abs(), R, PP, C), 1, mode, out=out,
                                 bnd=_as(bnd, R, PP, C), uniform=(), label=f"group_norm bwd dy R={R} PP={PP} C={C}")
    dc.assert_channels_within(dbeta, bw.dbeta, tol_db, label=f"group_norm dbeta R={R} PP={PP} C={C} {mode}")
    dc.assert_channels_within(dgamma, bw.dgamma, tol_dg, label=f"group_norm dgamma R={R} PP={PP} C={C} {mode}")
    if R == 300:                                              # padding rows: no gradient, and nothing into the sums
        assert float(_f32(native, dy)[-2:].abs().max()) == 0.0
        _, dg2, db2 = native.group_norm_relu_bwd(dz[:-2].contiguous(), y[:-2].contiguous(), mean[:-2].contiguous(),
                                                 rstd[:-2].contiguous(), gamma, beta, out_dtype=odt)
        assert torch.equal(dg2, dgamma) and torch.equal(db2, dbeta)
    # twice: the same bits; accumulate = 1: the sum
    dy2, dg2, db2 = native.group_norm_relu_bwd(dz, y, mean, rstd, gamma, beta, out_dtype=odt)
    view = torch.bfloat16 if odt is not None else dy.dtype
    assert torch.equal(dy.view(view), dy2.view(view)) and torch.equal(dg2, dgamma) and torch.equal(db2, dbeta)
    g0, b0 = torch.randn(C, generator=torch.Generator().manual_seed(C)).to(DEV), torch.full((C,), 0.25, device=DEV)
    ga, ba = g0.clone(), b0.clone()
    native.group_norm_relu_bwd(dz, y, mean, rstd, gamma, beta, dgamma=ga, dbeta=ba, accumulate=True, out_dtype=odt)
    assert torch.equal(ga, g0 + dgamma) and torch.equal(ba, b0 + dbeta)


def test_group_norm_with_no_roi(native):
    y = torch.empty(0, 49, 64, device=DEV)
    gamma, beta = torch.ones(64, device=DEV), torch.zeros(64, device=DEV)
    z, _, mean, rstd = native.group_norm_relu_fwd(y, gamma, beta, out_dtype=native.SPLIT_DTYPE)
    assert tuple(z.shape) == (0, 49, 64) and tuple(mean.shape) == (0, 32)
    dg, db = torch.full((64,), 3.0, device=DEV), torch.full((64,), 3.0, device=DEV)
    native.group_norm_relu_bwd(y, y, mean, rstd, gamma, beta, dgamma=dg, dbeta=db)
    assert float(dg.abs().max()) == 0.0 and float(db.abs().max()) == 0.0
    dg.fill_(3.0)
    native.group_norm_relu_bwd(y, y, mean, rstd, gamma, beta, dgamma=dg, dbeta=db, accumulate=True)
    assert float(dg.min()) == 3.0


# ---- module level ----------------------------------------------------------------------------------------------------------
HEADS = {"2conv1fc-gn": (2, 64, 1, 128, "GN"), "1conv0fc": (1, 32, 0, 64, ""), "0conv1fc": (0, 32, 1, 64, ""),
         "0conv3fc": (0, 32, 3, 64, ""), "1conv1fc": (1, 32, 1, 64, "")}      # the last: the into-sink case without a norm
MODULE_CASES = [(h, m) for h in list(HEADS)[:4] for m in ("fp32", "bf16x3")] + [("2conv1fc-gn", "f16x3"), ("1conv0fc", "f16x3")]
Bm, Cm, Hf, Wf, Himg, Wimg = 2, 40, 21, 30, 336, 480


def _head_opts(name):
    nc, cd, nf, fd, norm = HEADS[name]
    return [H + "NUM_CONV", str(nc), H + "CONV_DIM", str(cd), H + "NUM_FC", str(nf), H + "FC_DIM", str(fd), H + "NORM", norm]


def _build_heads(sfod, name, mode, seed=11):
    cfg = sfod.config.setup_cfg(HOT_YAML, ["OUTPUT_DIR", "", "SFOD.COMPUTE_DTYPE", mode, "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", "64"]
                                + _head_opts(name))
    torch.manual_seed(seed)
    rh = importlib.import_module("simple-sfod_amd.modeling.roi_heads")
    heads = rh.StandardROIHeads(cfg, {"vgg4": sfod.structures.ShapeSpec(channels=Cm, stride=16)}).to(DEV).train()
    with torch.no_grad():      # the initial 0.01 / 0.001 predictor would leave the box gradient in the noise of the class one
        heads.box_predictor.bbox_pred.weight.normal_(std=0.05)
        heads.box_predictor.cls_score.weight.normal_(std=0.05)
        for conv in heads.box_head.convs:                    # GroupNorm off its (1, 0) initialisation
            if hasattr(conv, "norm"):
                conv.norm.weight.add_(torch.randn_like(conv.norm.weight) * 0.2)
                conv.norm.bias.add_(torch.randn_like(conv.norm.bias) * 0.2)
    return heads


def _scene(sfod, K, seed=12):
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(Bm, Cm, Hf, Wf, generator=g).to(DEV).requires_grad_(True)
    S = sfod.structures
    P = 40
    xy = torch.rand(Bm, P, 2, generator=g) * torch.tensor([Wimg * 0.7, Himg * 0.7])
    wh = torch.rand(Bm, P, 2, generator=g) * torch.tensor([Wimg * 0.3, Himg * 0.3]) + torch.tensor([0.4, 0.4])
    pboxes = torch.cat([xy, xy + wh], 2)
    targets = []
    for b in range(Bm):
        inst = S.Instances((Himg, Wimg))
        inst.gt_boxes = S.Boxes(pboxes[b, :5] + torch.randn(5, 4, generator=g) * 4)
        inst.gt_classes = torch.randint(0, K, (5,), generator=g)
        targets.append(inst)
    props = sfod.modeling.batched.BatchedProposals(pboxes.to(DEV), torch.zeros(Bm, P, device=DEV),
                                                   torch.tensor([P, P - 7], dtype=torch.int32, device=DEV), [(Himg, Wimg)] * Bm)
    return feat, props, targets


def _pooled64(feat, rois):
    """the oracle's ROIAlign (fp32 C code) on the rows of ``rois`` [n, 5] -> [n, C, 7, 7] float64; ``feat``: the device map
    (no graph) or a CPU fp32 leaf, whose gradient the composition then reaches"""
    f = feat if not feat.is_cuda else feat.detach().float().cpu()
    return om.roi_align(f, rois, 7, 1.0 / 16, 0, True).double()


@pytest.mark.parametrize("name,mode", MODULE_CASES, ids=[f"{h}-{m}" for h, m in MODULE_CASES])
def test_roi_heads_train_every_built_head(sfod, native, name, mode):
    nc, cd, nf, fd, norm = HEADS[name]
    heads = _build_heads(sfod, name, mode)
    assert heads._general and len(heads.box_head.convs) == nc and len(heads.box_head.fcs) == nf
    K = heads.num_classes
    feat, props, targets = _scene(sfod, K)
    samples, losses, _, _ = heads(None, {"vgg4": feat}, props, targets)
    (losses["loss_cls"] * 0.7 + losses["loss_box_reg"] * 1.3).backward()
    torch.cuda.synchronize()
    rois, cls = samples["rois"].cpu(), samples["gt_cls"].cpu().long()
    valid = cls >= 0
    assert int(valid.sum()) == int(samples["n_valid"].item()) and int(((cls >= 0) & (cls < K)).sum()) >= 8
    ocfg = om.Cfg(pooler_res=7, stride=16, feat_channels=Cm, fc_dim=fd)
    f32 = feat.detach().float().cpu().requires_grad_(True)
    pooled = _pooled64(f32, rois[valid])
    sd64 = om.clone_state({"roi_heads." + k: v.detach().double().cpu() for k, v in heads.state_dict().items()}, requires_grad=True)
    s64, d64, _ = bd.box_head_forward(sd64, pooled, nc, nf, norm)
    ref = om.fast_rcnn_losses(s64, d64, rois[valid, 1:5].double(), cls[valid], samples["gt_box"].cpu()[valid].double(), ocfg)
    (ref["loss_cls"] * 0.7 + ref["loss_box_reg"] * 1.3).backward()
    with torch.no_grad():
        sd32 = {k: v.detach().float() for k, v in sd64.items()}
        s32, d32, _ = bd.box_head_forward(sd32, pooled.detach().float(), nc, nf, norm)
        ref32 = om.fast_rcnn_losses(s32, d32, rois[valid, 1:5], cls[valid], samples["gt_box"].cpu()[valid], ocfg)
    for k in ("loss_cls", "loss_box_reg"):
        gate, e32 = D.gate(ref[k].detach(), ref32[k].detach(), ref[k].item())
        if mode != "fp32":
            gate = 1e-4 * ref[k].item()
        dist = abs(losses[k].item() - ref[k].item())
        print(f"[box head module {name} {mode}] {k}: float64 {ref[k].item():.9g} torch32 {e32:.3e} device {dist:.3e} gate {gate:.3e}")
        assert ref[k].item() > 1e-3 and dist <= gate, (k, dist, gate)
    params = dict(heads.named_parameters())
    assert len(params) == nc * (3 if norm else 2) + 2 * nf + 4
    for pname, p in params.items():
        want = sd64["roi_heads." + pname].grad
        rel = dc.rel_err(p.grad.cpu(), want)
        print(f"[box head module {name} {mode}] {pname}.grad {tuple(p.shape)}: relative L2 {rel:.3e} (gate 2e-3)")
        assert want.abs().sum() > 0 and rel <= 2e-3, pname
    rel = dc.rel_err(feat.grad.cpu(), f32.grad)        # the first layer's data gradient (rot180 weights) and the ROIAlign backward
    print(f"[box head module {name} {mode}] feature-map gradient: relative L2 {rel:.3e} (gate 2e-3)")
    assert f32.grad.abs().sum() > 0 and rel <= 2e-3
    # eval-mode inference runs the same pass
    heads.eval()
    with torch.no_grad():
        _, pred = heads._inference(feat.detach(), props)
    assert tuple(pred.shape)[0] == Bm * 40 and bool(torch.isfinite(pred).all())


def test_instance_level_domain_loss_through_a_one_fc_gn_head(sfod, native):
    """``dc_ins_loss`` (ROIAlign -> box head -> gradient reversal -> DAInsHead -> BCE) with the (2, 64, 1, 128, GN) head in fp32,
    dropout off: the loss under the module gate, the head's parameter gradients -- which ``_DCInsLossFn`` now takes as a list
    in ``box_head.parameters()`` order -- 2e-3 relative L2 against the float64 composition (reversed sign: the GRL)."""
    dann = importlib.import_module("simple-sfod_amd.modeling.dann")
    heads = _build_heads(sfod, "2conv1fc-gn", "fp32", seed=21)
    torch.manual_seed(22)
    ins = dann.DAInsHead(128, ["vgg4"], compute_dtype=torch.float32).to(DEV)
    with torch.no_grad():
        for p in ins.parameters():
            if p.dim() == 2:
                p.normal_(std=0.05)
    feat, props, _ = _scene(sfod, heads.num_classes, seed=23)
    rois = native.make_rois(props.boxes, props.count)
    loss = dann.dc_ins_loss(heads, ins, feat, rois, 1.0, training=False)
    loss.backward()
    torch.cuda.synchronize()
    r = rois.cpu()
    live = r[:, 0] >= 0
    assert int(live.sum()) == 73 and int((~live).sum()) >= 2
    sd64 = om.clone_state({"roi_heads." + k: v.detach().double().cpu() for k, v in heads.state_dict().items()}, requires_grad=True)
    _, _, x = bd.box_head_forward(sd64, _pooled64(feat, r[live]), 2, 1, "GN")
    w = {k: v.detach().double().cpu() for k, v in ins.state_dict().items()}
    lv = "_level_vgg4."
    x = torch.relu(F.linear(x, w["da_ins_fc1" + lv + "weight"], w["da_ins_fc1" + lv + "bias"]))
    x = torch.relu(F.linear(x, w["da_ins_fc2" + lv + "weight"], w["da_ins_fc2" + lv + "bias"]))
    zl = F.linear(x, w["da_ins_fc3" + lv + "weight"], w["da_ins_fc3" + lv + "bias"])[:, 0]
    ref = F.binary_cross_entropy_with_logits(zl, torch.ones_like(zl))
    ref.backward()
    print(f"[box head instance branch] loss: float64 {ref.item():.9g} device {loss.item():.9g}")
    np.testing.assert_allclose(loss.item(), ref.item(), rtol=1e-5)
    for pname, p in heads.box_head.named_parameters():
        want = -sd64["roi_heads.box_head." + pname].grad
        rel = dc.rel_err(p.grad.cpu(), want)
        print(f"[box head instance branch] box_head.{pname}.grad: relative L2 {rel:.3e} (gate 2e-3)")
        assert want.abs().sum() > 0 and rel <= 2e-3, pname


SINK_CASES = [("2conv1fc-gn", "fp32"), ("2conv1fc-gn", "bf16x3"), ("1conv1fc", "fp32"), ("1conv1fc", "f16x3")]


@pytest.mark.parametrize("name,mode", SINK_CASES, ids=[f"{h}-{m}" for h, m in SINK_CASES])
def test_two_backward_passes_add_into_preallocated_gradients(sfod, native, name, mode):
    """What a trainer step does to the head: every parameter has a preallocated, NON-ZERO ``.grad`` (the flat-gradient sinks of
    ``native.grad_sink``), and two backward passes -- the ROI losses, then the instance-level domain loss behind the gradient
    reversal -- add into them.  So the into-sink branches of ``_box_head_backward_general`` run: ``group_norm_relu_bwd(accumulate)``
    into the GroupNorm sinks, ``unpack_fc_wgrad(accumulate=True)`` for the first flat layer, ``conv_weight_grad`` into the sink
    (directly for a 64 -> 64 layer, through the packed form behind the channel-padded input), each twice.
    Held, per parameter and for the feature map, as relative L2 of ``.grad`` minus what was there before:
      - against the SAME two passes on the same samples without sinks (autograd adds the returned gradients), every mode: the same
        launches with the same ReLU gates, so only the fp32 rounding of adding onto the earlier content differs -- at most
        4 u (|before| + |gradient|) per element, about 1e-6 relative here -- while an overwrite, a dropped pass or a wrong sign is off
        by O(1); gate 1e-4;
      - in fp32 also against the float64 composition of both losses (2e-3, the module cases' gate).  Not in the pair modes: there
        the operands' 2^-16 rounding moves a few pre-activations across zero, and in float64 that rounding ALONE moves these
        gradients by 1e-3 ... 2e-2 on scenes of this size (ReLU gates flip), so float64 is no reference for a sum
        of gradients at that level; the no-sink passes are, and the module cases hold them."""
    dann = importlib.import_module("simple-sfod_amd.modeling.dann")
    rh = importlib.import_module("simple-sfod_amd.modeling.roi_heads")
    nc, cd, nf, fd, norm = HEADS[name]
    heads = _build_heads(sfod, name, mode, seed=31)
    torch.manual_seed(32)
    ins = dann.DAInsHead(fd, ["vgg4"], compute_dtype=heads.compute_dtype).to(DEV)
    with torch.no_grad():
        for p in ins.parameters():
            if p.dim() == 2:
                p.normal_(std=0.05)
    K = heads.num_classes
    feat, props, targets = _scene(sfod, K, seed=33)
    samples = heads.label_and_sample_proposals(props, sfod.modeling.batched.BatchedGT.from_instances(targets, feat.device))
    g = torch.Generator().manual_seed(34)
    before = {pname: (torch.randn(p.shape, generator=g) * 0.01).to(DEV) for pname, p in heads.named_parameters()}

    def two_passes(sinks):
        feat.grad = None
        for pname, p in heads.named_parameters():
            p.grad = before[pname].clone() if sinks else None
            assert (native.grad_sink(p) is p.grad) if sinks else (native.grad_sink(p) is None)
        l_cls, l_box = rh._ROILossFn.apply(heads, feat, samples, *heads._params())
        (l_cls * 0.7 + l_box * 1.3).backward()
        ins_loss = dann.dc_ins_loss(heads, ins, feat, samples["rois"], 1.0, training=False)
        (ins_loss * 0.9).backward()
        torch.cuda.synchronize()
        out = {pname: p.grad.cpu().double() - (before[pname].cpu().double() if sinks else 0.0) for pname, p in heads.named_parameters()}
        out["feature map"] = feat.grad.cpu().double()
        return out, ins_loss.item()
    plain, _ = two_passes(False)
    added, ins_loss = two_passes(True)
    worst = {k: dc.rel_err(added[k], plain[k]) for k in plain}
    for k, v in worst.items():
        print(f"[box head sinks {name} {mode}] {k}: added into the sink against returned to autograd, relative L2 {v:.3e} (gate 1e-4)")
    assert all(float(v.abs().sum()) > 0 for v in plain.values()) and max(worst.values()) <= 1e-4, worst
    if mode != "fp32":
        return
    # ---- float64: both losses on the same rows, the instance loss behind the gradient reversal ----
    rois, cls = samples["rois"].cpu(), samples["gt_cls"].cpu().long()
    valid, live = cls >= 0, rois[:, 0] >= 0
    assert int(valid.sum()) >= 16 and int(live.sum()) >= int(valid.sum())
    ocfg = om.Cfg(pooler_res=7, stride=16, feat_channels=Cm, fc_dim=fd)
    f32 = feat.detach().float().cpu().requires_grad_(True)
    sd64 = om.clone_state({"roi_heads." + k: v.detach().double().cpu() for k, v in heads.state_dict().items()}, requires_grad=True)
    s64, d64, _ = bd.box_head_forward(sd64, _pooled64(f32, rois[valid]), nc, nf, norm)
    ref = om.fast_rcnn_losses(s64, d64, rois[valid, 1:5].double(), cls[valid], samples["gt_box"].cpu()[valid].double(), ocfg)
    _, _, x = bd.box_head_forward(sd64, _pooled64(f32, rois[live]), nc, nf, norm)
    x = dann.gradient_scalar(x, -1.0)
    w = {k: v.detach().double().cpu() for k, v in ins.state_dict().items()}
    lv = "_level_vgg4."
    x = torch.relu(F.linear(x, w["da_ins_fc1" + lv + "weight"], w["da_ins_fc1" + lv + "bias"]))
    x = torch.relu(F.linear(x, w["da_ins_fc2" + lv + "weight"], w["da_ins_fc2" + lv + "bias"]))
    zl = F.linear(x, w["da_ins_fc3" + lv + "weight"], w["da_ins_fc3" + lv + "bias"])[:, 0]
    ref_ins = F.binary_cross_entropy_with_logits(zl, torch.ones_like(zl))
    (ref["loss_cls"] * 0.7 + ref["loss_box_reg"] * 1.3 + ref_ins * 0.9).backward()
    np.testing.assert_allclose(ins_loss, ref_ins.item(), rtol=1e-5)
    want = {pname: sd64["roi_heads." + pname].grad for pname in before}
    want["feature map"] = f32.grad
    worst = {k: dc.rel_err(added[k], want[k]) for k in want}
    for k, v in worst.items():
        print(f"[box head sinks {name} {mode}] {k}: added into the sink against float64, relative L2 {v:.3e} (gate 2e-3)")
    assert all(float(v.abs().sum()) > 0 for v in want.values()) and max(worst.values()) <= 2e-3, worst


# ---- step level ------------------------------------------------------------------------------------------------------------
def test_two_deterministic_steps_with_the_gn_head_are_reproducible_and_move_every_head_parameter(sfod, native):
    """The source-free trainer on the synthetic data set at 256 x 384, (2, 64, 1, 128, GN) head, bf16x3, SFOD.DETERMINISTIC, the
    domain branch live (ELIDE_DEAD_BRANCHES False, instance level on): two steps, twice -> bit-identical state and losses, finite
    losses, and every box-head parameter (``conv*.norm.*`` included) moved in the student and, through the EMA, in the teacher."""
    Bs, Hs, Ws = 2, 256, 384

    def run():
        cfg = sfod.config.setup_cfg(HOT_YAML, [
            "OUTPUT_DIR", "", "SOLVER.IMS_PER_BATCH_TARGET", str(Bs), "SFOD.SYNTHETIC.HEIGHT", str(Hs), "SFOD.SYNTHETIC.WIDTH", str(Ws),
            "SFOD.SYNTHETIC.NUM_IMAGES", "8", "INPUT.MIN_SIZE_TRAIN", f"({Hs},)", "SOLVER.WARMUP_ITERS", "0", "SOLVER.BASE_LR", "0.01",
            "SOLVER.CHECKPOINT_PERIOD", "0", "TEST.EVAL_PERIOD", "0", "TEST.VAL_LOSS", "False", "SFOD.EVAL_HOOK", "False",
            "WEAK_STRONG_AUGMENT", "False", "SFOD.DETERMINISTIC", "True", "SEMISUPNET.EMA_KEEP_RATE", "0.5",
            "SFOD.ELIDE_DEAD_BRANCHES", "False", "DOMAIN_CLASSIFIER.ENABLED", "True", "DOMAIN_CLASSIFIER.INSTANCE", "True"]
            + _head_opts("2conv1fc-gn"))
        torch.manual_seed(5)
        tr = sfod.engine.SourceFreeAdaptiveTeacherTrainer(cfg)
        assert tr.model.roi_heads._general
        with torch.no_grad():
            tr.model.roi_heads.box_predictor.cls_score.weight.mul_(30.0)
            tr._copy_main_model()
        g = torch.Generator().manual_seed(1)
        tr.model.proposal_generator._forced_keys = torch.randint(0, 2 ** 31 - 1, (Bs, (Hs // 32) * (Ws // 32) * 15), generator=g).to(torch.int32).to(DEV)
        tr.model.roi_heads._forced_keys = torch.randint(0, 2 ** 31 - 1, (Bs, 2100), generator=g).to(torch.int32).to(DEV)
        before = {w: {k: v.detach().clone() for k, v in m.named_parameters() if "roi_heads.box_head." in k}
                  for w, m in (("student", tr.model), ("teacher", tr.model_teacher))}
        losses = []
        for it in range(2):
            tr.iter = it
            tr.run_step()
            tr.scheduler.step()
            rec = tr.storage.flush()
            losses.append({k: rec[k] for k in sorted(rec) if k.startswith("loss")})
        torch.cuda.synchronize()
        after = {w: {k: v.detach().clone() for k, v in m.named_parameters() if "roi_heads.box_head." in k}
                 for w, m in (("student", tr.model), ("teacher", tr.model_teacher))}
        state = [tr.optimizer.flat.param.clone(), tr.optimizer.mom.clone(), tr.teacher_flat.param.clone()]
        del tr
        torch.cuda.empty_cache()
        return state, losses, before, after

    try:
        (a, la, before, after), (b, lb, _, _) = run(), run()
    finally:
        native.set_deterministic(False)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"state tensor {i} differs between two runs"
    assert la == lb and all(np.isfinite(v) for rec in la for v in rec.values()), la
    assert any(k.startswith("loss_DC_ins") for k in la[0]), sorted(la[0])
    names = sorted(before["student"])
    assert len(names) == 2 * 3 + 2 and sum(".norm." in k for k in names) == 4
    for who in ("student", "teacher"):
        for k in names:
            assert not torch.equal(before[who][k], after[who][k]), f"{who} {k} did not move"
