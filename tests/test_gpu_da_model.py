"""DA Faster R-CNN on the device: ``DAImgHead``, the per-domain function of modeling/da_faster_rcnn.py against the reference's
recorded values (tests/golden/da_ref.npz, tools/record_da_golden.py; inputs: tests/helpers/da_cases.py), one ``DATrainer``
step, and ``sample_unlabeled_proposals``.  Mode: fp32; the per-domain function also in bf16x3, f16x3 and bf16 (losses only).

Tolerances are the ones the existing GPU tests of the same kernels and mode use (tests/test_gpu_model.py): the image-level
discriminator's forward 2e-5 and gradients 1e-4 (``test_dc_img_loss_backward_matches_reference_golden`` and the forward
test above it), the ROIAlign -> box head -> DAInsHead chain's losses 2e-5 and gradients 2e-4
(``test_dc_ins_loss_backward_matches_a_torch_restatement``); relative error in the 2-norm, over the recorded elements.
"""
import os
from importlib import import_module

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import da_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
DA_YAML = os.path.join(os.path.dirname(GOLDEN), "..", "configs", "faster_rcnn_VGG_cityscapes_foggy_da.yaml")
LEVEL = "vgg4"


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "da_ref.npz"), allow_pickle=False)


def make_cfg(sfod, *opts):
    return sfod.config.setup_cfg(DA_YAML, ["OUTPUT_DIR", "", "SFOD.COMPUTE_DTYPE", "fp32"] + list(opts))      # (later options win)


def recorded(fx, keys, numel):
    """sum of the recorded tensors ``keys`` at the recorded positions -> (values, positions)"""
    idx = C.probe_indices(numel)
    tot = torch.zeros(len(idx), dtype=torch.float64)
    for k in keys:
        tot += torch.from_numpy(fx[k] if k in fx.files else fx[k + "@probe"]).reshape(-1)
    return tot, idx


def rel_err(t, fx, keys):
    t = t.detach().double().cpu().reshape(-1)
    ref, idx = recorded(fx, keys, t.numel())
    return ((t[idx] - ref).norm() / (ref.norm() + 1e-300)).item()


def case_model(sfod, dtype):
    """the DA yaml's model in arithmetic mode ``dtype`` with the model case's box head and domain heads"""
    mc = C.model_case()
    torch.manual_seed(0)
    m = sfod.modeling.build_model(make_cfg(sfod, "SFOD.COMPUTE_DTYPE", dtype)).train()
    c1, c2 = m.DC_img.convs()
    fcs = sfod.modeling.dann.ins_head_layers(m.DC_ins)
    bh = m.roi_heads.box_head
    with torch.no_grad():
        for mod, w, name in [(c1, mc["w_img"], "conv1"), (c2, mc["w_img"], "conv2"), (fcs[0], mc["w_ins"], "fc1"),
                             (fcs[1], mc["w_ins"], "fc2"), (fcs[2], mc["w_ins"], "fc3"), (bh.fc1, mc["w_box"], "fc1"),
                             (bh.fc2, mc["w_box"], "fc2")]:
            mod.weight.copy_(w[name + ".weight"].float())
            mod.bias.copy_(w[name + ".bias"].float())
    return m


@pytest.fixture(scope="module")
def model(sfod, native):
    return case_model(sfod, "fp32")


def test_da_img_head_matches_the_recorded_reference(sfod, native, model, fx):
    mc = C.model_case()
    head = model.DC_img
    feat = mc["feat"].float().to(DEV)
    y = head({LEVEL: feat})[LEVEL]
    assert tuple(y.shape) == (2, 1, 5, 7) and y.dtype == torch.float32
    assert rel_err(y, fx, ["img_head_model/out"]) < 2e-5
    x = native.nhwc_operand(feat, head.compute_dtype)
    h1, z = head.logits(x)
    assert torch.equal(z[..., 0], y[:, 0]) and (z[..., 1:] == 0).all()
    dz = torch.zeros_like(z)
    dz[..., 0] = torch.from_numpy(fx["img_head_model/upstream"]).float().to(DEV)[:, 0]
    dx, grads = head.grads(x, h1, dz, dz)
    assert rel_err(dx.permute(0, 3, 1, 2), fx, ["img_head_model/g/feat"]) < 1e-4
    for g, name in zip(grads, ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias")):
        assert rel_err(g, fx, ["img_head_model/g/w_img/" + name]) < 1e-4, name


def run_domain(sfod, model, weights, label, which=("img", "ins", "cons"), masks=True):
    """one domain of the model case through ``_DADomainFn`` (target side: no detection loss), backward of the sum of the
    losses in ``which`` -> (losses, feature gradient, box-feature gradient handed to the box head, parameter gradients)"""
    F = sfod.modeling.da_faster_rcnn
    O = import_module("simple-sfod_amd.modeling.da_options")
    mc = C.model_case()
    model.da = O.DAOptions(LEVEL, *weights)
    for p in model.parameters():
        p.grad = None
    feat = mc["feat"].float().to(DEV).requires_grad_(True)
    m = [[t.to(DEV) for t in pair] for pair in mc["masks"]] if masks else None
    rh = model.roi_heads
    seen = {}
    orig = rh._box_head_backward

    def spy(st, rois, dh):
        seen["dbf"] = dh.detach().clone()
        return orig(st, rois, dh)
    rh._box_head_backward = spy
    try:
        out = F.da_domain_losses(model, feat, {"rois": mc["rois"].to(DEV)}, False, label, m)
        losses = dict(zip(("cls", "box", "img", "ins", "cons"), out))
        sum(losses[k] for k in which).backward()
    finally:
        del rh._box_head_backward
    c1, c2 = model.DC_img.convs()
    fcs = sfod.modeling.dann.ins_head_layers(model.DC_ins)
    bh = rh.box_head
    grads = {"w_img/conv1": c1, "w_img/conv2": c2, "w_ins/fc1": fcs[0], "w_ins/fc2": fcs[1], "w_ins/fc3": fcs[2],
             "w_box/fc1": bh.fc1, "w_box/fc2": bh.fc2}
    pg = {f"{k}.{p}": getattr(mod, p).grad.detach().clone() for k, mod in grads.items() for p in ("weight", "bias")}
    return losses, feat.grad.detach().clone(), seen["dbf"], pg


@pytest.mark.parametrize("run", C.MODEL_RUNS, ids=lambda r: "w{}-l{}".format(*r))
def test_domain_function_matches_the_recorded_reference(sfod, native, model, fx, run):
    k, label = run
    losses, dfeat, dbf, pg = run_domain(sfod, model, C.WEIGHT_SETS[k], label)
    prefix = f"model/w{k}/l{label}/train"
    assert losses["cls"].item() == 0.0 and losses["box"].item() == 0.0 and not losses["cls"].requires_grad
    for which in ("img", "ins", "cons"):
        ref = float(fx[f"{prefix}/{which}/value"])
        print(f"{prefix}/{which}: device {losses[which].item():.9g} recorded {ref:.9g}")
        np.testing.assert_allclose(losses[which].item(), ref, rtol=2e-5, err_msg=which)
    every = [f"{prefix}/{w}/g/" for w in ("img", "ins", "cons")]
    has = lambda key: key in fx.files or key + "@probe" in fx.files
    figures = {"feat": rel_err(dfeat, fx, [p + "feat" for p in every]),
               "box_features": rel_err(dbf, fx, [p + "box_features" for p in every if has(p + "box_features")])}
    for name, g in pg.items():
        keys = [p + name for p in every if has(p + name)]
        assert keys, name
        figures[name] = rel_err(g, fx, keys)
    print({n: f"{v:.2e}" for n, v in figures.items()})
    for name, v in figures.items():
        assert v < 2e-4, (name, v)
    # the padding rows hand nothing to the box head
    assert (dbf.cpu()[C.model_case()["rois"][:, 0] < 0] == 0).all()


# Loss gates of the other arithmetic modes, from the number formats (the recorded values are float64):
#   bf16x3 / f16x3: operand pairs hold >= 16 significand bits and sums are fp32 -- the project's loss gate for these modes, 1e-4
#                   relative (README: "the VGG configs' 1e-4-gated mode");
#   bf16:           every stored activation is rounded to 8 significand bits (2^-9 relative); six stored layers lie between the
#                   features and an instance logit (ROIAlign, fc1, fc2, and the head's three), each logit is at most ~1 in magnitude
#                   here and d loss / d logit <= 1: 6 x 2^-9 = 1.2e-2 absolute, doubled for the operands' own rounding: 2.4e-2.
MODE_GATES = {"bf16x3": ("rtol", 1e-4), "f16x3": ("rtol", 1e-4), "bf16": ("atol", 2.4e-2)}


@pytest.mark.parametrize("dtype", sorted(MODE_GATES))
def test_domain_function_runs_in_every_compute_dtype(sfod, native, fx, dtype):
    k, label = C.MODEL_RUNS[1]
    losses, dfeat, dbf, pg = run_domain(sfod, case_model(sfod, dtype), C.WEIGHT_SETS[k], label)
    prefix = f"model/w{k}/l{label}/train"
    kind, tol = MODE_GATES[dtype]
    for which in ("img", "ins", "cons"):
        ref = float(fx[f"{prefix}/{which}/value"])
        err = abs(losses[which].item() - ref)
        print(f"{dtype} {which}: device {losses[which].item():.9g} recorded {ref:.9g} abs err {err:.3e} rel {err / abs(ref):.3e}")
        assert err <= (tol * abs(ref) if kind == "rtol" else tol), (dtype, which, err)
    every = [f"{prefix}/{w}/g/feat" for w in ("img", "ins", "cons")]
    print(f"{dtype} feature gradient: relative error {rel_err(dfeat, fx, every):.3e} (reported)")
    assert torch.isfinite(dfeat).all() and float(dfeat.abs().max()) > 0 and torch.isfinite(dbf.float()).all()
    assert all(torch.isfinite(g).all() and float(g.abs().max()) > 0 for g in pg.values())


def test_gradient_reversal_structure(sfod, native, model):
    """w_c = 0: the feature gradient of the image-level loss is -w_i times the un-reversed one (w_i = 1/4 scales every
    intermediate exactly).  w_i = w_n = 0: every backbone and box-head gradient of the domain terms is exactly zero while
    the domain heads' own gradients are not."""
    _, g_rev, _, _ = run_domain(sfod, model, (0.25, 0.0, 0.0), 1, which=("img",))
    _, g_fwd, _, _ = run_domain(sfod, model, (-1.0, 0.0, 0.0), 1, which=("img",))
    assert float(g_fwd.abs().max()) > 0
    assert torch.equal(g_rev, -0.25 * g_fwd)
    _, dfeat, dbf, pg = run_domain(sfod, model, (0.0, 0.0, 1.0), 0)
    assert (dfeat == 0).all() and (dbf == 0).all()
    for name, g in pg.items():
        if name.startswith("w_box/"):
            assert (g == 0).all(), name
        else:
            assert float(g.abs().max()) > 0, name


def test_eval_mode_uses_one_instance_head_evaluation(sfod, native, model):
    """without masks the instance-level and the consistency term read the same logits: the losses are finite, differ from
    the training-mode ones, and a backward works"""
    train, *_ = run_domain(sfod, model, C.WEIGHT_SETS[0], 1)
    ev, dfeat, _, pg = run_domain(sfod, model, C.WEIGHT_SETS[0], 1, masks=False)
    assert ev["img"].item() == train["img"].item()
    assert all(np.isfinite(ev[k].item()) for k in ("ins", "cons")) and ev["ins"].item() != train["ins"].item()
    assert torch.isfinite(dfeat).all() and float(dfeat.abs().max()) > 0 and float(pg["w_ins/fc2.weight"].abs().max()) > 0


# ---- sampling ------------------------------------------------------------------------------------------------------------------
def test_sample_unlabeled_proposals_takes_the_smallest_keys(sfod, native):
    B, P, S = 2, 40, 16
    cfg = make_cfg(sfod, "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", str(S))
    torch.manual_seed(0)
    rh = sfod.modeling.build_model(cfg).roi_heads.train()
    Bt = import_module("simple-sfod_amd.modeling.batched")
    g = torch.Generator().manual_seed(5)
    xy = torch.rand(B, P, 2, generator=g) * 100
    boxes = torch.cat([xy, xy + 10 + torch.rand(B, P, 2, generator=g) * 50], -1)
    count = torch.tensor([P, 7], dtype=torch.int32)
    keys = torch.randint(0, 2 ** 31 - 1, (B, P), generator=g).to(torch.int32)
    props = Bt.BatchedProposals(boxes.to(DEV), torch.zeros(B, P, device=DEV), count.to(DEV), [(160, 224)] * B)
    rh._forced_keys_unlabeled = keys.to(DEV)
    sm = rh.sample_unlabeled_proposals(props)
    assert sm["count"].tolist() == [S, 7] and tuple(sm["rois"].shape) == (B * S, 5)
    rois, idx, cls = sm["rois"].cpu(), sm["sampled_idxs"].cpu(), sm["gt_cls"].cpu()
    for b, n in enumerate([S, 7]):
        live = int(count[b])
        want = sorted(torch.argsort(keys[b, :live].long() * P + torch.arange(live))[:n].tolist())      # smallest (key, index)
        assert idx[b, :n].tolist() == want
        rows = rois[b * S: b * S + n]
        assert (rows[:, 0] == b).all() and torch.equal(rows[:, 1:], boxes[b][want])
        assert (rois[b * S + n: (b + 1) * S, 0] == -1).all()
        assert (cls[b * S: b * S + n] == rh.num_classes).all() and (cls[b * S + n: (b + 1) * S] == -1).all()
    # the keys argument, like label_and_sample_proposals'
    sm2 = rh.sample_unlabeled_proposals(props, keys=keys.to(DEV))
    assert torch.equal(sm2["rois"], sm["rois"])


# ---- one trainer step ------------------------------------------------------------------------------------------------------------
LOSS_KEYS = ("loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc", "loss_DC_img", "loss_DC_ins", "loss_DC_consistency")


def one_step(sfod):
    cfg = make_cfg(sfod, "SOLVER.IMS_PER_BATCH", "2", "SOLVER.IMS_PER_BATCH_TARGET", "2", "SFOD.SYNTHETIC.HEIGHT", "64",
                   "SFOD.SYNTHETIC.WIDTH", "96", "SFOD.SYNTHETIC.NUM_IMAGES", "4", "INPUT.MIN_SIZE_TRAIN", "(64,)",
                   "SOLVER.CHECKPOINT_PERIOD", "0", "SFOD.DETERMINISTIC", "True")
    torch.manual_seed(cfg.SEED)
    tr = sfod.engine.get_trainer_class(cfg)(cfg)
    assert type(tr) is sfod.engine.DATrainer and tr._reducer is None
    m = tr.model
    g = torch.Generator().manual_seed(9)
    P = m.proposal_generator.post_nms_topk[True]
    S = m.roi_heads.batch_size_per_image
    key = lambda *shape: torch.randint(0, 2 ** 31 - 1, shape, generator=g).to(torch.int32).to(DEV)
    m.proposal_generator._forced_keys = key(2, 2 * 3 * m.proposal_generator.num_anchors)
    m.roi_heads._forced_keys = key(2, P + 100)
    m.roi_heads._forced_keys_unlabeled = key(2, P)
    m._forced_masks = {k: [(torch.rand(2 * S, 1024, generator=g) >= 0.5).to(torch.uint8).to(DEV) for _ in range(2)]
                       for k in sfod.modeling.da_faster_rcnn.MASK_ORDER}
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    tr.run_step()
    rec = tr.storage.flush()
    torch.cuda.synchronize()
    return tr, before, rec


def test_one_da_trainer_step(sfod, native):
    tr, before, rec = one_step(sfod)
    assert {k for k in rec if k.startswith("loss")} == set(LOSS_KEYS)
    for k in LOSS_KEYS:
        assert np.isfinite(float(rec[k])), (k, rec[k])
    assert 0.3 < float(rec["loss_DC_img"]) < 1.2 and 0.3 < float(rec["loss_DC_ins"]) < 1.2          # ~ln 2 at initialisation
    assert 0.0 <= float(rec["loss_DC_consistency"]) < 0.5
    after = dict(tr.model.named_parameters())
    moved = {n for n, p in after.items() if not torch.equal(before[n], p.detach())}
    for prefix in ("backbone.", "proposal_generator.", "roi_heads.box_head.", "roi_heads.box_predictor.", "DC_img.", "DC_ins."):
        assert any(n.startswith(prefix) for n in moved), prefix
    # a second identical run under SFOD.DETERMINISTIC gives the same bits
    tr2, _, rec2 = one_step(sfod)
    for (n, p), (n2, p2) in zip(tr.model.named_parameters(), tr2.model.named_parameters()):
        assert n == n2 and torch.equal(p.detach(), p2.detach()), n
    assert all(float(rec[k]) == float(rec2[k]) for k in LOSS_KEYS)
    # a list input: source only, exactly the four detection losses
    src, _ = next(iter(tr.data_loader))
    losses = tr.model(src)
    assert set(losses) == {"loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc"}
    assert all(torch.isfinite(v) for v in losses.values())
