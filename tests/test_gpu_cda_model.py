"""Conditional DA Faster R-CNN on the device: the per-domain function of modeling/cda_faster_rcnn.py against the reference's
recorded values (tests/golden/cda_ref.npz, tools/record_cda_golden.py; inputs: tests/helpers/cda_cases.py), the model's
``forward`` and one ``DATrainer`` step.  Mode: fp32; the per-domain function also in bf16x3 and f16x3.

Gate of the fp32 comparison (relative error in the 2-norm over the recorded elements, the measure of tests/test_gpu_da_model.py):
it starts at 1e-6.  fc1 of the conditioned head sums 9216 terms, nine times the DA head's, so where 1e-6 is out of reach of fp32
arithmetic itself the gate is not a chosen number: the float64 definition (tests/helpers/cda_definitions.py) is evaluated by
torch in fp32 on the CPU, and the gate is 4 x its distance from the recorded value.  Every case prints the device's and
torch-fp32's distances (profiles/cda_faster.txt holds a run).  bf16x3 / f16x3: the margins those modes have in
tests/test_gpu_da_model.py (losses 1e-4 relative; gradients finite, non-zero and reported).
"""
import functools
import os
from importlib import import_module

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import cda_cases as C
from helpers import cda_definitions as CD
from helpers import da_definitions as D

pytestmark = pytest.mark.gpu
DEV = "cuda"
CDA_YAML = os.path.join(os.path.dirname(GOLDEN), "..", "configs", "faster_rcnn_VGG_cityscapes_foggy_cda.yaml")
LEVEL = "vgg4"
BASE_GATE = 1e-6
WHICH = ("img", "ins", "cons")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "cda_ref.npz"), allow_pickle=False)


def make_cfg(sfod, *opts):
    return sfod.config.setup_cfg(CDA_YAML, ["OUTPUT_DIR", "", "SFOD.COMPUTE_DTYPE", "fp32"] + list(opts))      # (later options win)


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


def has(fx, key):
    return key in fx.files or key + "@probe" in fx.files


def case_model(sfod, dtype):
    """the CDA yaml's model in arithmetic mode ``dtype`` with the model case's box head and domain heads"""
    mc = C.model_case()
    torch.manual_seed(0)
    m = sfod.modeling.build_model(make_cfg(sfod, "SFOD.COMPUTE_DTYPE", dtype)).train()
    assert type(m) is sfod.modeling.cda_faster_rcnn.CDAFasterRCNN
    c1, c2 = m.DC_img.convs()
    fcs = sfod.modeling.dann.ins_head_layers(m.DC_ins)
    assert tuple(fcs[0].weight.shape) == (1024, 9216)
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


def run_domain(sfod, model, weights, label, entropy, which=WHICH, masks=True, scores=None):
    """one domain of the model case through ``_CDADomainFn`` (target side: no detection loss) conditioned on the case's class
    logits, backward of the sum of the losses in ``which`` -> (losses, feature gradient, box-feature gradient handed to the box
    head, parameter gradients)"""
    F = sfod.modeling.cda_faster_rcnn
    O = import_module("simple-sfod_amd.modeling.da_options")
    mc = C.model_case()
    model.da = O.DAOptions(LEVEL, *weights, conditional=True, entropy_conditioning=entropy)
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
        sc = (mc["scores"] if scores is None else scores).to(DEV)
        out = F.cda_domain_losses(model, feat, {"rois": mc["rois"].to(DEV)}, False, label, m, scores=sc)
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


@functools.lru_cache(maxsize=None)
def torch_fp32(run):
    """the float64 definition evaluated by torch in fp32 on the CPU -> ({which: loss}, {leaf: summed gradient}); never modified"""
    k, label, ent, mode = run
    mc = C.model_case()
    pooler = C.POOLERS[0]
    leaf = lambda t: t.float().clone().requires_grad_(True)
    feat = leaf(mc["feat"])
    w_box, w_img, w_ins = ({n: leaf(v) for n, v in mc[key].items()} for key in ("w_box", "w_img", "w_ins"))
    rois = mc["rois"]
    live = torch.nonzero(rois[:, 0] >= 0).flatten()
    bf_live = D.box_head(feat, rois[live], w_box, pooler[0], 1.0 / C.STRIDE, pooler[1], pooler[2])
    bf = torch.zeros(C.N_ROWS, bf_live.shape[1]).index_copy(0, live, bf_live)
    bf.retain_grad()
    res = CD.evaluate_losses(feat, bf, mc["scores"], rois, w_img, w_ins, C.WEIGHT_SETS[k], label, pooler, ent,
                             mc["masks"] if mode == "train" else None, pool="oracle",
                             extra_leaves={"w_box/" + n: v for n, v in w_box.items()})
    total = {}
    for which, (_, grads) in res.items():
        for n, g in grads.items():
            total[n] = total.get(n, 0) + g.double()
    return {w: v.item() for w, (v, _) in res.items()}, total


def gate_of(e32):
    return max(BASE_GATE, 4.0 * e32)


@pytest.mark.parametrize("run", C.RUNS, ids=lambda r: C.run_name(*r).replace("/", "-"))
def test_domain_function_matches_the_recorded_reference(sfod, native, model, fx, run):
    k, label, ent, mode = run
    losses, dfeat, dbf, pg = run_domain(sfod, model, C.WEIGHT_SETS[k], label, ent, masks=(mode == "train"))
    l32, g32 = torch_fp32(run)
    prefix = "model/" + C.run_name(*run)
    assert losses["cls"].item() == 0.0 and losses["box"].item() == 0.0 and not losses["cls"].requires_grad
    failures = []
    for which in WHICH:
        ref = float(fx[f"{prefix}/{which}/value"])
        dev, e32 = abs(losses[which].item() - ref) / abs(ref), abs(l32[which] - ref) / abs(ref)
        print(f"{prefix}/{which}: device {losses[which].item():.9g} recorded {ref:.9g} rel {dev:.3e} torch32 {e32:.3e} gate {gate_of(e32):.3e}")
        if dev > gate_of(e32):
            failures.append((which, dev, gate_of(e32)))
    every = [f"{prefix}/{w}/g/" for w in WHICH]
    tensors = {"feat": dfeat, "box_features": dbf, **pg}
    for name, t in tensors.items():
        keys = [p + name for p in every if has(fx, p + name)]
        assert keys, name
        dev, e32 = rel_err(t, fx, keys), rel_err(g32[name], fx, keys)
        print(f"{prefix}/g/{name}: device {dev:.3e} torch32 {e32:.3e} gate {gate_of(e32):.3e}")
        if dev > gate_of(e32):
            failures.append((name, dev, gate_of(e32)))
    assert not failures, failures
    # the padding rows (NaN logits) hand nothing to the box head
    assert (dbf.cpu()[C.model_case()["rois"][:, 0] < 0] == 0).all() and torch.isfinite(dfeat).all()


@pytest.mark.parametrize("dtype", ["bf16x3", "f16x3"])
def test_domain_function_runs_in_the_pair_modes(sfod, native, fx, dtype):
    run = (1, 1, True, "train")
    k, label, ent, _ = run
    losses, dfeat, dbf, pg = run_domain(sfod, case_model(sfod, dtype), C.WEIGHT_SETS[k], label, ent)
    native.check_f16x3_range(DEV)
    prefix = "model/" + C.run_name(*run)
    for which in WHICH:
        ref = float(fx[f"{prefix}/{which}/value"])
        err = abs(losses[which].item() - ref)
        print(f"{dtype} {which}: device {losses[which].item():.9g} recorded {ref:.9g} rel {err / abs(ref):.3e}")
        assert err <= 1e-4 * abs(ref), (dtype, which, err)
    every = [f"{prefix}/{w}/g/feat" for w in WHICH]
    print(f"{dtype} feature gradient: relative error {rel_err(dfeat, fx, every):.3e} (reported)")
    print(f"{dtype} DC_ins fc1 weight gradient: relative error "
          f"{rel_err(pg['w_ins/fc1.weight'], fx, [f'{prefix}/{w}/g/w_ins/fc1.weight' for w in ('ins', 'cons')]):.3e} (reported)")
    assert torch.isfinite(dfeat).all() and float(dfeat.abs().max()) > 0 and torch.isfinite(dbf.float()).all()
    assert all(torch.isfinite(g).all() and float(g.abs().max()) > 0 for g in pg.values())


def test_uniform_scores_make_the_entropy_weights_a_no_op(sfod, native, model):
    """every score row equal: p is uniform, the entropy weights are equal, and after the normalisation by their mean the
    weighted instance loss is the unweighted one.  Both are fp32 sums of 70 positive terms, each a few ulps from the exact value:
    the fp32 gate, 1e-6 relative."""
    sc = torch.full((C.N_ROWS, 9), -0.375)
    on, _, _, g_on = run_domain(sfod, model, C.WEIGHT_SETS[0], 1, True, scores=sc)
    off, _, _, g_off = run_domain(sfod, model, C.WEIGHT_SETS[0], 1, False, scores=sc)
    print(f"uniform scores: weighted {on['ins'].item():.9g} unweighted {off['ins'].item():.9g}")
    assert abs(on["ins"].item() - off["ins"].item()) <= BASE_GATE * abs(off["ins"].item())
    assert on["cons"].item() == off["cons"].item() and on["img"].item() == off["img"].item()
    a, b = g_on["w_ins/fc3.weight"], g_off["w_ins/fc3.weight"]
    assert float((a - b).norm() / b.norm()) <= 1e-5
    # and with the case's scores the weights do act
    on2, *_ = run_domain(sfod, model, C.WEIGHT_SETS[0], 1, True)
    off2, *_ = run_domain(sfod, model, C.WEIGHT_SETS[0], 1, False)
    assert abs(on2["ins"].item() - off2["ins"].item()) > 1e-5 * abs(off2["ins"].item())


def test_conditioning_reads_the_predictors_logits_by_default(sfod, native, model):
    """without ``scores`` the node conditions on st["pred"][:, :K + 1] of its own pass: the same losses as handing it those
    logits, and no gradient reaches the predictor (the condition is detached, the target side has no detection loss)"""
    F = sfod.modeling.cda_faster_rcnn
    O = import_module("simple-sfod_amd.modeling.da_options")
    mc = C.model_case()
    model.da = O.DAOptions(LEVEL, *C.WEIGHT_SETS[0], conditional=True, entropy_conditioning=True)
    for p in model.parameters():
        p.grad = None
    feat = mc["feat"].float().to(DEV).requires_grad_(True)
    rois = mc["rois"].to(DEV)
    rh = model.roi_heads
    a = F.cda_domain_losses(model, feat, {"rois": rois}, False, 1, None)
    pred = rh._box_forward(feat.detach(), rois)["pred"]
    b = F.cda_domain_losses(model, feat, {"rois": rois}, False, 1, None, scores=pred[:, : rh.num_classes + 1].contiguous())
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    sum(a[2:]).backward()
    bp = rh.box_predictor
    assert all(p.grad is None or float(p.grad.abs().max()) == 0.0 for p in (bp.cls_score.weight, bp.bbox_pred.weight))
    # CDAStandardROIHeads hands the same logits back, in the reference's return order
    Bt = import_module("simple-sfod_amd.modeling.batched")
    boxes = mc["rois"][mc["rois"][:, 0] == 0][:16, 1:].clamp(min=0)
    props = Bt.BatchedProposals(torch.stack([boxes, boxes]).to(DEV), torch.zeros(2, 16, device=DEV),
                                torch.tensor([16, 9], dtype=torch.int32, device=DEV), [(160, 224)] * 2)
    out = rh(None, {LEVEL: feat.detach()}, props)
    assert len(out) == 4
    samples, losses, box_features, box_scores = out
    assert losses == {} and box_features.shape[0] == samples["rois"].shape[0] == box_scores.shape[0]
    assert tuple(box_scores.shape[1:]) == (rh.num_classes + 1,) and tuple(box_features.shape[1:]) == (1024,)
    st = rh._box_forward(feat.detach(), samples["rois"])
    assert torch.equal(box_scores, st["pred"][:, : rh.num_classes + 1])


# ---- the model and one trainer step ----------------------------------------------------------------------------------------------
LOSS_KEYS = ("loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc", "loss_DC_img", "loss_DC_ins", "loss_DC_consistency")


def one_step(sfod):
    cfg = make_cfg(sfod, "SOLVER.IMS_PER_BATCH", "2", "SOLVER.IMS_PER_BATCH_TARGET", "2", "SFOD.SYNTHETIC.HEIGHT", "64",
                   "SFOD.SYNTHETIC.WIDTH", "96", "SFOD.SYNTHETIC.NUM_IMAGES", "4", "INPUT.MIN_SIZE_TRAIN", "(64,)",
                   "SOLVER.CHECKPOINT_PERIOD", "0", "SFOD.DETERMINISTIC", "True")
    torch.manual_seed(cfg.SEED)
    tr = sfod.engine.get_trainer_class(cfg)(cfg)
    assert type(tr) is sfod.engine.DATrainer and tr._reducer is None
    m = tr.model
    assert type(m) is sfod.modeling.cda_faster_rcnn.CDAFasterRCNN and m.da.entropy_conditioning
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


def test_one_cda_trainer_step(sfod, native):
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
    assert all(torch.isfinite(p).all() for p in after.values())
    # a second identical run under SFOD.DETERMINISTIC gives the same bits
    tr2, _, rec2 = one_step(sfod)
    for (n, p), (n2, p2) in zip(tr.model.named_parameters(), tr2.model.named_parameters()):
        assert n == n2 and torch.equal(p.detach(), p2.detach()), n
    assert all(float(rec[k]) == float(rec2[k]) for k in LOSS_KEYS)
    # the model itself: a (source, target) tuple gives the seven keys, a list alone the four detection losses
    src, tgt = next(iter(tr.data_loader))
    losses = tr.model((src, tgt))
    assert set(losses) == set(LOSS_KEYS) and all(torch.isfinite(v) for v in losses.values())
    losses = tr.model(src)
    assert set(losses) == {"loss_cls", "loss_box_reg", "loss_rpn_cls", "loss_rpn_loc"}
    assert all(torch.isfinite(v) for v in losses.values())
