"""Classification-loss options on the device: MODEL.ROI_HEADS.LOSS "FocalLoss" (SFOD.FOCAL_LOSS_GAMMA) and
MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE through the ``sfod_*_cls`` entry points (include/sfod_hip.h).

Reference: the definitions of tests/helpers/cls_loss_definitions.py (torch ops) in float64 on the CPU, autograd gradients.
Tolerance: the project's gate (tests/test_gpu_box_reg_options.py) -- per compared quantity the same definition is also
evaluated by torch in fp32 and the gate is 4 x max(torch-fp32's distance from float64, 2^-24 * s), s = the sum of absolute
terms (a loss) or the largest magnitude (a gradient or probability tensor); where torch's fp32 evaluation is not finite
(focal, gamma < 1, a saturated row: inf * 0) the floor alone.  No element is excluded.  Every case prints its figures; with
SFOD_CLS_LOSS_REPORT=<file> they are appended there (profiles/cls_loss_options.txt is such a run).  The module level has
its own gate: 4 x the distance the same harness measures with "CrossEntropy".
"""
import functools
import importlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import box_reg_definitions as BD
from helpers import cls_loss_definitions as D

from oracle import box_ops as OB
from oracle import model as om

pytestmark = pytest.mark.gpu
DEV = "cuda"
CONFIGS = os.path.join(os.path.dirname(GOLDEN), "..", "configs")
HOT_YAML = os.path.join(CONFIGS, "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free.yaml")
FOCAL_YAML = os.path.join(CONFIGS, "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free_focal.yaml")
SEED = 3           # the first seed from 1 upwards at which no sigmoid probability of the candidates case lies within 1e-5 of the
#                    score threshold 0.05 or of 0.5 (asserted in float64 before anything is compared)
ROI_W = (10.0, 10.0, 5.0, 5.0)
GS = (0.7, 1.3)
GS32 = tuple(float(torch.tensor(v, dtype=torch.float32)) for v in GS)      # what the kernel reads
RR, RLIVE, NPLANT = 300, 250, 8
SCORE_THRESH = 0.05


def report(line):
    print(line)
    path = os.environ.get("SFOD_CLS_LOSS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def cls_opts(native, kind, gamma=1.5):
    return native.ClsLossOptions("FocalLoss" if kind == "focal" else "CrossEntropy", gamma, kind == "sigmoid")


# ---- loss inputs: R = 300 (250 live rows, the rest -1: two blocks, the second partial) ---------------------------------------
@functools.lru_cache(maxsize=None)
def roi_case(K, agnostic):
    """random logits of scale 3; rows 0..7 have the right class ahead of every other logit by 20 (saturated in fp32, finite in
    float64), rows 8..15 behind by 60"""
    g = torch.Generator().manual_seed(SEED + 10 * K + int(agnostic))
    src = BD.make_boxes(RR, g)
    gt = BD.make_gt(src, g, "smooth_l1")
    nreg = 1 if agnostic else K
    deltas = BD.make_deltas(RR * nreg, g).view(RR, nreg * 4)
    cls = torch.randint(0, K + 1, (RR,), generator=g)
    cls[:4], cls[4:8] = K, 0                                      # planted rows: background and foreground, both ends
    cls[8:12], cls[12:16] = K, K - 1
    cls[RLIVE:] = -1
    cols = K + 1 + 4 * nreg
    pred = torch.zeros(RR, (cols + 7) // 8 * 8)
    z = torch.randn(RR, K + 1, generator=g) * 3
    for r in range(2 * NPLANT):
        c = int(cls[r])
        others = torch.cat([z[r, :c], z[r, c + 1:]]).max()
        z[r, c] = others + (20.0 if r < NPLANT else -60.0)
    pred[:, :K + 1] = z
    pred[:, K + 1:cols] = deltas
    return {"K": K, "src": src, "gt": gt, "cls": cls.int(), "pred": pred, "cols": cols, "nreg": nreg, "agnostic": agnostic,
            "rois": torch.cat([torch.zeros(RR, 1), src], 1), "nv": torch.tensor([RLIVE], dtype=torch.int32)}


def run_roi_loss(native, c, cls_loss, grad=True, box_reg="auto"):
    if box_reg == "auto":
        box_reg = native.BoxRegOptions(ROI_W, cls_agnostic=True) if c["agnostic"] else None
    gs = torch.tensor(GS, device=DEV) if grad else None
    kw = {} if cls_loss is None else {"cls_loss": cls_loss}
    loss, d = native.frcnn_loss(c["pred"].to(DEV), c["K"], c["rois"].to(DEV), c["cls"].to(DEV), c["gt"].to(DEV), c["nv"].to(DEV),
                                grad_scale=gs, box_reg=box_reg, **kw)
    return loss.cpu(), (d.cpu() if d is not None else None)


@functools.lru_cache(maxsize=None)
def reference(K, agnostic, kind, gamma):
    c = roi_case(K, agnostic)
    z, cls = c["pred"][:, :K + 1], c["cls"].long()
    return (D.evaluate(z, cls, kind, gamma, GS32[0], torch.float64, RLIVE), D.evaluate(z, cls, kind, gamma, GS32[0], torch.float32, RLIVE))


def check_cls(native, label, K, agnostic, kind, gamma):
    c = roi_case(K, agnostic)
    loss, d = run_roi_loss(native, c, cls_opts(native, kind, gamma))
    (l64, s64, g64), (l32, _, g32) = reference(K, agnostic, kind, gamma)
    assert torch.isfinite(l64) and torch.isfinite(g64).all()          # the planted rows stay finite in float64
    assert torch.isfinite(loss).all() and torch.isfinite(d).all()
    gate_l, e32_l = D.gate(l64, l32, s64)
    dist_l = abs(loss[0].item() - l64.item())
    gmax = g64.abs().max().item()
    gate_g, e32_g = D.gate(g64, g32, gmax)
    dcls = d[:, :K + 1]
    dist_g = (dcls.double() - g64).abs().max().item()
    report(f"{label}: loss={l64.item():.9g} sum|terms|={s64.item():.6g} torch32={e32_l:.3e} device={dist_l:.3e} gate={gate_l:.3e} | "
           f"grad max={gmax:.6g} torch32={e32_g:.3e} device={dist_g:.3e} gate={gate_g:.3e}")
    assert dist_l <= gate_l, (label, "loss", dist_l, gate_l)
    assert dist_g <= gate_g, (label, "grad", dist_g, gate_g)
    assert gmax > 0 and (d[RLIVE:] == 0).all() and (d[:, c["cols"]:] == 0).all()      # padding rows and columns: exactly 0
    # the box half does not know the class mode: bit-identical to the "CrossEntropy" call on the same inputs
    l0, d0 = run_roi_loss(native, c, None)
    assert torch.equal(loss[1], l0[1]) and torch.equal(d[:, K + 1:], d0[:, K + 1:]) and d0[:, K + 1:].abs().sum() > 0
    return c, loss, d, (l0, d0)


KS = [1, 8, 80]
LAYOUTS = [False, True]


@pytest.mark.parametrize("agnostic", LAYOUTS, ids=["per-class", "class-agnostic"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("gamma", [0.0, 0.5, 1.0, 1.5, 2.0])
def test_focal_loss_and_gradient_match_the_definition(native, gamma, K, agnostic):
    c, loss, d, (l0, d0) = check_cls(native, f"focal gamma={gamma} K={K} {'agnostic' if agnostic else 'per-class'}", K, agnostic,
                                     "focal", gamma)
    (_, _, _), (_, _, g32) = reference(K, agnostic, "focal", gamma)
    if 0 < gamma < 1:
        assert not torch.isfinite(g32).all()                          # torch's fp32 gradient is inf * 0 on the saturated rows
    if gamma > 0:
        assert loss[0].item() < l0[0].item()                          # down-weighted rows
    # saturated rows ahead by 20: gradient ~0 but finite; rows behind by 60: the largest gradients of the matrix
    assert d[:NPLANT, :K + 1].abs().max().item() <= 1e-6 * d[:, :K + 1].abs().max().item() or gamma == 0.0
    assert d[NPLANT:2 * NPLANT, :K + 1].abs().max().item() >= 0.5 * GS[0] / RLIVE


@pytest.mark.parametrize("agnostic", LAYOUTS, ids=["per-class", "class-agnostic"])
@pytest.mark.parametrize("K", KS)
def test_sigmoid_ce_loss_and_gradient_match_the_definition(native, K, agnostic):
    c, loss, d, _ = check_cls(native, f"sigmoid K={K} {'agnostic' if agnostic else 'per-class'}", K, agnostic, "sigmoid", 0.0)
    assert (d[:, K] == 0).all()                                       # the background column gets no gradient
    # background rows have the all-zero target: their gradient is sigmoid(z) g / N > 0 in every foreground column
    bg = c["cls"] == K
    assert int(bg.sum()) >= 8
    want = torch.sigmoid(c["pred"][bg, :K].double()) * GS32[0] / RLIVE
    got = d[bg, :K].double()
    assert (got >= 0).all() and (got - want).abs().max().item() <= 4 * 2.0 ** -24 * want.max().item()


@pytest.mark.parametrize("kind", ["focal", "sigmoid"])
def test_a_nan_score_gives_a_nan_loss_as_cross_entropy_does(native, kind):
    """a diverged run must not log a finite loss_cls: one NaN score in one live row -> loss[0] is NaN in every mode"""
    c = dict(roi_case(8, False))
    c["pred"] = c["pred"].clone()
    c["pred"][20, 0] = float("nan")
    assert torch.isnan(run_roi_loss(native, c, None)[0][0])
    loss, d = run_roi_loss(native, c, cls_opts(native, kind))
    assert torch.isnan(loss[0]) and torch.isfinite(loss[1]) and torch.isnan(d[20, 0]) and torch.isfinite(d[21:]).all()


# ---- bit-identity of the existing entry points ---------------------------------------------------------------------------------
def _teacher_inputs(K, P, agnostic=False, seed=SEED):
    g = torch.Generator().manual_seed(seed)
    B = 2
    pc = torch.tensor([P, P - 33], dtype=torch.int32)
    span = torch.tensor([900.0, 400.0])
    props = []
    for _ in range(B):
        xy = torch.rand(P, 2, generator=g) * span
        props.append(torch.cat([xy, xy + torch.rand(P, 2, generator=g) * 250 + 2], 1))
    props = torch.stack(props)
    nreg = 1 if agnostic else K
    cols = K + 1 + 4 * nreg
    pred = torch.zeros(B * P, (cols + 7) // 8 * 8)
    pred[:, :K + 1] = torch.randn(B * P, K + 1, generator=g) * 3
    pred[:, K + 1:cols] = torch.randn(B * P, 4 * nreg, generator=g) * 0.7
    return B, pc, props, pred, cols, [(600, 1200), (590, 1100)]


def _candidates(native, name, pred, K, P, props, pc, sizes, thresh, *tail):
    B = props.shape[0]
    n = P * K
    cb = torch.empty(B, n, 4, device=DEV)
    cs, cc = torch.empty(B, n, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
    native.call(name, pred.to(DEV), pred.shape[1], B, P, K, props.to(DEV), pc.to(DEV),
                torch.tensor(sizes, dtype=torch.int32, device=DEV), thresh, cb, cs, cc, *tail)
    return cb.cpu(), cs.cpu(), cc.cpu()


def _bpc_inputs(K, agnostic=False, seed=77):
    g = torch.Generator().manual_seed(seed)
    B, per, G = 2, 60, 16
    sizes = [(200, 320), (220, 260)]
    R = B * per + 8
    nreg = 1 if agnostic else K
    cols = K + 1 + 4 * nreg
    pred = torch.zeros(R, (cols + 7) // 8 * 8)
    pred[:, :K + 1] = torch.randn(R, K + 1, generator=g) * 2.5
    pred[:, K + 1:cols] = torch.randn(R, 4 * nreg, generator=g) * 0.3
    rois = torch.full((R, 5), -1.0)
    roi_cls = torch.full((R,), K, dtype=torch.int32)
    gtb, gtc, gcnt = torch.zeros(B, G, 4), torch.zeros(B, G, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        xy = torch.rand(6, 2, generator=g) * torch.tensor([200.0, 120.0])
        gb = torch.cat([xy, xy + torch.rand(6, 2, generator=g) * 80 + 10], 1)
        gtb[b, :6], gtc[b, :6], gcnt[b] = gb, torch.randint(0, K, (6,), generator=g).int(), 6
        rows = slice(b * per, (b + 1) * per)
        xy = torch.rand(per, 2, generator=g) * torch.tensor([220.0, 130.0])
        pb = torch.cat([xy, xy + torch.rand(per, 2, generator=g) * 70 + 8], 1)
        pb[:30] = gb[torch.randint(0, 6, (30,), generator=g)] + torch.randn(30, 4, generator=g) * 3
        rois[rows, 0], rois[rows, 1:] = b, pb
        roi_cls[rows] = torch.randint(0, K + 1, (per,), generator=g).int()
    return pred, rois, roi_cls, sizes, gtb, gtc, gcnt, cols


def _bpc(native, pred, K, rois, roi_cls, sizes, gtb, gtc, gcnt, **kw):
    return native.bpc_loss(pred.to(DEV), K, rois.to(DEV), roi_cls.to(DEV), torch.tensor(sizes, dtype=torch.int32, device=DEV),
                           gtb.to(DEV), gtc.to(DEV), gcnt.to(DEV), **kw).cpu()


def test_existing_entry_points_equal_the_new_ones_in_mode_0(native, monkeypatch):
    """sfod_frcnn_loss, sfod_frcnn_loss_opt, sfod_frcnn_candidates(_opt), sfod_predict_probs and sfod_bpc_loss(_opt) against the
    ``*_cls`` entry points with cls_mode 0 (and a gamma that mode 0 must not read): torch.equal on every output."""
    names = []
    o_call = native.call

    def call(name, *a, **k):
        names.append(name)
        return o_call(name, *a, **k)
    monkeypatch.setattr(native, "call", call)
    ce = native.ClsLossOptions("CrossEntropy", 2.5, False)
    assert ce.mode == 0
    agn = native.BoxRegOptions((5.0, 5.0, 2.5, 2.5), "giou", 0.0, True)
    per = native.BoxRegOptions((5.0, 5.0, 2.5, 2.5), "smooth_l1", 0.5, False)
    for K in KS:
        for agnostic, box_reg in ((False, None), (False, per), (True, agn)):
            c = roi_case(K, agnostic)
            a, b = run_roi_loss(native, c, None, box_reg=box_reg), run_roi_loss(native, c, ce, box_reg=box_reg)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1].abs().sum() > 0
    K, P = 8, 300
    for agnostic, box_reg in ((False, None), (False, per), (True, agn)):
        B, pc, props, pred, _, sizes = _teacher_inputs(K, P, agnostic)
        szd = torch.tensor(sizes, dtype=torch.int32, device=DEV)
        x, y = [native.frcnn_inference(pred.to(DEV), K, props.to(DEV), pc.to(DEV), szd, SCORE_THRESH, 0.5, 100, 0.8, box_reg=box_reg, **kw)
                for kw in ({}, {"cls_loss": ce})]
        assert set(x) == set(y) and x["det_count"].sum() > 20
        for k in x:
            assert torch.equal(x[k], y[k]), k
        tail = (*(box_reg.weights if box_reg else ROI_W), int(agnostic))
        old = _candidates(native, "sfod_frcnn_candidates_opt", pred, K, P, props, pc, sizes, SCORE_THRESH, *tail)
        new = _candidates(native, "sfod_frcnn_candidates_cls", pred, K, P, props, pc, sizes, SCORE_THRESH, *tail, 0, 2.5)
        assert all(torch.equal(u, v) for u, v in zip(old, new)) and int(old[2].sum()) > 50
        if box_reg is None:
            plain = _candidates(native, "sfod_frcnn_candidates", pred, K, P, props, pc, sizes, SCORE_THRESH)
            assert all(torch.equal(u, v) for u, v in zip(plain, new))
        bi = _bpc_inputs(K, agnostic)
        u, v = _bpc(native, bi[0], K, *bi[1:7], box_reg=box_reg), _bpc(native, bi[0], K, *bi[1:7], box_reg=box_reg, cls_loss=ce)
        assert torch.equal(u, v) and u.item() > 0
    z = _teacher_inputs(K, P)[3][:, :K + 1].to(DEV)
    assert torch.equal(native.predict_probs(z), native.predict_probs(z, cls_loss=ce))
    ran = set(names)
    assert {"sfod_frcnn_loss", "sfod_frcnn_loss_opt", "sfod_frcnn_loss_cls", "sfod_frcnn_candidates", "sfod_frcnn_candidates_opt",
            "sfod_frcnn_candidates_cls", "sfod_predict_probs", "sfod_predict_probs_cls", "sfod_bpc_loss", "sfod_bpc_loss_opt",
            "sfod_bpc_loss_cls"} <= ran


# ---- probabilities, candidates and BPC under the sigmoid -----------------------------------------------------------------------
def test_predict_probs_and_candidates_with_sigmoid(native):
    """B = 2, P = 300 (300 and 267 live), K = 8.  No float64 probability lies within 1e-5 of the score threshold (asserted
    first; SEED is chosen for it), so the pass set and the counts are exact; the boxes are the softmax call's boxes."""
    K, P = 8, 300
    B, pc, props, pred, cols, sizes = _teacher_inputs(K, P)
    z = pred[:, :K + 1]
    p64 = D.probs(z.double(), True)
    margin = (p64 - SCORE_THRESH).abs().min().item()
    assert margin >= 1e-5 and (p64 - 0.5).abs().min().item() >= 1e-5, margin
    sg = native.ClsLossOptions("CrossEntropy", 1.5, True)
    got = native.predict_probs(z.to(DEV), cls_loss=sg).cpu()
    gate, e32 = D.gate(p64, D.probs(z, True), p64.max().item())
    dist = (got.double() - p64).abs().max().item()
    report(f"predict_probs sigmoid [{B * P}, {K + 1}]: margin to {SCORE_THRESH}={margin:.3e} torch32={e32:.3e} device={dist:.3e} gate={gate:.3e}")
    assert dist <= gate and got.shape == p64.shape
    # softmax mode through the same entry point, inside its own gate
    sm64 = D.probs(z.double(), False)
    got_sm = native.predict_probs(z.to(DEV), cls_loss=native.ClsLossOptions("FocalLoss", 1.5, False)).cpu()
    gate_sm, e32_sm = D.gate(sm64, D.probs(z, False), sm64.max().item())
    dist_sm = (got_sm.double() - sm64).abs().max().item()
    report(f"predict_probs softmax (focal) [{B * P}, {K + 1}]: torch32={e32_sm:.3e} device={dist_sm:.3e} gate={gate_sm:.3e}")
    assert dist_sm <= gate_sm and torch.equal(got_sm, native.predict_probs(z.to(DEV)).cpu())
    cb, cs, cc = _candidates(native, "sfod_frcnn_candidates_cls", pred, K, P, props, pc, sizes, SCORE_THRESH, *ROI_W, 0, 2, 1.5)
    allb, _, allc = _candidates(native, "sfod_frcnn_candidates_cls", pred, K, P, props, pc, sizes, -1.0, *ROI_W, 0, 0, 1.5)
    assert allc.tolist() == [int(pc[0]) * K, int(pc[1]) * K]          # every live entry: the softmax call's boxes
    live = (torch.arange(P)[None, :] < pc[:, None]).view(B, P, 1)
    want = (p64.view(B, P, K + 1)[:, :, :K] > SCORE_THRESH) & live
    passed = (cs > -1).view(B, P, K)
    assert torch.equal(passed, want) and cc.tolist() == want.view(B, -1).sum(1).tolist() and 50 < int(cc.sum()) < int(allc.sum())
    m = passed.view(B, P * K)
    assert torch.equal(cb[m], allb[m]) and (cb[~m] == 0).all() and (cs[~m] == -1).all()
    # the scores are predict_probs' probabilities, bit for bit (one device function)
    assert torch.equal(cs[m], got.view(B, P, K + 1)[:, :, :K].reshape(B, P * K)[m])
    # and the whole teacher post-processing runs on them
    out = native.frcnn_inference(pred.to(DEV), K, props.to(DEV), pc.to(DEV), torch.tensor(sizes, dtype=torch.int32, device=DEV),
                                 SCORE_THRESH, 0.5, 100, 0.8, cls_loss=sg)
    assert out["cand_count"].cpu().tolist() == cc.tolist() and int(out["det_count"].sum()) > 20
    n0 = int(out["det_count"][0])
    sc = out["det_scores"][0, :n0].cpu()
    assert (sc[:-1] >= sc[1:]).all() and sc.min() > SCORE_THRESH


def _bpc_reference(pred, K, rois, roi_cls, sizes, gtb, gtc, gcnt, dtype):
    """float64 / float32 restatement: the helper's sigmoid probabilities in the existing host definition of BPC (oracle/model.py:
    predict_boxes_for_gt_classes -> fast_rcnn_inference_single_image_new -> bpc_loss)"""
    ocfg = om.Cfg()
    assert ocfg.num_classes == K and tuple(ocfg.roi_bbox_weights) == ROI_W
    B = len(sizes)
    idx = [torch.nonzero(rois[:, 0] == b).flatten() for b in range(B)]
    inst, gts = [], []
    for b in range(B):
        r = idx[b]
        sc, dl = pred[r, :K + 1].to(dtype), pred[r, K + 1:5 * K + 1].to(dtype)
        nb = om.predict_boxes_for_gt_classes(dl, rois[r, 1:].to(dtype), roi_cls[r].long(), ocfg)
        bx = OB.apply_deltas(dl, nb, ROI_W)
        inst.append(om.frcnn_inference_new_single(bx, D.probs(sc, True), sizes[b]))
        n = int(gcnt[b])
        gts.append((gtb[b, :n].to(dtype), gtc[b, :n].long()))
    return om.bpc_loss(K, gts, inst), inst


def test_bpc_with_sigmoid(native):
    """s = the value (a loss of non-negative terms)"""
    K = 8
    bi = _bpc_inputs(K)
    pred, rois, roi_cls, sizes, gtb, gtc, gcnt, cols = bi
    ref64, inst = _bpc_reference(pred, K, rois, roi_cls, sizes, gtb, gtc, gcnt, torch.float64)
    ref32, _ = _bpc_reference(pred, K, rois, roi_cls, sizes, gtb, gtc, gcnt, torch.float32)
    p64 = D.probs(pred[rois[:, 0] >= 0, :K].double(), True)
    assert (p64 - 0.5).abs().min().item() >= 1e-5                     # no score on the confident / not-confident boundary
    sg = native.ClsLossOptions("CrossEntropy", 1.5, True)
    got = _bpc(native, pred, K, rois, roi_cls, sizes, gtb, gtc, gcnt, cls_loss=sg)
    soft = _bpc(native, pred, K, rois, roi_cls, sizes, gtb, gtc, gcnt)
    gate, e32 = D.gate(ref64, ref32, ref64.item())
    dist = abs(got.item() - ref64.item())
    report(f"bpc sigmoid K={K}: float64={ref64.item():.9g} torch32={e32:.3e} device={dist:.3e} gate={gate:.3e} (softmax value {soft.item():.9g})")
    assert ref64.dtype == torch.float64 and ref64.item() > 0.01 and dist <= gate
    assert abs(soft.item() - ref64.item()) > 1e-3                     # the mode is read


# ---- module level ----------------------------------------------------------------------------------------------------------------
Bm, Cm, Hf, Wf = 2, 512, 10, 12
Himg, Wimg = Hf * 16, Wf * 16
MODULE_OPTS = {"ce": [], "focal": ["MODEL.ROI_HEADS.LOSS", "FocalLoss"], "sigmoid": ["MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE", "True"]}


@functools.lru_cache(maxsize=None)
def module_run(kind):
    """SourceFreeAdaptiveTeacherStandardROIHeads of the hot yaml in fp32 mode on a 2 x 512 x 10 x 12 map with injected sampling
    keys -> relative distances of loss_cls (from the definition in float64 on the module's own prediction matrix) and of
    cls_score.weight.grad (from float64 autograd of definition + Linear on the module's own box features)"""
    sfod = importlib.import_module("simple-sfod_amd")
    cfg = sfod.config.setup_cfg(HOT_YAML, ["OUTPUT_DIR", "", "SFOD.COMPUTE_DTYPE", "fp32", "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", "64"]
                                + MODULE_OPTS[kind])
    torch.manual_seed(11)
    rh = sfod.modeling.roi_heads
    heads = rh.SourceFreeAdaptiveTeacherStandardROIHeads(cfg, {"vgg4": sfod.structures.ShapeSpec(channels=Cm, stride=16)}).to(DEV).train()
    bp = heads.box_predictor
    assert isinstance(bp, rh.SourceFreeFastRCNNOutputLayers) and (bp._cls_loss is None) == (kind == "ce")
    with torch.no_grad():
        bp.cls_score.weight.normal_(std=0.05)
        bp.bbox_pred.weight.normal_(std=0.05)
    K = heads.num_classes
    g = torch.Generator().manual_seed(12)
    feat = torch.randn(Bm, Cm, Hf, Wf, generator=g).to(DEV).requires_grad_(True)
    P = 40
    xy = torch.rand(Bm, P, 2, generator=g) * torch.tensor([Wimg * 0.7, Himg * 0.7])
    wh = torch.rand(Bm, P, 2, generator=g) * torch.tensor([Wimg * 0.3, Himg * 0.3]) + torch.tensor([0.4, 0.4])
    pboxes = torch.cat([xy, xy + wh], 2)
    S = sfod.structures
    targets = []
    for b in range(Bm):
        inst = S.Instances((Himg, Wimg))
        inst.gt_boxes = S.Boxes(pboxes[b, :5] + torch.randn(5, 4, generator=g) * 4)
        inst.gt_classes = torch.randint(0, K, (5,), generator=g)
        targets.append(inst)
    gt = sfod.modeling.batched.BatchedGT.from_instances(targets, DEV)
    props = sfod.modeling.batched.BatchedProposals(pboxes.to(DEV), torch.zeros(Bm, P, device=DEV),
                                                   torch.tensor([P, P - 7], dtype=torch.int32, device=DEV), [(Himg, Wimg)] * Bm)
    heads._forced_keys = torch.randint(0, 2 ** 31 - 1, (Bm, P + gt.boxes.shape[1]), generator=g).to(torch.int32).to(DEV)
    cap = {}
    o_fwd = heads._box_forward

    def box_forward(*a, **k):
        cap["st"] = o_fwd(*a, **k)
        return cap["st"]
    heads._box_forward = box_forward
    samples, losses, _, inst_props = heads(None, {"vgg4": feat}, props, gt)
    (losses["loss_cls"] * GS[0] + losses["loss_box_reg"] * GS[1]).backward()
    bpc = inst_props.bpc_loss(gt)
    torch.cuda.synchronize()
    assert torch.isfinite(bpc) and torch.isfinite(feat.grad).all()
    cls = samples["gt_cls"].cpu().long()
    n = int(samples["n_valid"].item())
    assert int((cls >= 0).sum()) == n and int(((cls >= 0) & (cls < K)).sum()) >= 8 and int((cls == K).sum()) >= 8
    pred = cap["st"]["pred"].float().cpu()
    l64, _ = D.cls_loss(pred[:, :K + 1].double(), cls, kind, cfg.SFOD.FOCAL_LOSS_GAMMA)
    d_loss = abs(losses["loss_cls"].item() - l64.item()) / abs(l64.item())
    h = heads.box_features(cap["st"]).float().cpu().double()
    W = bp.cls_score.weight.detach().double().cpu().requires_grad_(True)
    bias = bp.cls_score.bias.detach().double().cpu()
    l2, _ = D.cls_loss(h @ W.t() + bias, cls, kind, cfg.SFOD.FOCAL_LOSS_GAMMA)
    (gW,) = torch.autograd.grad(l2 * GS32[0], W)
    got = bp.cls_score.weight.grad.double().cpu()
    d_grad = ((got - gW).norm() / gW.norm()).item()
    assert gW.norm().item() > 0 and l64.item() > 1e-3
    if kind == "sigmoid":
        assert (got[K] == 0).all()                                     # the background score's weights get no class gradient
    return d_loss, d_grad, l64.item()


@pytest.mark.parametrize("kind", ["focal", "sigmoid"])
def test_module_loss_and_classifier_gradient_match_the_definition(native, kind):
    """Gate: 4 x the distance the same harness measures with "CrossEntropy" (the project's usual margin); all distances are
    relative.  The focal and sigmoid loss_cls is the fp32 rounding of a sum held in double (relative distance <= 2^-24)."""
    ce_loss, ce_grad, ce_val = module_run("ce")
    d_loss, d_grad, val = module_run(kind)
    gate_l, gate_g = 4 * ce_loss, 4 * ce_grad
    report(f"module {kind}: loss_cls float64={val:.9g} relative distance {d_loss:.3e} (CrossEntropy {ce_val:.9g}: {ce_loss:.3e}, gate "
           f"{gate_l:.3e}) | cls_score.weight.grad relative L2 distance {d_grad:.3e} (CrossEntropy {ce_grad:.3e}, gate {gate_g:.3e})")
    assert d_loss <= gate_l and d_grad <= gate_g


# ---- trainer ---------------------------------------------------------------------------------------------------------------------
def test_two_deterministic_focal_steps_are_reproducible(sfod, native):
    """TRAINER source_free_adaptive_teacher on the focal yaml, planted head, 256 x 384 frames, SFOD.DETERMINISTIC: two steps,
    twice -> finite losses with loss_cls_pseudo among them, bit-identical state and losses."""
    Bs, Hs, Ws = 2, 256, 384

    def run():
        cfg = sfod.config.setup_cfg(FOCAL_YAML, [
            "OUTPUT_DIR", "", "SOLVER.IMS_PER_BATCH_TARGET", str(Bs), "SFOD.SYNTHETIC.HEIGHT", str(Hs), "SFOD.SYNTHETIC.WIDTH", str(Ws),
            "SFOD.SYNTHETIC.NUM_IMAGES", "8", "INPUT.MIN_SIZE_TRAIN", f"({Hs},)", "SOLVER.WARMUP_ITERS", "0", "SOLVER.BASE_LR", "0.01",
            "SOLVER.CHECKPOINT_PERIOD", "0", "TEST.EVAL_PERIOD", "0", "TEST.VAL_LOSS", "False", "SFOD.EVAL_HOOK", "False",
            "WEAK_STRONG_AUGMENT", "False", "SFOD.DETERMINISTIC", "True", "SEMISUPNET.EMA_KEEP_RATE", "0.5"])
        torch.manual_seed(5)
        tr = sfod.engine.SourceFreeAdaptiveTeacherTrainer(cfg)
        bp = tr.model.roi_heads.box_predictor
        assert bp._cls_loss is not None and bp._cls_loss.mode == 1 and bp._cls_loss.gamma == 1.5
        assert tr.model_teacher.roi_heads.box_predictor._cls_loss.mode == 1
        with torch.no_grad():      # planted head: the teacher labels something from the first step on
            bp.cls_score.weight.mul_(30.0)
            tr._copy_main_model()
        g = torch.Generator().manual_seed(1)
        tr.model.proposal_generator._forced_keys = torch.randint(0, 2 ** 31 - 1, (Bs, (Hs // 32) * (Ws // 32) * 15), generator=g).to(torch.int32).to(DEV)
        tr.model.roi_heads._forced_keys = torch.randint(0, 2 ** 31 - 1, (Bs, 2100), generator=g).to(torch.int32).to(DEV)
        losses = []
        for it in range(2):
            tr.iter = it
            tr.run_step()
            tr.scheduler.step()
            rec = tr.storage.flush()
            losses.append({k: rec[k] for k in sorted(rec) if k.startswith("loss")})
        torch.cuda.synchronize()
        state = [tr.optimizer.flat.param.clone(), tr.optimizer.mom.clone(), tr.teacher_flat.param.clone()]
        del tr
        torch.cuda.empty_cache()
        return state, losses

    try:
        (a, la), (b, lb) = run(), run()
    finally:
        native.set_deterministic(False)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"state tensor {i} differs between two runs"
    assert la == lb and all(np.isfinite(v) for rec in la for v in rec.values()), la
    assert all("loss_cls_pseudo" in rec for rec in la), sorted(la[0])
    report(f"trainer focal: loss_cls_pseudo {[rec['loss_cls_pseudo'] for rec in la]}")
