"""The score-side kernels of csrc/detect.hip -- the ones that decide which boxes become proposals and which teacher detections
become pseudo ground truth -- at their threshold and non-finite edges.

Definitions: oracle/model.py (rpn_proposals, fast_rcnn_inference, threshold_bbox, bpc_loss) and oracle/box_ops.py on the CPU,
never the library.  Inputs: tests/helpers/score_edge_cases.py (fixed seeds, nothing excluded or drawn again);
tests/test_score_edge_cases_host.py holds every generator to the edge it is named for.  Exact decisions use dyadic geometry
(integer boxes, deltas that are zero or a translation by a multiple of 1/16 of the box), so decoded boxes are compared with
torch.equal; a threshold "exactly on a score" takes the score from the device's own sfod_predict_probs, which detect.hip
promises to be the value the candidates kernel thresholds.  The clamp and BPC cases are not dyadic: distance to the float64
definition <= 4 x max(torch-fp32's own distance to float64, 2^-24 x magnitude), both figures printed; with
SFOD_SCORE_EDGES_REPORT=<file> they are appended there (profiles/score_edges.txt is such a run).  OB.apply_deltas casts to
float32 (Detectron2's deltas.float()), so the float64 side of those gates is the helper's apply_deltas: OB's operations
without the cast, OB's bits in float32.

kernel                          definition                         cases
sfod_rpn_decode[_opt]           OB.apply_deltas + OB.clip_boxes,   divergence flag: NaN / +inf / -inf logit, NaN in each delta, +-inf dx alone
                                finite test of om.rpn_proposals    in a finite batch at anchor 0 of image 0 and the tail block's last lane of
                                                                   image 1 -> raised; dw = +-inf, NaN / inf padding -> not; sticky, stays 0;
                                                                   dw / ww at the fp32 clamp constant, one ulp below / above, 10, weights
                                                                   (1,1,1,1) and (2,2,1,1); boxes exactly on 0 and on (w, h), wholly outside,
                                                                   two image sizes
sfod_rpn_gather_topk[_opt]      OB.nonempty (strict)               width == min_size, min_size + 1, height == min_size, zero extent at
                                                                   min_size 0; k < NA and k == NA
decode -> sort -> gather ->     om.rpn_proposals(training=False)   NaN / +inf / -inf logits on finite boxes, non-finite deltas; k < NA, k == NA
nms -> gather_kept
RPN module                      FloatingPointError                 a NaN objectness bias -> check_finite() raises; a fresh module does not
sfod_predict_probs[_cls] +      probs > thr on predict_probs' own  thr == a probability of the batch and its predecessor; sigmoid(0) == 0.5 at
sfod_frcnn_candidates[_opt,_cls] bits                              thr 0.5; softmax / sigmoid x per-class / class-agnostic
native.frcnn_inference          om.fast_rcnn_inference +           pseudo_thr == a detection's score; 100 | 101 survivors at max_det 100; a NaN
(candidates, prepare_nms, nms,  om.threshold_bbox                  score, +inf dx, NaN dw row; NaN / +100 padding rows; logit gaps of +-60;
finalize)                                                          K = 32 (33 refused, outputs untouched); a dw beyond the clamp
sfod_bpc_loss                   om.bpc_loss                        score exactly 0.5 (K = 1); legacy IoU exactly 1/2 and one pixel row more;
                                                                   two ground truths at one IoU; no ground truth of the class; a background
                                                                   row; rows of image -1 and >= B; a wavefront with two images beside
                                                                   wavefronts with one
"""
import os

import pytest
import torch

from helpers import d2_published as D2
from helpers import score_edge_cases as sc
from oracle import box_ops as OB
from oracle import model as om

from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
HOT = os.path.join(ROOT, "configs", "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free.yaml")
COMBOS = [(False, False), (False, True), (True, False), (True, True)]
COMBO_IDS = ["softmax-per-class", "softmax-agnostic", "sigmoid-per-class", "sigmoid-agnostic"]


def report(line):
    print(line)
    path = os.environ.get("SFOD_SCORE_EDGES_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sizes(sizes):
    return torch.tensor(sizes, dtype=torch.int32, device=DEV)


def gated(label, dev, ref64, ref32):
    """the gate of tests/test_gpu_box_reg_options.py on one compared tensor; prints both figures"""
    mag = ref64.abs().max().item()
    gate, e32 = sc.gate(ref64, ref32, mag)
    dist = (dev.double() - ref64).abs().max().item()
    report(f"{label}: magnitude={mag:.6g} torch32={e32:.3e} device={dist:.3e} gate={gate:.3e}")
    assert dist <= gate, (label, dist, gate)


# ---- A. RPN decode and top-k gather -----------------------------------------------------------------------------------------
def decode(native, out, sizes=sc.RPN_SIZES, weights=None, flag=0):
    flags = torch.full((1,), flag, dtype=torch.int32, device=DEV)
    box_reg = None if weights is None else native.BoxRegOptions(weights)
    props, scores = native.rpn_decode(out.to(DEV), sc.CELL.to(DEV), sc.RB, sc.HF, sc.WF, sc.STRIDE, _sizes(sizes), flags,
                                      box_reg=box_reg)
    return props.cpu(), scores.cpu(), flags.item()


@pytest.mark.parametrize("place", sc.FLAG_PLACES, ids=["image0-anchor0", "image1-last-lane"])
@pytest.mark.parametrize("name,field,value,raises", sc.FLAG_PLANTS, ids=[p[0] for p in sc.FLAG_PLANTS])
def test_rpn_decode_raises_the_divergence_flag_exactly_when_detectron2_would(native, name, field, value, raises, place):
    out = sc.flag_case(name, place)
    props, scores, flag = decode(native, out)
    assert (flag != 0) == raises, (name, place, flag)
    logits, _ = sc.split(out)
    assert torch.equal(_bits(scores), _bits(logits))                  # the logits travel as they are, NaN payload included
    if not raises:
        assert torch.isfinite(props).all()


@pytest.mark.parametrize("weights", [None, sc.RPN_W2], ids=["sfod_rpn_decode", "sfod_rpn_decode_opt"])
def test_rpn_decode_flag_is_sticky_and_stays_zero_on_finite_input(native, weights):
    assert decode(native, sc.rpn_finite(), weights=weights)[2] == 0
    assert decode(native, sc.rpn_finite(), weights=weights, flag=4)[2] == 4            # a set flag is not cleared
    for place in sc.FLAG_PLACES:
        got = decode(native, sc.flag_case("nan-logit", place), weights=weights, flag=4)[2]
        assert got & 4 and got != 0
        assert decode(native, sc.flag_case("nan-dw", place), weights=weights)[2] != 0


@pytest.mark.parametrize("weights", [sc.RPN_W, sc.RPN_W2], ids=["weights-1-1-1-1", "weights-2-2-1-1"])
def test_rpn_decode_clamps_at_the_fp32_constant(native, weights):
    got = {}
    for name, value in sc.CLAMP_VALUES:
        out = sc.clamp_case(value, weights)
        props, _, flag = decode(native, out, sizes=sc.CLAMP_SIZES, weights=None if weights == sc.RPN_W else weights)
        assert flag == 0
        ref64 = sc.decode_definition(out, weights, sc.CLAMP_SIZES, torch.float64)
        ref32 = sc.decode_definition(out, weights, sc.CLAMP_SIZES, torch.float32)
        gated(f"rpn_decode clamp dw/ww={name} weights={weights} planted boxes", props[:, sc.CLAMP_ANCHORS],
              ref64[:, sc.CLAMP_ANCHORS], ref32[:, sc.CLAMP_ANCHORS])
        gated(f"rpn_decode clamp dw/ww={name} weights={weights} all boxes", props, ref64, ref32)
        got[name] = props
    assert torch.equal(got["above"], got["at"]) and torch.equal(got["ten"], got["at"])
    planted = got["at"][:, sc.CLAMP_ANCHORS]
    assert not torch.equal(got["below"][:, sc.CLAMP_ANCHORS], planted)                 # one ulp below is not clamped
    ext = torch.stack([planted[0, :, 2] - planted[0, :, 0], planted[1, :, 3] - planted[1, :, 1]])
    side = torch.stack([(sc.anchors()[sc.CLAMP_ANCHORS, 2] - sc.anchors()[sc.CLAMP_ANCHORS, 0]),
                        (sc.anchors()[sc.CLAMP_ANCHORS, 3] - sc.anchors()[sc.CLAMP_ANCHORS, 1])])
    assert ((ext / side - 62.5).abs() < 1e-3).all()                   # 1000 / 16


def test_rpn_decode_clips_exactly_onto_the_image_edges(native):
    """zero deltas: the decode is the identity, the proposals are the clipped anchors bit for bit -- boxes on 0 and on (w, h)
    stay, boxes wholly outside the smaller image collapse onto its edge"""
    out = sc.rpn_zero()
    for weights in (None, sc.RPN_W2):
        props, scores, flag = decode(native, out, weights=weights)
        ref = sc.decode_definition(out, sc.RPN_W, sc.RPN_SIZES, torch.float32)
        assert flag == 0 and torch.equal(props, ref) and (scores == 0).all()
        h, w = sc.RPN_SIZES[1]
        outside = (sc.anchors()[:, 0] >= w) | (sc.anchors()[:, 1] >= h)
        area = (props[1, :, 2] - props[1, :, 0]) * (props[1, :, 3] - props[1, :, 1])
        assert int(outside.sum()) > 20 and (area[outside] == 0).all() and (area[~outside] > 0).any()


@pytest.mark.parametrize("k", sc.PIPE_K)
@pytest.mark.parametrize("min_size", [sc.MIN_SIZE, 0.0])
def test_rpn_gather_topk_validity_is_strict_at_min_size(native, min_size, k):
    props, scores, planted = sc.min_size_case()
    ss, si = torch.sort(scores, dim=1, descending=True, stable=True)
    cb, cs, cv = native.rpn_gather_topk(props.to(DEV), ss.to(DEV), si.int().to(DEV), k, min_size=min_size)
    for b in range(sc.RB):
        order = si[b, :k]
        assert torch.equal(cb[b].cpu(), props[b][order]) and torch.equal(cs[b].cpu(), ss[b, :k])
        want = OB.nonempty(props[b][order], min_size)
        assert torch.equal(cv[b].cpu().bool(), want)
        pos = {int(i): j for j, i in enumerate(order.tolist())}
        for name, (i, _) in planted.items():
            if i in pos:
                valid = bool(cv[b, pos[i]])
                assert valid == (name in ("width-plus-1", "both-plus-1") or (min_size == 0.0 and name in ("width-eq", "height-eq"))), name


def proposals(native, out, k, post=sc.PIPE_POST, sizes=sc.PIPE_SIZES):
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    props, scores = native.rpn_decode(out.to(DEV), sc.CELL.to(DEV), sc.RB, sc.HF, sc.WF, sc.STRIDE, _sizes(sizes), flags)
    ss, si = native.segmented_sort_desc(scores)
    cb, cs, cv = native.rpn_gather_topk(props, ss, si, k)
    keep_idx, keep_cnt = native.nms(cb, 0.7, post, valid=cv)
    pb, ps = native.gather_kept(cb, cs, keep_idx, keep_cnt)
    return pb.cpu(), ps.cpu(), keep_cnt.cpu(), flags.item(), (cs.cpu(), cv.cpu())


@pytest.mark.parametrize("k", sc.PIPE_K, ids=["k-lt-NA", "k-eq-NA"])
def test_eval_mode_proposals_drop_non_finite_candidates_like_the_oracle(native, k):
    """find_top_rpn_proposals in eval mode drops every top-k candidate whose box or logit is not finite; NaN and +inf rank
    first, -inf is inside the top k when k == NA.  Counts and scores exact; no kept score is non-finite."""
    out = sc.pipeline_case()
    ref = sc.pipeline_definition(out, k)
    pb, ps, cnt, flag, (cs, cv) = proposals(native, out, k)
    assert flag != 0                                                   # and the divergence is still reported
    for b in range(sc.RB):
        n = cnt[b].item()
        assert torch.isfinite(ps[b, :n]).all() and torch.isfinite(pb[b, :n]).all()
        assert n == len(ref[b][0]) and n >= 10, (b, n, len(ref[b][0]))
        assert torch.equal(ps[b, :n], ref[b][1])
        torch.testing.assert_close(pb[b, :n], ref[b][0], rtol=1e-5, atol=1e-3)
        assert torch.equal(pb[b, :n], ref[b][0])                       # (dyadic: the same bits)
        assert (pb[b, n:] == 0).all() and (ps[b, n:] == 0).all()
    assert not (cv.bool() & ~torch.isfinite(cs)).any()                 # a candidate with a non-finite logit is not valid
    # the same batch without the plants: same kernels, flag down
    clean = sc.rpn_dyadic()
    ref = sc.pipeline_definition(clean, k)
    pb, ps, cnt, flag, _ = proposals(native, clean, k)
    assert flag == 0
    for b in range(sc.RB):
        n = cnt[b].item()
        assert n == len(ref[b][0]) and torch.equal(ps[b, :n], ref[b][1]) and torch.equal(pb[b, :n], ref[b][0])


def test_rpn_module_reports_a_nan_objectness_bias(sfod, native):
    c = D2.rpn_case()
    S = sfod.structures
    cfg = sfod.config.setup_cfg(HOT, ["SFOD.COMPUTE_DTYPE", "fp32", "MODEL.DEVICE", DEV, "OUTPUT_DIR", "", "MODEL.RPN.IN_FEATURES",
                                      "['res4']", "MODEL.ANCHOR_GENERATOR.SIZES", "[[32, 64, 128, 256, 512]]",
                                      "MODEL.ANCHOR_GENERATOR.ASPECT_RATIOS", "[[0.5, 1.0, 2.0]]"])
    images = S.ImageList(torch.zeros(2, 3, 20, 30), c["image_sizes"])
    gt = []
    for b in c["gt_boxes"]:
        inst = S.Instances((15, 15))
        inst.gt_boxes, inst.gt_classes = S.Boxes(b), torch.zeros(len(b), dtype=torch.long)
        gt.append(inst)
    for poisoned in (False, True):
        rpn = sfod.modeling.rpn.RPN(cfg, {"res4": S.ShapeSpec(channels=1024, stride=16)})
        rpn.rpn_head.load_state_dict(c["head"])
        rpn = rpn.to(DEV).train()
        if poisoned:
            with torch.no_grad():
                rpn.rpn_head.objectness_logits.bias[3] = float("nan")
        with torch.no_grad():
            rpn(images, {"res4": c["feat"].to(DEV)}, gt)
        if poisoned:
            with pytest.raises(FloatingPointError):
                rpn.check_finite()
        else:
            rpn.check_finite()


# ---- B. teacher post-processing ---------------------------------------------------------------------------------------------
def cls_opts(native, sigmoid):
    return native.ClsLossOptions("CrossEntropy", 1.5, True) if sigmoid else None


def box_opts(native, case):
    return native.BoxRegOptions(sc.ROI_W, cls_agnostic=True) if case["agnostic"] else None


def inference(native, case, sigmoid, score_thresh=sc.SCORE_THRESH, pseudo_thr=sc.PSEUDO_THR, max_det=sc.MAX_DET):
    out = native.frcnn_inference(case["pred"].to(DEV), case["K"], case["props"].to(DEV), case["pc"].to(DEV), _sizes(case["sizes"]),
                                 score_thresh, sc.NMS_THRESH, max_det, pseudo_thr, box_reg=box_opts(native, case),
                                 cls_loss=cls_opts(native, sigmoid))
    return {k: v.cpu() for k, v in out.items()}


def candidates(native, case, sigmoid, thr):
    B, P, _ = case["props"].shape
    K = case["K"]
    cb = torch.full((B, P * K, 4), -7.0, device=DEV)
    cs, cc = torch.full((B, P * K), -7.0, device=DEV), torch.full((B,), -7, dtype=torch.int32, device=DEV)
    native.call("sfod_frcnn_candidates_cls", case["pred"].to(DEV), case["pred"].shape[1], B, P, K, case["props"].to(DEV),
                case["pc"].to(DEV), _sizes(case["sizes"]), thr, cb, cs, cc, *sc.ROI_W, int(case["agnostic"]), 2 if sigmoid else 0, 0.0)
    return cb.cpu().view(B, P, K, 4), cs.cpu().view(B, P, K), cc.cpu()


def device_probs(native, case, sigmoid):
    K = case["K"]
    pred = case["pred"].to(DEV)
    p = native.predict_probs(pred[:, :K + 1], cls_loss=cls_opts(native, sigmoid)).cpu()
    return p.view(case["props"].shape[0], -1, K + 1)


def live_mask(case):
    B, P, _ = case["props"].shape
    return (torch.arange(P)[None, :] < case["pc"][:, None]).view(B, P, 1)


def check_inference(out, ref, case, exact_boxes=True, pseudo_thr=sc.PSEUDO_THR):
    """counts, classes and (dyadic) boxes exact; scores as tests/test_gpu_ops.py compares two fp32 softmaxes"""
    assert out["cand_count"].tolist() == [r["cand"] for r in ref]
    for b, r in enumerate(ref):
        n = out["det_count"][b].item()
        assert n == len(r["scores"]), (b, n, len(r["scores"]))
        assert out["det_classes"][b, :n].long().tolist() == r["classes"].tolist()
        torch.testing.assert_close(out["det_scores"][b, :n], r["scores"], rtol=1e-5, atol=1e-7)
        if exact_boxes:
            assert torch.equal(out["det_boxes"][b, :n], r["boxes"])
        assert (out["det_boxes"][b, n:] == 0).all() and (out["det_scores"][b, n:] == 0).all()
        pl = om.threshold_bbox(r, pseudo_thr)
        m = out["gt_count"][b].item()
        assert m == len(pl["gt_classes"]) and out["gt_classes"][b, :m].long().tolist() == pl["gt_classes"].tolist()
        assert torch.equal(out["gt_boxes"][b, :m], out["det_boxes"][b, :m])
        assert (out["gt_boxes"][b, m:] == 0).all() and (out["gt_classes"][b, m:] == 0).all()


@pytest.mark.parametrize("sigmoid,agnostic", COMBOS, ids=COMBO_IDS)
def test_score_threshold_is_strict_on_the_devices_own_probabilities(native, sigmoid, agnostic):
    case = sc.teacher_random_case(8, agnostic)
    K = case["K"]
    if sigmoid:                                                        # 1 / (1 + expf(-0)) is exactly 0.5
        pred = case["pred"].clone()
        pred[3, 2] = 0.0
        case = sc.with_pred(case, pred)
    probs = device_probs(native, case, sigmoid)
    fg, live = probs[:, :, :K], live_mask(case)
    vals = fg[live.expand_as(fg)]
    vals = torch.sort(vals[vals > sc.SCORE_THRESH])[0]
    stars = [vals[len(vals) // 2].item(), vals[0].item(), vals[-1].item()]
    if sigmoid:
        assert probs[0, 3, 2].item() == 0.5
        stars.append(0.5)
    for p_star in stars:
        hit = (fg == p_star) & live
        assert hit.any()
        below = torch.nextafter(torch.tensor(p_star), torch.tensor(-float("inf"))).item()
        for thr, passes in ((p_star, False), (below, True)):
            cb, cs, cc = candidates(native, case, sigmoid, thr)
            passed = cs != -1.0
            want = (fg > thr) & live
            assert torch.equal(passed, want), (p_star, thr)
            assert bool(passed[hit].all()) == passes and bool(passed[hit].any()) == passes
            assert cc.tolist() == want.view(want.shape[0], -1).sum(1).tolist()
            assert torch.equal(_bits(cs[passed]), _bits(fg[passed]))   # one device function: the same bits
            assert (cb[~passed] == 0).all()


@pytest.mark.parametrize("sigmoid,agnostic", COMBOS, ids=COMBO_IDS)
def test_pseudo_label_threshold_is_strict_on_a_detections_own_score(native, sigmoid, agnostic):
    case = sc.teacher_case(8, agnostic)
    first = inference(native, case, sigmoid)
    n0 = first["det_count"][0].item()
    assert n0 >= 10 and first["gt_count"].sum() > 0
    for pos in (n0 // 2, 0, n0 - 1):
        s_star = first["det_scores"][0, pos].item()
        out = inference(native, case, sigmoid, pseudo_thr=s_star)
        for key in ("det_boxes", "det_scores", "det_classes", "det_count", "cand_count"):
            assert torch.equal(out[key], first[key]), key
        for b in range(sc.TB):
            n = out["det_count"][b].item()
            m = int((out["det_scores"][b, :n] > s_star).sum())
            assert out["gt_count"][b].item() == m
            assert torch.equal(out["gt_boxes"][b, :m], out["det_boxes"][b, :m])
            assert torch.equal(out["gt_classes"][b, :m], out["det_classes"][b, :m])
            assert (out["gt_boxes"][b, m:] == 0).all() and (out["gt_classes"][b, m:] == 0).all()
        assert out["gt_count"][0].item() <= pos                        # the detection on the threshold is not a label


@pytest.mark.parametrize("sigmoid,agnostic", COMBOS, ids=COMBO_IDS)
def test_detections_are_cut_at_max_det_and_the_lowest_score_goes(native, sigmoid, agnostic):
    case = sc.max_det_case(8, agnostic, sigmoid)
    out = inference(native, case, sigmoid)
    assert out["cand_count"].tolist() == [100, 101] and out["det_count"].tolist() == [100, 100]
    check_inference(out, sc.teacher_definition(case, sigmoid), case)
    lowest = case["props"][1, 0]                                       # row 0 has image 1's lowest score
    assert not (out["det_boxes"][1] == lowest).all(1).any() and (out["det_boxes"][0] == lowest).all(1).any()
    sc1 = out["det_scores"][1]
    assert (sc1[:-1] > sc1[1:]).all()


@pytest.mark.parametrize("sigmoid,agnostic", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("name", [p[0] for p in sc.ROW_PLANTS])
def test_a_non_finite_row_disappears_for_every_class(native, name, sigmoid, agnostic):
    base = sc.teacher_case(8, agnostic)
    case, b, j = sc.row_plant_case(base, name)
    cb0, cs0, cc0 = candidates(native, base, sigmoid, sc.SCORE_THRESH)
    cb1, cs1, cc1 = candidates(native, case, sigmoid, sc.SCORE_THRESH)
    lost = int((cs0[b, j] != -1).sum())
    assert lost > 0 and (cs1[b, j] == -1).all() and (cb1[b, j] == 0).all()
    cs0[b, j], cb0[b, j] = -1.0, 0.0
    assert torch.equal(cs0, cs1) and torch.equal(cb0, cb1)             # the neighbours are untouched
    want = cc0.clone()
    want[b] -= lost
    assert cc1.tolist() == want.tolist()
    check_inference(inference(native, case, sigmoid), sc.teacher_definition(case, sigmoid), case)


@pytest.mark.parametrize("sigmoid,agnostic", COMBOS, ids=COMBO_IDS)
def test_rows_beyond_prop_count_are_never_read_as_candidates(native, sigmoid, agnostic):
    base, case = sc.padding_case(sc.teacher_case(8, agnostic))
    a, b = inference(native, base, sigmoid), inference(native, case, sigmoid)
    for key in a:
        assert torch.equal(a[key], b[key]), key
    _, cs, cc = candidates(native, case, sigmoid, sc.SCORE_THRESH)
    n0 = int(case["pc"][0])
    assert (cs[0, n0:] == -1).all() and cc.tolist() == a["cand_count"].tolist()
    check_inference(b, sc.teacher_definition(case, sigmoid), case)
    assert a["det_count"][1].item() >= 10


@pytest.mark.parametrize("sigmoid,agnostic", COMBOS, ids=COMBO_IDS)
def test_saturated_rows_decide_like_the_oracle(native, sigmoid, agnostic):
    case, up, down = sc.saturated_case(sc.teacher_case(8, agnostic), sigmoid)
    probs = device_probs(native, case, sigmoid).view(-1, case["K"] + 1)
    for r, c in up:
        assert probs[r, c].item() == 1.0 and (torch.cat([probs[r, :c], probs[r, c + 1:case["K"]]]) < sc.SCORE_THRESH).all()
    for r, c in down:
        assert probs[r, c].item() < sc.SCORE_THRESH
    out = inference(native, case, sigmoid)
    check_inference(out, sc.teacher_definition(case, sigmoid), case)
    assert (out["det_scores"] == 1.0).sum() >= 6 and out["gt_count"].min() >= 3


@pytest.mark.parametrize("sigmoid,agnostic", COMBOS, ids=COMBO_IDS)
def test_thirty_two_classes_fill_the_per_thread_arrays(native, sigmoid, agnostic):
    case = sc.teacher_case(32, agnostic)
    out = inference(native, case, sigmoid)
    check_inference(out, sc.teacher_definition(case, sigmoid), case)
    assert out["det_count"].min() >= 10 and int(out["det_classes"].max()) > 8
    probs = device_probs(native, case, sigmoid)
    ref = sc.probs_of(sc.scores_of(case), sigmoid).view(probs.shape)
    torch.testing.assert_close(probs, ref, rtol=1e-5, atol=1e-7)


def test_thirty_three_classes_are_refused_before_anything_is_written(native):
    K, B, P, G = 33, 2, 8, 4
    ld = 5 * K + 1 + 3
    pred = torch.zeros(B * P, ld, device=DEV)
    props = torch.tensor([0.0, 0, 16, 16], device=DEV).repeat(B, P, 1)
    pc = torch.full((B,), P, dtype=torch.int32, device=DEV)
    szd = _sizes([(64, 64)] * B)
    cb, cs = torch.full((B, P * K, 4), -7.0, device=DEV), torch.full((B, P * K), -7.0, device=DEV)
    cc = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    for name, tail in (("sfod_frcnn_candidates", ()), ("sfod_frcnn_candidates_opt", (*sc.ROI_W, 0)),
                       ("sfod_frcnn_candidates_cls", (*sc.ROI_W, 1, 2, 0.0))):
        with pytest.raises(native.NativeLibraryError):
            native.call(name, pred, ld, B, P, K, props, pc, szd, 0.05, cb, cs, cc, *tail)
    probs = torch.full((B * P, K + 1), -7.0, device=DEV)
    for name, tail in (("sfod_predict_probs", ()), ("sfod_predict_probs_cls", ())):
        with pytest.raises(native.NativeLibraryError):
            if name.endswith("_cls"):
                native.call(name, pred, ld, B * P, K, 2, 0.0, probs)
            else:
                native.call(name, pred, ld, B * P, K, probs)
    rois = torch.cat([torch.zeros(B * P, 1, device=DEV), props.view(-1, 4)], 1)
    roi_cls = torch.zeros(B * P, dtype=torch.int32, device=DEV)
    gtb, gtc = torch.zeros(B, G, 4, device=DEV), torch.zeros(B, G, dtype=torch.int32, device=DEV)
    gcnt = torch.zeros(B, dtype=torch.int32, device=DEV)
    loss, ws = torch.full((1,), -7.0, device=DEV), torch.full((4 * B,), -7.0, dtype=torch.float64, device=DEV)
    for name, tail in (("sfod_bpc_loss", ()), ("sfod_bpc_loss_opt", (*sc.ROI_W, 0)), ("sfod_bpc_loss_cls", (*sc.ROI_W, 1, 2, 0.0))):
        with pytest.raises(native.NativeLibraryError):
            native.call(name, pred, ld, B * P, K, rois, roi_cls, B, szd, gtb, gtc, gcnt, G, 0.5, loss, ws, *tail)
    torch.cuda.synchronize()
    for t in (cb, cs, probs, loss, ws):
        assert (t == -7.0).all()
    assert (cc == -7).all()
    # 32 is accepted by all three (the arrays' last slots)
    native.call("sfod_frcnn_candidates", pred[:, :168].contiguous(), 168, B, P, 32, props, pc, szd, 0.05, cb, cs, cc)
    native.call("sfod_predict_probs", pred[:, :168].contiguous(), 168, B * P, 32, probs)
    native.call("sfod_bpc_loss", pred[:, :168].contiguous(), 168, B * P, 32, rois, roi_cls, B, szd, gtb, gtc, gcnt, G, 0.5, loss, ws)
    torch.cuda.synchronize()
    dense = probs.view(-1)[: B * P * 33]                                # [R, K + 1] with K = 32, written densely
    assert cc.tolist() == [0, 0] and (dense == dense[0]).all() and abs(dense[0].item() - 1 / 33) < 1e-7
    assert torch.isfinite(loss).all()


@pytest.mark.parametrize("agnostic", [False, True], ids=["per-class", "class-agnostic"])
def test_teacher_decode_clamps_a_scale_delta_beyond_the_clamp(native, agnostic):
    case, rows = sc.decode_clamp_case(8, agnostic)
    out = inference(native, case, False)
    ref64 = sc.teacher_definition(case, False, dtype=torch.float64)
    ref32 = sc.teacher_definition(case, False, dtype=torch.float32)
    check_inference(out, ref32, case, exact_boxes=False)
    for b, j in rows:
        n = out["det_count"][b].item()
        hit64 = torch.nonzero((ref64[b]["roi_idx"] == j) & (ref64[b]["classes"] == 1)).flatten()
        hit32 = torch.nonzero((ref32[b]["roi_idx"] == j) & (ref32[b]["classes"] == 1)).flatten()
        assert len(hit64) == 1 and hit64.tolist() == hit32.tolist() and hit64[0] < n
        i = int(hit64[0])
        assert out["det_scores"][b, i].item() == 1.0 and out["det_classes"][b, i].item() == 1
        gated(f"frcnn_inference clamp {'dw' if b == 0 else 'dh'} {'class-agnostic' if agnostic else 'per-class'} image {b} row {j}",
              out["det_boxes"][b, i], ref64[b]["boxes"][i], ref32[b]["boxes"][i])
        others = [k for k in range(n) if k != i and not (agnostic and int(ref32[b]["roi_idx"][k]) == j)]
        assert torch.equal(out["det_boxes"][b, others], ref32[b]["boxes"][others])       # the rest of the batch is dyadic


# ---- C. BPC sums -----------------------------------------------------------------------------------------------------------
def bpc(native, case):
    return native.bpc_loss(case["pred"].to(DEV), case["K"], case["rois"].to(DEV), case["roi_cls"].to(DEV), _sizes(case["sizes"]),
                           case["gtb"].to(DEV), case["gtc"].to(DEV), case["gcnt"].to(DEV), iou_thresh=case["iou_thr"]).cpu()


def check_bpc(native, label, case):
    ref64 = sc.bpc_definition(case, torch.float64)[0]
    ref32 = sc.bpc_definition(case, torch.float32)[0]
    got = bpc(native, case)
    assert ref64.item() > 0
    gated(f"bpc_loss {label} float64={ref64.item():.9g}", got.view(1), ref64.view(1), ref32.view(1))
    return got


@pytest.mark.parametrize("name", sc.BPC_NAMES)
def test_bpc_decisions_at_their_edges(native, name):
    check_bpc(native, name, sc.bpc_case(name))


def test_bpc_iou_exactly_on_the_threshold_is_a_false_positive(native):
    on, above = check_bpc(native, "iou-half", sc.bpc_case("iou-half")), check_bpc(native, "iou-above-half", sc.bpc_case("iou-above-half"))
    assert abs(on.item() - above.item()) > 1e-3


def test_bpc_wavefronts_with_one_image_and_with_two_in_one_launch(native):
    case = sc.bpc_mixed_case()
    waves = sc.wave_images(case)
    assert {0, 1} in waves and {0} in waves and {1} in waves
    check_bpc(native, "mixed wavefronts K=3 R=100", case)
