"""tests/helpers/score_edge_cases.py held to the edges its cases are named for, on the CPU: every planted edge is asserted in
float64 or by bit pattern, the exact-decision cases are dyadic, and the oracle ALONE produces what tests/test_gpu_score_edges.py
assumes of it (non-empty outputs, exactly the planted rows dropped, a true and a false positive in every BPC case)."""
import math
import os

import numpy as np
import pytest
import torch

from helpers import score_edge_cases as sc
from oracle import box_ops as OB
from oracle import model as om


def _bits(t):
    return t.contiguous().view(torch.int32)


def _dyadic(t, denom=16):
    return bool((t.double() * denom == (t.double() * denom).round()).all())


# ---- A. RPN ----------------------------------------------------------------------------------------------------------------
def test_rpn_grid_is_small_ragged_and_padded():
    assert sc.NA == 270 and sc.NA % 256 != 0 and sc.NA > 256 and sc.LD > 5 * sc.A
    assert sc.FLAG_PLACES == [(0, 0), (1, sc.NA - 1)]
    assert _dyadic(sc.anchors(), 1) and sc.rpn_finite().shape == (sc.RB * sc.HF * sc.WF, sc.LD)
    assert (sc.rpn_finite()[:, 5 * sc.A:] == 0).all() and torch.isfinite(sc.rpn_finite()).all()


@pytest.mark.parametrize("place", sc.FLAG_PLACES)
@pytest.mark.parametrize("name,field,value,raises", sc.FLAG_PLANTS)
def test_flag_plants_are_alone_and_the_oracle_agrees_on_which_diverge(name, field, value, raises, place):
    base, out = sc.rpn_finite(), sc.flag_case(name, place)
    diff = torch.nonzero(_bits(base) != _bits(out))
    assert len(diff) == 1                                             # one element, nothing else touched
    row, col = diff[0].tolist()
    assert row == place[0] * sc.HF * sc.WF + place[1] // sc.A
    got = out[row, col].item()
    assert (math.isnan(got) and math.isnan(value)) or got == value
    assert (col >= 5 * sc.A) == (field == "pad")
    assert not sc.oracle_raises(base)
    assert sc.oracle_raises(out) == raises
    if name in ("+inf-dw", "-inf-dw"):
        _, deltas = sc.split(out)
        box = OB.apply_deltas(deltas[place[0]], sc.anchors(), sc.RPN_W)[place[1]]
        assert torch.isfinite(box).all()
        assert (box[2] - box[0]).item() == (0.0 if value < 0 else pytest.approx(62.5 * (sc.anchors()[place[1], 2] - sc.anchors()[place[1], 0]).item()))


def test_clamp_values_are_the_fp32_constant_and_its_neighbours():
    c = np.float32(sc.CLAMP64)
    assert sc.CLAMP32 == float(c) and abs(sc.CLAMP32 - math.log(1000.0 / 16)) <= 2.0 ** -24 * 4.2
    b, a = np.float32(sc.CLAMP32_BELOW), np.float32(sc.CLAMP32_ABOVE)
    assert b < c < a and int(c.view(np.int32)) - int(b.view(np.int32)) == 1 and int(a.view(np.int32)) - int(c.view(np.int32)) == 1
    assert [v for _, v in sc.CLAMP_VALUES] == [sc.CLAMP32, sc.CLAMP32_BELOW, sc.CLAMP32_ABOVE, 10.0]
    for w in (sc.RPN_W, sc.RPN_W2):
        for name, v in sc.CLAMP_VALUES:
            out = sc.clamp_case(v, w)
            _, d = sc.split(out)
            for i in sc.CLAMP_ANCHORS:                                # the quotient the kernel forms is the value, in fp32
                assert (d[0, i, 2] / np.float32(w[2])).item() == v and (d[1, i, 3] / np.float32(w[3])).item() == v
                assert (d[0, i, 0] / np.float32(w[0])).item() == 40.0
            ref = sc.decode_definition(out, w, sc.CLAMP_SIZES, torch.float64)
            raw = torch.stack([sc.apply_deltas(d[b].double(), sc.anchors().double(), w) for b in range(sc.RB)])
            assert ref.dtype == raw.dtype == torch.float64
            r32 = sc.decode_definition(out, w, sc.CLAMP_SIZES, torch.float32)
            assert torch.equal(r32, torch.stack([OB.clip_boxes(OB.apply_deltas(d[b], sc.anchors(), w), sc.CLAMP_SIZES[b]) for b in range(sc.RB)]))
            assert 0 < (r32.double() - ref)[:, sc.CLAMP_ANCHORS].abs().max().item() < 1e-3      # a float64 definition: fp32 is not on it
            assert torch.equal(ref[:, sc.CLAMP_ANCHORS], raw[:, sc.CLAMP_ANCHORS])      # the planted boxes are not clipped
            ext = ref[0, sc.CLAMP_ANCHORS, 2] - ref[0, sc.CLAMP_ANCHORS, 0]
            wid = (sc.anchors()[sc.CLAMP_ANCHORS, 2] - sc.anchors()[sc.CLAMP_ANCHORS, 0]).double()
            want = 62.5 if name != "below" else math.exp(sc.CLAMP32_BELOW)
            assert ((ext / wid - want).abs() <= 1e-6 * want).all()


def test_zero_deltas_decode_to_the_anchors_and_the_clip_edges_are_there():
    out = sc.rpn_zero()
    for dtype in (torch.float32, torch.float64):
        _, d = sc.split(out)
        assert torch.equal(sc.apply_deltas(d[0].to(dtype), sc.anchors().to(dtype), sc.RPN_W), sc.anchors().to(dtype))
    ref = sc.decode_definition(out, sc.RPN_W, sc.RPN_SIZES, torch.float32)
    an = sc.anchors()
    for b, (h, w) in enumerate(sc.RPN_SIZES):
        assert (an[:, 0] == 0).any() and (an[:, 1] == 0).any()                          # exactly on 0
        outside = (an[:, 0] >= w) | (an[:, 1] >= h)
        ext = (ref[b, :, 2] - ref[b, :, 0]) * (ref[b, :, 3] - ref[b, :, 1])
        assert (ext[outside] == 0).all()
        assert int(outside.sum()) == (0 if b == 0 else int(outside.sum())) and (b == 0 or int(outside.sum()) > 20)
    assert (an[:, 2] == sc.RPN_SIZES[0][1]).any() and (an[:, 3] == sc.RPN_SIZES[0][0]).any()          # exactly on (w, h)
    assert (an[:, 0] < 0).any() and (an[:, 2] > sc.RPN_SIZES[1][1]).any()               # and clipped on both sides
    assert sc.RPN_SIZES[0] != sc.RPN_SIZES[1]


def test_min_size_plants_sit_exactly_on_the_threshold():
    props, scores, planted = sc.min_size_case()
    assert _dyadic(props, 1) and len(torch.unique(scores)) == scores.numel()
    w, h = props[..., 2] - props[..., 0], props[..., 3] - props[..., 1]
    for b in range(sc.RB):
        valid = OB.nonempty(props[b], sc.MIN_SIZE)
        want = {"width-eq": False, "width-plus-1": True, "height-eq": False, "both-plus-1": True, "zero-extent": False,
                "zero-width": False}
        for name, (i, (pw, ph)) in planted.items():
            assert (w[b, i].item(), h[b, i].item()) == (pw, ph)
            assert bool(valid[i]) == want[name], name
        assert w[b, 0].item() == sc.MIN_SIZE and h[b, 2].item() == sc.MIN_SIZE and w[b, 1].item() == sc.MIN_SIZE + 1
        z = OB.nonempty(props[b], 0.0)
        assert not z[4] and not z[sc.NA - 1] and z[0] and 100 < int(valid.sum()) < int(z.sum())
        top = torch.sort(scores[b], descending=True, stable=True)[1][: sc.PIPE_K[0]]
        assert {0, 1, 2, 3, 4} <= set(top.tolist())


@pytest.mark.parametrize("k", sc.PIPE_K)
def test_eval_pipeline_case_is_dyadic_and_the_oracle_drops_exactly_the_plants(k):
    clean, out = sc.rpn_dyadic(), sc.pipeline_case()
    logits, deltas = sc.split(clean)
    assert _dyadic(deltas) and (deltas[..., 2:] == 0).all() and _dyadic(logits, 64)
    assert len(torch.unique(logits[0])) == sc.NA and len(torch.unique(logits[1])) == sc.NA
    for b in range(sc.RB):
        box = OB.apply_deltas(deltas[b], sc.anchors(), sc.RPN_W)
        assert torch.equal(box.double(), sc.apply_deltas(deltas[b].double(), sc.anchors().double(), sc.RPN_W)) and _dyadic(box)
    logits, deltas = sc.split(out)
    ref = sc.pipeline_definition(out, k)
    ref_clean = sc.pipeline_definition(clean, k)
    for b in range(sc.RB):
        boxes = OB.apply_deltas(deltas[b], sc.anchors(), sc.RPN_W)
        order = torch.sort(logits[b], descending=True, stable=True)[1][:k]
        bad = ~(torch.isfinite(boxes).all(1) & torch.isfinite(logits[b]))
        plants = {i for bb, i, _, _ in sc.PIPE_PLANTS if bb == b}
        assert set(torch.nonzero(bad).flatten().tolist()) == plants
        in_topk = plants & set(order.tolist())
        # NaN and +inf rank first, a broken box carries a top logit; -inf is inside the top k only when k == NA
        minus = {i for bb, i, f, v in sc.PIPE_PLANTS if bb == b and f == "logit" and v == -sc.INF}
        assert in_topk == (plants if k == sc.NA else plants - minus)
        assert torch.isnan(logits[b][order[0]])                        # what the device must not hand on
        n = len(ref[b][1])
        assert 10 <= n <= sc.PIPE_POST and torch.isfinite(ref[b][1]).all() and torch.isfinite(ref[b][0]).all()
        assert n >= 10 and len(ref_clean[b][1]) >= 10
        # the survivors are the clean run's without the planted anchors (a plant may also have suppressed a neighbour there)
        kept_scores = set(ref[b][1].tolist())
        assert not kept_scores & {50.0 + i for i in plants}


# ---- B. teacher ------------------------------------------------------------------------------------------------------------
LAYOUTS = [(8, False), (8, True), (32, False), (32, True)]


@pytest.mark.parametrize("K,agnostic", LAYOUTS)
def test_teacher_case_is_dyadic_padded_and_clear_of_the_threshold(K, agnostic):
    c = sc.teacher_case(K, agnostic)
    cols = K + 1 + 4 * c["nreg"]
    assert c["pred"].shape == (sc.TB * sc.TP, sc.ld_of(cols)) and c["pred"].shape[1] > cols and sc.TP <= 128
    assert (c["pred"][:, cols:] == 0).all() and c["pc"].tolist() == [96, 70]
    d = sc.deltas_of(c).view(-1, c["nreg"], 4)
    assert _dyadic(c["props"], 1) and (d[..., 2:] == 0).all() and _dyadic(d[..., :2] / np.float32(10.0))
    for b in range(sc.TB):
        rows = slice(b * sc.TP, (b + 1) * sc.TP)
        b32 = OB.apply_deltas(sc.deltas_of(c)[rows], c["props"][b], sc.ROI_W)
        b64 = sc.apply_deltas(sc.deltas_of(c)[rows].double(), c["props"][b].double(), sc.ROI_W)
        assert torch.equal(b32.double(), b64)                          # exact decodes
    for sigmoid in (False, True):
        p = sc.probs_of(sc.scores_of(c).double(), sigmoid)[:, :K]
        assert (p - sc.SCORE_THRESH).abs().min().item() >= 1e-6        # asserted, not arranged: nothing is drawn again
        assert (p - sc.PSEUDO_THR).abs().min().item() >= 1e-6          # (the strict edges have their own tests)
        ref = sc.teacher_definition(c, sigmoid)
        for b in range(sc.TB):
            assert len(ref[b]["scores"]) >= 10 and ref[b]["cand"] >= len(ref[b]["scores"])
            cs = torch.sort(p.view(sc.TB, sc.TP, K)[b, : int(c["pc"][b])].flatten(), descending=True)[0]
            cs = cs[cs > sc.SCORE_THRESH]
            gaps = (cs[:-1] - cs[1:]) / cs[1:]
            rel = gaps[gaps > 0].min().item()
            assert rel == 0 or rel >= 1e-4, rel                        # the candidates' order is not a rounding question


@pytest.mark.parametrize("K", [8, 32])
def test_teacher_definition_is_the_oracles_inference_in_softmax_mode(K):
    c = sc.teacher_case(K, False)
    a, b = sc.teacher_definition(c, False), sc.softmax_definition(c)
    for x, y in zip(a, b):
        for key in ("boxes", "scores", "classes", "roi_idx"):
            assert torch.equal(x[key], y[key]), key


@pytest.mark.parametrize("sigmoid", [False, True])
@pytest.mark.parametrize("K,agnostic", LAYOUTS[:2])
@pytest.mark.parametrize("name,kind,value", sc.ROW_PLANTS)
def test_the_oracle_drops_exactly_the_planted_row(name, kind, value, K, agnostic, sigmoid):
    base = sc.teacher_case(K, agnostic)
    case, b, j = sc.row_plant_case(base, name)
    assert int((_bits(case["pred"]) != _bits(base["pred"])).sum()) == 1 and j < int(base["pc"][b])
    ref0, ref1 = sc.teacher_definition(base, sigmoid), sc.teacher_definition(case, sigmoid)
    for i in range(sc.TB):
        rows0 = list(zip(ref0[i]["cand_rows"].tolist(), ref0[i]["cand_classes"].tolist()))
        rows1 = list(zip(ref1[i]["cand_rows"].tolist(), ref1[i]["cand_classes"].tolist()))
        assert rows1 == [rc for rc in rows0 if not (i == b and rc[0] == j)]
        assert len(ref1[i]["scores"]) >= 10
    assert any(r == j for r in ref0[b]["cand_rows"].tolist())           # the row had candidates to lose


@pytest.mark.parametrize("sigmoid", [False, True])
def test_padding_rows_would_count_if_they_were_read(sigmoid):
    base, case = sc.padding_case(sc.teacher_case(8, False))
    assert base["pc"].tolist() == [70, 96]
    assert torch.equal(_bits(base["pred"][:70]), _bits(case["pred"][:70])) and torch.equal(base["pred"][96:], case["pred"][96:])
    pad = case["pred"][70:96, :9]
    assert torch.isnan(pad[0::2]).all() and (pad[1::2, :8] == 100).all()
    p = sc.probs_of(pad[1::2], sigmoid)[:, :8]
    assert (p > sc.SCORE_THRESH).all()
    a, b = sc.teacher_definition(base, sigmoid), sc.teacher_definition(case, sigmoid)
    for x, y in zip(a, b):
        assert torch.equal(x["scores"], y["scores"]) and len(x["scores"]) >= 10


@pytest.mark.parametrize("sigmoid", [False, True])
def test_saturated_rows_saturate_in_torch_fp32(sigmoid):
    case, up, down = sc.saturated_case(sc.teacher_case(8, False), sigmoid)
    p = sc.probs_of(sc.scores_of(case), sigmoid)
    for r, c in up:
        assert p[r, c].item() == 1.0
        rest = torch.cat([p[r, :c], p[r, c + 1:8]])
        assert (rest < 1e-20).all() and (rest > 0).all()               # ~ e^-60: far from expf's underflow
    for r, c in down:
        assert 0 < p[r, c].item() < 1e-20 and (torch.cat([p[r, :c], p[r, c + 1:8]]) > sc.SCORE_THRESH).all()
    ref = sc.teacher_definition(case, sigmoid)
    for b in range(sc.TB):
        assert len(ref[b]["scores"]) >= 10 and (ref[b]["scores"] == 1.0).sum() >= 3
        assert len(om.threshold_bbox(ref[b], sc.PSEUDO_THR)["scores"]) >= 3


@pytest.mark.parametrize("sigmoid", [False, True])
@pytest.mark.parametrize("K,agnostic", LAYOUTS[:2])
def test_max_det_case_has_one_survivor_per_row_and_distinct_scores(K, agnostic, sigmoid):
    c = sc.max_det_case(K, agnostic, sigmoid)
    assert c["pc"].tolist() == [100, 101] and c["props"].shape[1] == 101 <= 128
    iou = OB.pairwise_iou(c["props"][0], c["props"][0])
    assert (iou - torch.eye(101)).abs().max().item() == 0              # non-overlapping
    p = sc.probs_of(sc.scores_of(c), sigmoid)[:101, :K]
    assert ((p > sc.SCORE_THRESH).sum(1) == 1).all()
    best = p.max(1).values
    assert len(torch.unique(best)) == 101 and (best[1:] > best[:-1]).all() and best.min() > 0.8
    for limit in (100, 1000):
        ref = sc.teacher_definition(c, sigmoid, max_det=limit)
        assert [len(r["scores"]) for r in ref] == [100, min(limit, 101)]
    ref = sc.teacher_definition(c, sigmoid)
    assert sorted(ref[1]["roi_idx"].tolist()) == list(range(1, 101))    # the dropped one is the lowest score: row 0
    assert sorted(ref[0]["roi_idx"].tolist()) == list(range(100))


@pytest.mark.parametrize("K,agnostic", LAYOUTS[:2])
def test_decode_clamp_case_is_beyond_the_clamp_and_inside_the_image(K, agnostic):
    case, rows = sc.decode_clamp_case(K, agnostic)
    for b, j in rows:
        r = b * sc.TP + j
        q = case["pred"][r, sc.delta_col(case, 1, 2 + b)].double().item() / sc.ROI_W[2 + b]
        assert q >= sc.CLAMP64 + 0.999
    ref = sc.teacher_definition(case, False, dtype=torch.float64)
    for b, j in rows:
        hit = torch.nonzero((ref[b]["roi_idx"] == j) & (ref[b]["classes"] == 1)).flatten()
        assert len(hit) == 1
        box = ref[b]["boxes"][hit[0]]
        ext = (box[2] - box[0], box[3] - box[1])
        assert ext[b].item() == pytest.approx(1000.0, rel=1e-12) and ext[1 - b].item() == 16.0
        assert box.min() > 0 and box.max() < 2048                      # not clipped


# ---- C. BPC ----------------------------------------------------------------------------------------------------------------
def _tp_fp(case):
    loss, inst, gts = sc.bpc_definition(case)
    conf = sc.bpc_confusions(inst, gts, case["K"], case["iou_thr"])
    return loss, inst, gts, conf


@pytest.mark.parametrize("name", sc.BPC_NAMES)
def test_bpc_hand_cases_are_dyadic_identities_with_both_kinds_of_detection(name):
    case = sc.bpc_case(name)
    K = case["K"]
    assert _dyadic(case["rois"], 1) and _dyadic(case["gtb"], 1) and case["pred"].shape[1] > 5 * K + 1
    loss, inst, gts, conf = _tp_fp(case)
    flat = [r for img in conf for r in img]
    assert any(r[0] > 0 for r in flat) and any(r[0] == 0 for r in flat)
    assert loss.dtype == torch.float64 and loss.item() > 0
    live = case["rois"][:, 0] == 0
    if name != "background-row":                                       # both decodes are identities: detections = ROIs
        assert (sc.deltas_of(dict(case, nreg=K)) == 0).all()
        assert torch.equal(inst[0]["boxes"].view(-1, K, 4)[:, 0], case["rois"][live, 1:].double())
    img0, F = conf[0], sc.N_FILL
    if name == "score-half":
        z = case["pred"][:, :2]
        p32 = torch.softmax(z, dim=1)
        halves = torch.nonzero(z[:, 0] == z[:, 1]).flatten()
        assert len(halves) == 3 and (_bits(p32[halves, 0]) == _bits(torch.tensor([0.5] * 3))).all()
        assert sorted(r[0] for r in img0 if r[1] == 0.5) == [0, 1, 1]
    elif name in ("iou-half", "iou-above-half"):
        iou = sc.legacy_iou(torch.tensor([sc.GT_BOX]), case["rois"][2 * F:2 * F + 1, 1:])[0, 0].item()
        assert iou == (0.5 if name == "iou-half" else 0.6)
        assert img0[F * K][0] == (0 if name == "iou-half" else 1) and img0[F * K][3] == iou      # row 2, class 0
    elif name == "tie":
        assert img0[F * K][0] == 2 and img0[F * K][3] == 100.0 / 150.0
    elif name == "no-gt-of-class":
        assert img0[F * K + 1] == (0, img0[F * K + 1][1], 1, None) and img0[F * K + 1][1] > 0.99
    elif name == "background-row":
        assert case["roi_cls"][2 * F].item() == K
        assert inst[0]["boxes"].view(-1, K, 4)[F].tolist() == [[48, 40, 64, 56], [56, 40, 72, 56]]
        assert img0[F * K][0] == 1 and img0[F * K][3] == 1.0
        unclamped = sc.legacy_iou(torch.tensor([[48.0, 40, 64, 56]]), torch.tensor([[40.0, 40, 56, 56]]))[0, 0].item()
        assert unclamped < 0.5
    elif name == "padding-rows":
        assert sorted(case["rois"][2 * F:, 0].tolist()) == [-1, -1, 2, 7]
        assert len(inst[0]["scores"]) == F * K and len(inst[1]["scores"]) == F * K


def test_bpc_decisions_move_the_loss_far_beyond_the_gate():
    """each hand case against its neighbour: the decision under test is worth more than 1000 gates"""
    def value(name):
        return sc.bpc_definition(sc.bpc_case(name))[0].item()
    fill = value("padding-rows")                                       # the fillers alone
    assert abs(value("iou-half") - value("iou-above-half")) > 1e-3
    for name in ("score-half", "tie", "no-gt-of-class", "background-row", "iou-half"):
        assert abs(value(name) - fill) > 1e-4, name              # the gate is ~ 4 * 2^-24 * 0.03 = 7e-9
    # score exactly 0.5 on the other side of `>=`
    case = sc.bpc_case("score-half")
    loss, inst, gts = sc.bpc_definition(case)
    below = [dict(d, scores=torch.where(d["scores"] == 0.5, torch.nextafter(d["scores"], torch.zeros(())), d["scores"])) for d in inst]
    assert abs(om.bpc_loss(1, gts, below).item() - loss.item()) > 1e-2


def test_bpc_mixed_case_mixes_images_in_one_wavefront_and_not_in_another():
    case = sc.bpc_mixed_case()
    K = case["K"]
    waves = sc.wave_images(case)
    assert len(waves) == 5 and waves[0] == {0} and waves[1] == {0, 1} and waves[2] == waves[3] == waves[4] == {1}
    assert len(case["rois"]) * K > 256                                 # two blocks
    assert int((case["rois"][:, 0] < 0).sum()) >= 10
    assert _dyadic(case["rois"], 1) and _dyadic(case["gtb"], 1) and (sc.deltas_of(dict(case, nreg=K)) == 0).all()
    loss, inst, gts, conf = _tp_fp(case)
    for img in conf:
        assert sum(1 for r in img if r[0] > 0) >= 5 and sum(1 for r in img if r[0] == 0) >= 5
    p = torch.cat([d["scores"] for d in inst])
    assert (p - 0.5).abs().min().item() >= 1e-5 and 200 < len(p) <= 300
    # IoUs are ratios of small integers: a pair of them is either equal or apart by far more than an fp32 rounding
    for d, (gb, gc) in zip(inst, gts):
        for c in range(K):
            if (gc == c).any() and (d["classes"] == c).any():
                iou = sc.legacy_iou(gb[gc == c], d["boxes"][d["classes"] == c])
                gap = (iou[:, None, :] - iou[None, :, :]).abs()
                assert ((gap == 0) | (gap > 1e-6)).all()
                assert (((iou - 0.5).abs() > 1e-6) | (iou == 0.5)).all()
    assert loss.item() > 0.01


def test_the_gpu_test_and_its_inputs_read_no_reference_tree():
    """neither file names the reference checkout or the binaries built from it: definitions come from oracle/*.py alone"""
    here = os.path.dirname(os.path.abspath(__file__))
    for path in (os.path.join(here, "helpers", "score_edge_cases.py"), os.path.join(here, "test_gpu_score_edges.py")):
        with open(path) as f:
            src = f.read()
        assert "_ref" + "/" not in src and "_ref" + os.sep not in src and "reference" + "/" not in src
