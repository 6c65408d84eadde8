"""Inputs of tests/test_gpu_score_edges.py: the score-side kernels of csrc/detect.hip (RPN decode and top-k gather, the
teacher's candidates / probabilities / NMS preparation / finalize, the BPC sums) at their threshold and non-finite edges.

CPU only, fixed seeds, nothing is excluded or drawn again.  Wherever a decision has to be exact the geometry is dyadic:
integer cell anchors / proposals and deltas that are zero or a pure translation by a multiple of 1/16 of the box (dw = dh = 0,
so expf(0) * w == w and dx * w + cx is exact in fp32): the decoded boxes are then the same bits on the device and in
oracle/box_ops.py.  tests/test_score_edge_cases_host.py holds every generator to the edge it is named for and checks that the
oracle alone behaves as the GPU test assumes.

The definitions are oracle/model.py (rpn_proposals, fast_rcnn_inference, threshold_bbox, bpc_loss) and oracle/box_ops.py.
``teacher_definition`` and ``bpc_definition`` only feed them: the first is om.fast_rcnn_inference with the probabilities
as an argument (the sigmoid head has no softmax; in softmax mode the host test holds it to om.fast_rcnn_inference itself).
OB.apply_deltas casts its deltas to float32 as Detectron2 does, so the float64 side of the clamp gates is ``apply_deltas``
below: the same operations without the cast, the same bits as OB.apply_deltas in float32 (held by the host test).
"""
import functools
import math

import numpy as np
import torch

from oracle import box_ops as OB
from oracle import model as om

NAN, INF = float("nan"), float("inf")
CLAMP64 = math.log(1000.0 / 16)
CLAMP32 = float(np.float32(CLAMP64))                       # the kernels' constant: float32(log(1000 / 16))
CLAMP32_BELOW = float(np.nextafter(np.float32(CLAMP64), np.float32(0)))
CLAMP32_ABOVE = float(np.nextafter(np.float32(CLAMP64), np.float32(10)))
RPN_W, RPN_W2 = (1.0, 1.0, 1.0, 1.0), (2.0, 2.0, 1.0, 1.0)
ROI_W = (10.0, 10.0, 5.0, 5.0)


def gate(ref64, val32, s):
    """4 x max(torch-fp32's distance from float64, 2^-24 * s) -> (gate, e32): tests/test_gpu_box_reg_options.py's"""
    e32 = (val32.double() - ref64.double()).abs().max().item()
    return 4.0 * max(e32, 2.0 ** -24 * float(s)), e32


def apply_deltas(deltas, boxes, weights):
    """OB.apply_deltas (Box2BoxTransform.apply_deltas) in the dtype of ``deltas``: the oracle's casts its deltas to float32 as
    Detectron2 does, so a float64 definition needs the same operations without that cast.  In float32 the two are the same
    bits (tests/test_score_edge_cases_host.py)."""
    boxes = boxes.to(deltas.dtype)
    wx, wy, ww, wh = weights
    widths = boxes[:, 2] - boxes[:, 0]
    heights = boxes[:, 3] - boxes[:, 1]
    ctr_x = boxes[:, 0] + 0.5 * widths
    ctr_y = boxes[:, 1] + 0.5 * heights
    dx = deltas[:, 0::4] / wx
    dy = deltas[:, 1::4] / wy
    dw = torch.clamp(deltas[:, 2::4] / ww, max=OB.SCALE_CLAMP)
    dh = torch.clamp(deltas[:, 3::4] / wh, max=OB.SCALE_CLAMP)
    pcx = dx * widths[:, None] + ctr_x[:, None]
    pcy = dy * heights[:, None] + ctr_y[:, None]
    pw = torch.exp(dw) * widths[:, None]
    ph = torch.exp(dh) * heights[:, None]
    return torch.stack((pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph), dim=-1).reshape(deltas.shape)


def ld_of(cols):
    """row stride of a prediction matrix: whole 16-byte chunks and at least one padding column"""
    return (cols + 8) // 8 * 8


# ---- A. RPN ----------------------------------------------------------------------------------------------------------------
RB, HF, WF, A, STRIDE = 2, 10, 9, 3, 16
NA = HF * WF * A                                            # 270: two 256-thread blocks, anchor 269 is the tail block's last lane
LD = 16                                                     # > 5 A = 15: one padding column
CELL = torch.tensor([[0.0, 0, 16, 16], [-12, -6, 12, 6], [-4, -10, 4, 10]])
RPN_SIZES = [(160, 144), (100, 90)]                         # image 0: the anchor grid exactly; image 1: smaller
FIELDS = {"logit": None, "dx": 0, "dy": 1, "dw": 2, "dh": 3}


def anchors():
    return OB.grid_anchors(HF, WF, STRIDE, CELL)


def rpn_zero():
    return torch.zeros(RB * HF * WF, LD)


def rpn_finite(seed=5):
    """random finite head output: logits ~ 2 N(0, 1), deltas ~ 0.3 N(0, 1), padding column 0"""
    g = torch.Generator().manual_seed(seed)
    out = rpn_zero()
    out[:, :A] = torch.randn(RB * HF * WF, A, generator=g) * 2
    out[:, A:5 * A] = torch.randn(RB * HF * WF, 4 * A, generator=g) * 0.3
    return out


def rpn_dyadic(seed=6):
    """distinct finite logits; deltas = translations by multiples of 1/16 of the anchor, no scaling: exact decodes"""
    g = torch.Generator().manual_seed(seed)
    out = rpn_zero()
    out[:, :A] = (torch.randperm(RB * HF * WF * A, generator=g).float().view(-1, A) - 400) / 64
    d = torch.zeros(RB * HF * WF, A, 4)
    d[:, :, :2] = torch.randint(-12, 13, (RB * HF * WF, A, 2), generator=g).float() / 16
    out[:, A:5 * A] = d.view(-1, 4 * A)
    return out


def plant(out, b, i, field, value):
    """write ``value`` into the logit / delta of anchor i of image b ("pad": the padding column of its row)"""
    row, a = b * HF * WF + i // A, i % A
    col = 5 * A if field == "pad" else (a if field == "logit" else A + 4 * a + FIELDS[field])
    out[row, col] = value
    return out


def split(out):
    """-> logits [B, NA], deltas [B, NA, 4] in the oracle's layout"""
    return out[:, :A].reshape(RB, NA), out[:, A:5 * A].reshape(RB, NA, 4)


# (name, field, value, raises the divergence flag)
FLAG_PLANTS = [
    ("nan-logit", "logit", NAN, True), ("+inf-logit", "logit", INF, True), ("-inf-logit", "logit", -INF, True),
    ("nan-dx", "dx", NAN, True), ("nan-dy", "dy", NAN, True), ("nan-dw", "dw", NAN, True), ("nan-dh", "dh", NAN, True),
    ("+inf-dx", "dx", INF, True), ("-inf-dx", "dx", -INF, True),
    ("+inf-dw", "dw", INF, False),                          # clamped like torch.clamp(max=): a finite box
    ("-inf-dw", "dw", -INF, False),                         # expf(-inf) = 0: width 0, finite
    ("nan-pad", "pad", NAN, False), ("+inf-pad", "pad", INF, False), ("-inf-pad", "pad", -INF, False),
]
FLAG_PLACES = [(0, 0), (1, NA - 1)]


def flag_case(name, place):
    field, value = next((f, v) for n, f, v, _ in FLAG_PLANTS if n == name)
    return plant(rpn_finite(), place[0], place[1], field, value)


def oracle_raises(out, weights=RPN_W):
    """what Detectron2 tests: a non-finite decoded box or logit anywhere"""
    logits, deltas = split(out)
    fin = torch.isfinite(logits).all()
    for b in range(RB):
        fin = fin and torch.isfinite(OB.apply_deltas(deltas[b], anchors(), weights)).all()
    return not bool(fin)


CLAMP_VALUES = [("at", CLAMP32), ("below", CLAMP32_BELOW), ("above", CLAMP32_ABOVE), ("ten", 10.0)]
CLAMP_ANCHORS = [0, 100, NA - 1]
CLAMP_SIZES = [(4096, 4096), (4096, 4096)]                  # nothing of a clamped box is clipped away


def clamp_case(value, weights):
    """dw / ww = ``value`` on three anchors of image 0 and dh / wh = ``value`` on the same of image 1, each pushed 40 box sizes
    into the image (dx / wx = dy / wy = 40) so that the 62.5-fold box stays inside it"""
    out = rpn_finite(seed=7)
    for i in CLAMP_ANCHORS:
        plant(out, 0, i, "dw", value * weights[2])
        plant(out, 0, i, "dx", 40.0 * weights[0])
        plant(out, 0, i, "dy", 40.0 * weights[1])
        plant(out, 1, i, "dh", value * weights[3])
        plant(out, 1, i, "dx", 40.0 * weights[0])
        plant(out, 1, i, "dy", 40.0 * weights[1])
    return out


def decode_definition(out, weights, sizes, dtype):
    """apply_deltas + OB.clip_boxes evaluated in ``dtype`` -> [B, NA, 4]"""
    _, deltas = split(out)
    return torch.stack([OB.clip_boxes(apply_deltas(deltas[b].to(dtype), anchors().to(dtype), weights), sizes[b])
                        for b in range(RB)])


MIN_SIZE = 8.0


def min_size_case(seed=8):
    """integer boxes [B, NA, 4] with distinct scores; planted: width exactly MIN_SIZE (invalid: the test is strict), MIN_SIZE + 1
    (valid), height exactly MIN_SIZE under a larger width (invalid), a zero-extent box (invalid at min_size 0 too)"""
    g = torch.Generator().manual_seed(seed)
    xy = torch.randint(0, 100, (RB, NA, 2), generator=g).float()
    wh = torch.randint(1, 30, (RB, NA, 2), generator=g).float()
    props = torch.cat([xy, xy + wh], 2)
    planted = {"width-eq": (0, (8.0, 20.0)), "width-plus-1": (1, (9.0, 20.0)), "height-eq": (2, (20.0, 8.0)),
               "both-plus-1": (3, (9.0, 9.0)), "zero-extent": (4, (0.0, 0.0)), "zero-width": (NA - 1, (0.0, 12.0))}
    for b in range(RB):
        for i, (w, h) in planted.values():
            props[b, i, 2:] = props[b, i, :2] + torch.tensor([w, h])
    scores = torch.randperm(RB * NA, generator=g).float().view(RB, NA) / 8 - 20     # the planted rows rank anywhere
    scores[:, :5] += 100                                                         # ... the first five inside every top-k
    return props, scores, planted


PIPE_K = [200, NA]
PIPE_POST = 100
# (image, anchor, field, value): non-finite logits on finite boxes, non-finite deltas under a top-ranked logit
PIPE_PLANTS = [(0, 7, "logit", NAN), (0, 50, "logit", INF), (0, 120, "logit", -INF), (0, 200, "dx", NAN), (0, 201, "dw", NAN),
               (1, NA - 1, "logit", NAN), (1, 3, "logit", NAN), (1, 60, "logit", -INF), (1, 90, "dy", INF), (1, 91, "dx", -INF)]
PIPE_SIZES = RPN_SIZES


def pipeline_case():
    out = rpn_dyadic()
    for b, i, field, value in PIPE_PLANTS:
        plant(out, b, i, field, value)
        if field != "logit":
            plant(out, b, i, "logit", 50.0 + i)              # the broken box is among the best k
    return out


def pipeline_definition(out, k):
    cfg = om.Cfg(rpn_pre_topk_test=k, rpn_post_topk_test=PIPE_POST)
    logits, deltas = split(out)
    return om.rpn_proposals(anchors(), logits, deltas, PIPE_SIZES, cfg, training=False)


# ---- B. teacher post-processing --------------------------------------------------------------------------------------------
TB, TP = 2, 96
T_SIZES = [(600, 1200), (590, 1100)]
SCORE_THRESH, NMS_THRESH, MAX_DET, PSEUDO_THR = 0.05, 0.5, 100, 0.8


def probs_of(scores, sigmoid):
    return torch.sigmoid(scores) if sigmoid else torch.softmax(scores, dim=-1)


def pred_matrix(scores, deltas):
    """[R, K + 1] scores and [R, 4 nreg] deltas -> the head's output matrix with its padded row stride"""
    cols = scores.shape[1] + deltas.shape[1]
    pred = torch.zeros(scores.shape[0], ld_of(cols))
    pred[:, :scores.shape[1]] = scores
    pred[:, scores.shape[1]:cols] = deltas
    return pred


def lattice_boxes(n, g, span=(1000, 500)):
    """n integer boxes: power-of-two sizes 16 ... 128 at integer positions (every 1/16 translation of one is exact)"""
    xy = torch.stack([torch.randint(0, span[0], (n,), generator=g), torch.randint(0, span[1], (n,), generator=g)], 1).float()
    wh = 2.0 ** torch.randint(4, 8, (n, 2), generator=g).float()
    return torch.cat([xy, xy + wh], 1)


def _case(K, agnostic, props, scores, deltas):
    nreg = 1 if agnostic else K
    return {"K": K, "agnostic": agnostic, "nreg": nreg, "props": props, "pc": torch.tensor([TP, TP - 26], dtype=torch.int32),
            "pred": pred_matrix(scores, deltas.view(TB * TP, -1)), "sizes": T_SIZES}


def _translations(n, nreg, g):
    """deltas = translations by multiples of 1/16 of the proposal (dx = 10 k / 16: exactly k / 16 after the division by wx = 10)"""
    d = torch.zeros(n, nreg, 4)
    d[:, :, :2] = torch.randint(-8, 9, (n, nreg, 2), generator=g).float() * 10 / 16
    return d


TOP_STEP, SECOND_GAP, REST = 1.0 / 32, 2.0, -8.0


@functools.lru_cache(maxsize=None)
def teacher_case(K=8, agnostic=False, seed=21):
    """B = 2, P = 96 (96 and 70 live rows), dyadic proposals and translations.  The scores are on a lattice, so that two
    implementations of the probabilities rank the candidates alike: per image row r has one class at u = perm(r) / 32 in [0, 3),
    another at u - 2, the background at 0 and the rest at -8.  Softmax: top probabilities 0.47 ... 0.84 at least 4e-3 apart,
    second ones e^-2 times that (0.06 ... 0.11); sigmoid: equal logits give equal bits, different ones differ by >= 1e-3."""
    g = torch.Generator().manual_seed(seed + K + 100 * agnostic)
    props = lattice_boxes(TB * TP, g).view(TB, TP, 4)
    scores = torch.full((TB * TP, K + 1), REST)
    scores[:, K] = 0.0
    for b in range(TB):
        u = torch.randperm(TP, generator=g).float() * TOP_STEP
        c1 = torch.randint(0, K, (TP,), generator=g)
        c2 = (c1 + torch.randint(1, K, (TP,), generator=g)) % K
        rows = torch.arange(b * TP, (b + 1) * TP)
        scores[rows, c1], scores[rows, c2] = u, u - SECOND_GAP
    return _case(K, agnostic, props, scores, _translations(TB * TP, 1 if agnostic else K, g))


@functools.lru_cache(maxsize=None)
def teacher_random_case(K=8, agnostic=False, seed=22):
    """the same shapes with scores ~ 3 N(0, 1): for the tests that take their thresholds from the device's own probabilities"""
    g = torch.Generator().manual_seed(seed + K + 100 * agnostic)
    props = lattice_boxes(TB * TP, g).view(TB, TP, 4)
    scores = torch.randn(TB * TP, K + 1, generator=g) * 3
    return _case(K, agnostic, props, scores, _translations(TB * TP, 1 if agnostic else K, g))


def with_pred(case, pred, **kw):
    out = dict(case)
    out["pred"] = pred
    out.update(kw)
    return out


def scores_of(case):
    return case["pred"][:, :case["K"] + 1]


def deltas_of(case):
    K = case["K"]
    return case["pred"][:, K + 1:K + 1 + 4 * case["nreg"]]


def delta_col(case, c, j):
    return case["K"] + 1 + (0 if case["agnostic"] else 4 * c) + j


def teacher_definition(case, sigmoid, score_thresh=SCORE_THRESH, max_det=MAX_DET, dtype=torch.float32):
    """om.fast_rcnn_inference with ``probs_of`` in the softmax's place and the class-agnostic deltas tiled K times"""
    K, P = case["K"], case["props"].shape[1]
    cfg = om.Cfg(num_classes=K, test_score_thresh=score_thresh, test_dets=max_det)
    out = []
    for b in range(case["props"].shape[0]):
        n = int(case["pc"][b])
        rows = slice(b * P, b * P + n)
        sc = probs_of(scores_of(case)[rows].to(dtype), sigmoid)
        dl = deltas_of(case)[rows].to(dtype).repeat(1, K // case["nreg"])
        bx = apply_deltas(dl, case["props"][b, :n].to(dtype), cfg.roi_bbox_weights)
        valid = torch.isfinite(bx).all(dim=1) & torch.isfinite(sc).all(dim=1)
        roi_ids = torch.arange(n)[valid]
        bx, sc = bx[valid], sc[valid][:, :-1]
        bx = OB.clip_boxes(bx.reshape(-1, 4), case["sizes"][b]).view(-1, K, 4)
        mask = sc > cfg.test_score_thresh
        inds = mask.nonzero()
        cb, cs = bx[mask], sc[mask]
        keep = OB.batched_nms(cb, cs, inds[:, 1], cfg.test_nms_thresh, cfg.nms_numel_limit)[: cfg.test_dets]
        out.append({"boxes": cb[keep], "scores": cs[keep], "classes": inds[keep, 1], "roi_idx": roi_ids[inds[keep, 0]],
                    "cand": int(mask.sum()), "cand_rows": roi_ids[inds[:, 0]], "cand_classes": inds[:, 1]})
    return out


def softmax_definition(case):
    """om.fast_rcnn_inference itself (per-class layout, softmax)"""
    K, P = case["K"], case["props"].shape[1]
    B = case["props"].shape[0]
    live = [slice(b * P, b * P + int(case["pc"][b])) for b in range(B)]
    cfg = om.Cfg(num_classes=K)
    return om.fast_rcnn_inference(torch.cat([scores_of(case)[r] for r in live]), torch.cat([deltas_of(case)[r] for r in live]),
                                  [case["props"][b, : int(case["pc"][b])] for b in range(B)], case["sizes"], cfg)


# (name, column kind, value)
ROW_PLANTS = [("nan-score", "score", NAN), ("+inf-dx", "dx", INF), ("nan-dw", "dw", NAN)]
ROW_PLANT_ROWS = {"nan-score": (0, 5), "+inf-dx": (0, 40), "nan-dw": (1, 69)}      # (image, row): 69 is image 1's last live row
ROW_PLANT_CLASS = 3


def row_plant_case(case, name):
    kind, value = next((k, v) for n, k, v in ROW_PLANTS if n == name)
    b, j = ROW_PLANT_ROWS[name]
    pred = case["pred"].clone()
    c = min(ROW_PLANT_CLASS, case["K"] - 1)
    col = c if kind == "score" else delta_col(case, c, FIELDS[kind])
    pred[b * TP + j, col] = value
    return with_pred(case, pred), b, j


def padding_case(case):
    """image 0's rows at and beyond prop_count are filled: NaN scores on the even rows, +100 logits on every class of the odd ones"""
    pc = torch.tensor([TP - 26, TP], dtype=torch.int32)
    base = with_pred(case, case["pred"].clone(), pc=pc)
    base["pred"][int(pc[0]):TP] = 0
    pred = base["pred"].clone()
    K = case["K"]
    for j in range(int(pc[0]), TP):
        pred[j, :K + 1] = NAN if j % 2 == 0 else 100.0
        pred[j, K] = NAN if j % 2 == 0 else -100.0          # (softmax: the odd rows' foreground classes share the mass)
    return base, with_pred(base, pred)


def saturated_case(case, sigmoid):
    """logit gaps of +-60: every fourth row has one class 60 above the rest (softmax) or at +60 with the rest at -60 (sigmoid) --
    probability exactly 1.0, the others ~ e^-60; every fourth-plus-one row has one class 60 below the rest"""
    pred = case["pred"].clone()
    K = case["K"]
    up, down = [], []
    for r in range(0, pred.shape[0], 4):
        c = (r // 4) % K
        pred[r, :K + 1] = -60.0 if sigmoid else 0.0
        pred[r, c] = 60.0
        up.append((r, c))
        pred[r + 1, :K + 1] = 0.0
        pred[r + 1, c] = -60.0
        down.append((r + 1, c))
    return with_pred(case, pred), up, down


def max_det_case(K, agnostic, sigmoid):
    """101 non-overlapping 16 x 16 boxes on a 20-pixel lattice, zero deltas, one class per row above the score threshold with
    its own score: NMS keeps them all.  Image 0 has 100 live rows, image 1 all 101 (its lowest score is row 0's)."""
    P = MAX_DET + 1
    i = torch.arange(P)
    xy = torch.stack([(i % 11) * 20, (i // 11) * 20], 1).float()
    props = torch.cat([xy, xy + 16], 1).repeat(2, 1, 1)
    scores = torch.full((2 * P, K + 1), -6.0 if sigmoid else 0.0)
    target = ((2.0 if sigmoid else 5.0) + 0.05 * i.float()).repeat(2)
    scores[torch.arange(2 * P), i.repeat(2) % K] = target
    nreg = 1 if agnostic else K
    return {"K": K, "agnostic": agnostic, "nreg": nreg, "props": props, "pc": torch.tensor([MAX_DET, P], dtype=torch.int32),
            "pred": pred_matrix(scores, torch.zeros(2 * P, 4 * nreg)), "sizes": [(240, 240), (240, 240)]}


def decode_clamp_case(K, agnostic):
    """one row per image whose class 1 is saturated and has dw / ww (image 0) or dh / wh (image 1) one above the clamp; its
    proposal is 16 x 16 in the middle of a 2048 x 2048 image, so the 1000-pixel box is not clipped"""
    case = teacher_case(K, agnostic)
    pred, props = case["pred"].clone(), case["props"].clone()
    rows = [(0, 11), (1, 12)]
    for b, j in rows:
        r = b * TP + j
        props[b, j] = torch.tensor([1000.0, 1008.0, 1016.0, 1024.0])
        pred[r, :K + 1] = 0.0
        pred[r, 1] = 60.0
        pred[r, K + 1:] = 0.0
        pred[r, delta_col(case, 1, 2 + b)] = ROI_W[2 + b] * (CLAMP64 + 1.0)
    return with_pred(case, pred, props=props, sizes=[(2048, 2048), (2048, 2048)]), rows


# ---- C. BPC ----------------------------------------------------------------------------------------------------------------
BPC_SIZES = [(200, 320), (220, 260)]
G_CAP = 8
LOGIT_HI, LOGIT_LO = 3.0, -3.0


def _bpc_pack(K, rows, gts, B=2, sizes=BPC_SIZES, iou_thr=0.5):
    """rows: (image index as stored in the ROI, box, gt class, scores [K + 1], deltas [K, 4] or None); gts: per image
    [(box, class)] -> the arrays sfod_bpc_loss takes"""
    R = len(rows)
    scores = torch.tensor([r[3] for r in rows], dtype=torch.float32).view(R, K + 1)
    deltas = torch.zeros(R, K, 4)
    for i, r in enumerate(rows):
        if r[4] is not None:
            deltas[i] = torch.tensor(r[4], dtype=torch.float32)
    rois = torch.tensor([[float(r[0])] + list(r[1]) for r in rows], dtype=torch.float32)
    gtb, gtc = torch.zeros(B, G_CAP, 4), torch.zeros(B, G_CAP, dtype=torch.int32)
    gcnt = torch.zeros(B, dtype=torch.int32)
    for b, g in enumerate(gts):
        gcnt[b] = len(g)
        for i, (box, c) in enumerate(g):
            gtb[b, i], gtc[b, i] = torch.tensor(box, dtype=torch.float32), c
    return {"K": K, "pred": pred_matrix(scores, deltas.view(R, -1)), "rois": rois,
            "roi_cls": torch.tensor([r[2] for r in rows], dtype=torch.int32), "sizes": sizes, "gtb": gtb, "gtc": gtc, "gcnt": gcnt,
            "iou_thr": iou_thr, "B": B}


GT_BOX = (20.0, 20.0, 29.0, 29.0)                            # 10 x 10 in the legacy (+1) extents
FAR_BOX = (100.0, 100.0, 109.0, 109.0)


N_FILL = 4


def _fill(K):
    """per image a confident and an unsure true positive (the ground-truth box itself) and a confident and an unsure false
    positive (a box far away): all four sums of the loss are non-zero before the case's own rows"""
    hi = [LOGIT_LO] * (K + 1)
    hi[0] = LOGIT_HI
    lo = [0.0] * (K + 1)
    lo[0] = -1.0
    return [(b, box, 0, sc, None) for b in range(2) for box, sc in ((GT_BOX, hi), (GT_BOX, lo), (FAR_BOX, hi), (FAR_BOX, lo))]


BPC_NAMES = ["score-half", "iou-half", "iou-above-half", "tie", "no-gt-of-class", "background-row", "padding-rows"]


def bpc_case(name):
    gts = [[(GT_BOX, 0)], [(GT_BOX, 0)]]
    if name == "score-half":
        # K = 1, equal logits: expf(0) / (expf(0) + expf(0)) is exactly 0.5 -- two true positives and one false positive on
        # the `>=` side (AC / IC), beside the fillers
        K = 1
        rows = _fill(K) + [(0, GT_BOX, 0, [1.5, 1.5], None), (0, GT_BOX, 0, [-2.0, -2.0], None), (0, FAR_BOX, 0, [0.25, 0.25], None)]
        return _bpc_pack(K, rows, gts)
    K = 2
    conf = [LOGIT_HI, LOGIT_LO, LOGIT_LO]
    if name in ("iou-half", "iou-above-half"):
        # a 10 x 5 box on the 10 x 10 ground truth: 50 / (100 + 50 - 50) = 1/2, a false positive; one pixel row more: 60 / 100
        h = 4.0 if name == "iou-half" else 5.0
        rows = _fill(K) + [(0, (20.0, 20.0, 29.0, 20.0 + h), 0, conf, None)]
    elif name == "tie":
        # two ground-truth boxes of class 0, 10 x 15 each, around a 10 x 10 detection: 100 / 150 twice
        gts = [[(GT_BOX, 0), ((60.0, 60.0, 69.0, 74.0), 0), ((60.0, 55.0, 69.0, 69.0), 0)], [(GT_BOX, 0)]]
        rows = _fill(K) + [(0, (60.0, 60.0, 69.0, 69.0), 0, conf, None)]
    elif name == "no-gt-of-class":
        # class 1 has no ground truth in image 0: its confident detection on the class-0 box is a false positive
        rows = _fill(K) + [(0, GT_BOX, 1, [LOGIT_LO, LOGIT_HI, LOGIT_LO], None)]
    elif name == "background-row":
        # gt class K: decoded with class K - 1's deltas (a shift of half the 16-pixel box), then per class from THAT box --
        # class 0 lands on the ground truth at (48, 40) only if the clamp is made
        gts = [[(GT_BOX, 0), ((48.0, 40.0, 64.0, 56.0), 0)], [(GT_BOX, 0)]]
        rows = _fill(K) + [(0, (40.0, 40.0, 56.0, 56.0), K, conf, [[0, 0, 0, 0], [5.0, 0, 0, 0]])]
    elif name == "padding-rows":
        # rows of image -1 (padding) and of images >= B, confident and on the ground truth: ignored
        rows = _fill(K) + [(-1, GT_BOX, 0, conf, None), (2, FAR_BOX, 0, conf, None), (7, GT_BOX, 0, conf, None),
                           (-1, FAR_BOX, 1, [LOGIT_LO, LOGIT_HI, LOGIT_LO], None)]
    else:
        raise KeyError(name)
    return _bpc_pack(K, rows, gts)


MIX_K, MIX_ROWS = 3, (40, 60)


@functools.lru_cache(maxsize=None)
def bpc_mixed_case(seed=31):
    """K = 3, 100 rows = 300 threads: image 0's rows 0..39 (threads 0..119), image 1's 40..99.  Wavefront 0 holds image 0
    alone, wavefront 1 both images (the per-lane atomic path), wavefronts 2..4 image 1 alone (the reduction path); every
    seventh row is padding.  Integer boxes around four ground-truth boxes per image, zero deltas, random scores."""
    g = torch.Generator().manual_seed(seed)
    K = MIX_K
    rows, gts = [], []
    for b, n in enumerate(MIX_ROWS):
        xy = torch.stack([torch.randint(0, 200, (4,), generator=g), torch.randint(0, 120, (4,), generator=g)], 1)
        wh = torch.randint(20, 60, (4, 2), generator=g)
        gb = torch.cat([xy, xy + wh], 1).float()
        gc = torch.randint(0, K, (4,), generator=g)
        gts.append([(tuple(gb[i].tolist()), int(gc[i])) for i in range(4)])
        for j in range(n):
            src = gb[int(torch.randint(0, 4, (1,), generator=g))]
            box = (src + torch.randint(-6, 7, (4,), generator=g).float()).clamp(min=0)
            sc = (torch.randn(K + 1, generator=g) * 2.5).tolist()
            img = -1 if len(rows) % 7 == 3 else b
            rows.append((img, tuple(box.tolist()), int(torch.randint(0, K + 1, (1,), generator=g)), sc, None))
    return _bpc_pack(K, rows, gts)


def wave_images(case):
    """per 64-thread wavefront of k_bpc_sums (thread = row * K + class) the set of image indices of its live rows"""
    K, img = case["K"], case["rois"][:, 0]
    out = []
    for w in range((len(img) * K + 63) // 64):
        rows = sorted({t // K for t in range(64 * w, min(64 * w + 64, len(img) * K))})
        out.append({int(img[r]) for r in rows if 0 <= img[r] < case["B"]})
    return out


def bpc_definition(case, dtype=torch.float64):
    """om.predict_boxes_for_gt_classes -> OB.apply_deltas -> om.frcnn_inference_new_single -> om.bpc_loss, evaluated in ``dtype``
    -> (loss, detections per image, ground truth per image).  (OB.apply_deltas decodes in float32 whatever ``dtype`` is: the
    boxes of these cases are dyadic identities or translations, exact in either; the scores, IoUs and sums are in ``dtype``.)"""
    K = case["K"]
    cfg = om.Cfg(num_classes=K)
    pred, rois = case["pred"], case["rois"]
    inst, gts = [], []
    for b in range(case["B"]):
        r = torch.nonzero(rois[:, 0] == b).flatten()
        sc, dl = pred[r, :K + 1].to(dtype), pred[r, K + 1:5 * K + 1].to(dtype)
        nb = om.predict_boxes_for_gt_classes(dl, rois[r, 1:].to(dtype), case["roi_cls"][r].long(), cfg)
        bx = OB.apply_deltas(dl, nb, cfg.roi_bbox_weights)
        inst.append(om.frcnn_inference_new_single(bx, torch.softmax(sc, dim=-1), case["sizes"][b]))
        n = int(case["gcnt"][b])
        gts.append((case["gtb"][b, :n].to(dtype), case["gtc"][b, :n].long()))
    return om.bpc_loss(K, gts, inst, case["iou_thr"]), inst, gts


def legacy_iou(e, o):
    """the +1 IoU of bpc_loss.py between ground truth e [G, 4] and detections o [D, 4], float64 -> [G, D]"""
    e, o = e.double(), o.double()
    ea = (e[:, 2] - e[:, 0] + 1) * (e[:, 3] - e[:, 1] + 1)
    oa = (o[:, 2] - o[:, 0] + 1) * (o[:, 3] - o[:, 1] + 1)
    w = (torch.min(e[:, None, 2], o[None, :, 2]) - torch.max(e[:, None, 0], o[None, :, 0]) + 1).clamp(min=0)
    h = (torch.min(e[:, None, 3], o[None, :, 3]) - torch.max(e[:, None, 1], o[None, :, 1]) + 1).clamp(min=0)
    return w * h / (ea[:, None] + oa[None, :] - w * h)


def bpc_confusions(inst, gts, K, thr=0.5):
    """per image [(true-positive multiplicity, score, class, best IoU or None)] of every detection"""
    out = []
    for d, (gb, gc) in zip(inst, gts):
        rec = []
        for i in range(len(d["scores"])):
            c = int(d["classes"][i])
            m = gc == c
            if not m.any():
                rec.append((0, float(d["scores"][i]), c, None))
                continue
            iou = legacy_iou(gb[m], d["boxes"][i:i + 1])[:, 0]
            best = iou.max().item()
            rec.append((int((iou == best).sum()) if best > thr else 0, float(d["scores"][i]), c, best))
        out.append(rec)
    return out
