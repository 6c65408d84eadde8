"""Built inputs of ``sfod_tta_merge`` + the merge chain (tests/test_gpu_tta.py), with the definition's answer
(tests/helpers/tta_definitions.py).  Everything runs on the CPU from fixed seeds; each generator checks that its input really
holds the edges it is named for and raises ``EdgeMissed`` otherwise (tests/test_tta_host.py runs them without a GPU).

``edges_case``: B = 2, A = 6, cap = 100, K = 8 on a dyadic geometry (a 64 x 128 test tensor of a 128 x 256 frame, sizes 32 /
64 / 128 with flip: every ratio is a power of two), so that the lattice boxes of tests/helpers/detection_cases.py keep pairs
whose IoU is exactly NMS_THRESH_TEST after the inverse transform.  ``ratios_case``: B = 3 on non-dyadic geometries (landscape,
portrait, identity ``pre``), where the order and the number of the float32 multiplications show in the bits.
"""
import numpy as np

from helpers import detection_cases as DC
from helpers import tta_definitions as D
from helpers.detection_cases import require

F32 = np.float32
NAN, INF = F32("nan"), F32("inf")
THR = F32(1e-8)
THR_NEXT = np.nextafter(THR, F32(1))
NMS_THRESH = 0.5


def _empty(B, A, cap, seed):
    """containers whose every slot is poison: NaN / +100 scores, far-away boxes, class 5 -- live rows are written over it"""
    g = np.random.RandomState(seed)
    boxes = (g.rand(B, A, cap, 4).astype(F32) * F32(1000) - F32(300))
    scores = np.where(g.rand(B, A, cap) < 0.5, NAN, F32(100)).astype(F32)
    classes = np.full((B, A, cap), 5, dtype=np.int32)
    return boxes, scores, classes, np.zeros((B, A), dtype=np.int32)


def _put(case, b, a, boxes, scores, classes):
    n = len(scores)
    case["det_boxes"][b, a, :n] = np.asarray(boxes, dtype=F32).reshape(n, 4)
    case["det_scores"][b, a, :n] = np.asarray(scores, dtype=F32)
    case["det_classes"][b, a, :n] = np.asarray(classes, dtype=np.int32)
    case["det_count"][b, a] = n


def _table(augs_per_image, geoms):
    """the table sfod_tta_merge reads, from the definition's own transform lists"""
    rows = []
    for augs, (h, w, H0, W0) in zip(augs_per_image, geoms):
        rows.append([[wa, ha, float(a["flip"]), F32(w * 1.0 / wa), F32(h * 1.0 / ha), F32(W0 * 1.0 / w), F32(H0 * 1.0 / h), 0.0]
                     for a in augs for (ha, wa) in [a["size"]]])
    return np.asarray(rows, dtype=F32)


def _case(name, geoms, min_sizes, max_size, flip, cap, K, topk, seed):
    augs = [D.augmentations(h, w, H0, W0, min_sizes, max_size, flip) for (h, w, H0, W0) in geoms]
    A = len(augs[0])
    boxes, scores, classes, count = _empty(len(geoms), A, cap, seed)
    return {"name": name, "geoms": geoms, "augs": augs, "B": len(geoms), "A": A, "cap": cap, "K": K, "topk": topk,
            "nms_thresh": NMS_THRESH, "det_boxes": boxes, "det_scores": scores, "det_classes": classes, "det_count": count,
            "table": _table(augs, geoms), "sizes": np.asarray([(g[2], g[3]) for g in geoms], dtype=np.int32)}


def passes_of(case, b):
    return [(case["det_boxes"][b, a, :n], case["det_scores"][b, a, :n], case["det_classes"][b, a, :n])
            for a in range(case["A"]) for n in [int(case["det_count"][b, a])]]


def expected(case, fault=None, topk=None):
    """the definition per image -> list of (boxes, scores, classes, number of candidates that passed the score test)"""
    return [D.tta_image(passes_of(case, b), case["augs"][b], (int(case["sizes"][b, 0]), int(case["sizes"][b, 1])), case["K"],
                        case["nms_thresh"], case["topk"] if topk is None else topk, fault=fault) for b in range(case["B"])]


def expected_candidates(case, b, fault=None):
    """what sfod_tta_merge writes for image b: boxes [A * cap, 4], scores [A * cap] (-1: a dead or dropped slot, box and
    class 0), classes [A * cap], the count of kept slots"""
    A, cap = case["A"], case["cap"]
    H0, W0 = (int(v) for v in case["sizes"][b])
    boxes, scores = np.zeros((A * cap, 4), F32), np.full(A * cap, F32(-1))
    classes = np.zeros(A * cap, np.int32)
    for a, (bx, sc, cl) in enumerate(passes_of(case, b)):
        inv = D.inverse_boxes(bx, case["augs"][b][a], fault)
        ok = np.isfinite(inv).all(axis=1) & np.isfinite(sc) & (cl >= 0) & (cl < case["K"])
        with np.errstate(invalid="ignore"):
            ok &= (sc >= THR) if fault == "ge" else (sc > THR)
        inv[:, 0::2] = np.clip(inv[:, 0::2], F32(0), F32(W0))
        inv[:, 1::2] = np.clip(inv[:, 1::2], F32(0), F32(H0))
        j = a * cap + np.nonzero(ok)[0]
        boxes[j], scores[j], classes[j] = inv[ok], sc[ok], cl[ok]
    return boxes, scores, classes, int((scores >= 0).sum())


def same(x, y):
    """bit equality of two ``expected`` lists (boxes and scores by their bits; classes and counts as integers)"""
    return len(x) == len(y) and all(
        p[0].shape == q[0].shape and (DC.bits(p[0]) == DC.bits(q[0])).all() and (DC.bits(p[1]) == DC.bits(q[1])).all()
        and (p[2] == q[2]).all() and p[3] == q[3] for p, q in zip(x, y))


def edges_case():
    c = _case("edges", [(64, 128, 128, 256), (64, 128, 128, 256)], (32, 64, 128), 4000, True, 100, 8, 100, seed=3)
    require([a["size"] for a in c["augs"][0]] == [(32, 64)] * 2 + [(64, 128)] * 2 + [(128, 256)] * 2, "edges: the sizes")
    # aug 0 (32 x 64, plain): 100 disjoint 2 x 2 boxes on a pitch of 4 -> 8 x 8 boxes on a pitch of 16 in the frame; classes
    # other than 3, so that every one survives the class-wise NMS; the lowest scores of the image, so that the top 100 hold the
    # edge rows and these fill the rest (the cut falls among them)
    ij = np.stack(np.meshgrid(np.arange(8), np.arange(16), indexing="ij"), -1).reshape(-1, 2)[:100]
    grid = np.stack([ij[:, 1] * 4 + 1, ij[:, 0] * 4 + 1, ij[:, 1] * 4 + 3, ij[:, 0] * 4 + 3], 1).astype(F32)
    _put(c, 0, 0, grid, F32(0.2) - np.arange(100, dtype=F32) * F32(0.001), [(0, 1, 2, 4, 5, 6, 7)[i % 7] for i in range(100)])
    # aug 1 (32 x 64, mirrored): the edge rows
    rows = [
        ((3, 3, 9, 9), THR, 1),                    # 0 score exactly 1e-8f: dropped (strict)
        ((3, 3, 9, 9), THR_NEXT, 1),               # 1 its successor: kept
        ((NAN, 2, 5, 6), 0.7, 2),                  # 2 NaN coordinate
        ((1, 2, 5, INF), 0.7, 2),                  # 3 infinite coordinate
        ((1, 2, 5, 6), NAN, 2),                    # 4 NaN score
        ((20, 4, 20, 12), 0.61, 6),                # 5 x1 == x2 under the flip
        ((-7, -3, 70, 40), 0.62, 7),               # 6 outside the augmented frame on every side: clipped to the whole frame
        ((90, 50, 99, 60), 0.63, 7),               # 7 wholly outside: clipped to the corner, width and height 0
        ((40, 8, 48, 16), 0.64, 1),                # 8 the same box and score as aug 3's row 0 (there: class 0)
    ]
    _put(c, 0, 1, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    # aug 2 (64 x 128, plain): nothing (det_count 0 over poisoned slots)
    # aug 3 (64 x 128, mirrored): the twin of row 8 -- both come back as (64, 32, 96, 64)
    _put(c, 0, 3, [(80, 16, 96, 32), (2.5, 3.25, 30.75, 20.5)], [0.64, 0.33], [0, 4])
    # aug 4 (128 x 256, plain; x 0.5 x 2 = the identity): 100 lattice boxes of one class in score order
    lat = DC.lattice_boxes(100, DC.SEED_A).numpy()
    _put(c, 0, 4, lat, F32(0.6) - np.arange(100, dtype=F32) * F32(0.002), [3] * 100)
    # aug 5 (128 x 256, mirrored): a few ordinary boxes
    g = np.random.RandomState(11)
    xy = g.randint(0, 100, (37, 2))
    wh = g.randint(4, 60, (37, 2))
    _put(c, 0, 5, np.concatenate([xy, xy + wh], 1), F32(0.3) + g.rand(37).astype(F32) * F32(0.1), g.randint(0, 8, 37))
    # image 1: every augmentation empty
    # ---- the edges are there ----
    s = c["det_scores"]
    require(DC.bits(s[0, 1, 0]) == DC.bits(THR) and DC.bits(s[0, 1, 1]) == DC.bits(THR) + 1, "edges: 1e-8f and its successor")
    require(np.isnan(c["det_boxes"][0, 1, 2]).any() and np.isinf(c["det_boxes"][0, 1, 3]).any() and np.isnan(s[0, 1, 4]),
            "edges: non-finite live rows")
    dead = np.arange(100)[None, None, :] >= c["det_count"][:, :, None]
    require(np.isnan(s[dead]).any() and (s[dead] == 100).any(), "edges: NaN and +100 scores in dead slots")
    require(c["det_count"][0, 2] == 0 and (c["det_count"][0] > 0).sum() == 5 and not c["det_count"][1].any(),
            "edges: an empty augmentation and an empty image")
    require(c["det_boxes"][0, 1, 5, 0] == c["det_boxes"][0, 1, 5, 2] and c["augs"][0][1]["flip"], "edges: x1 == x2 under flip")
    inv1 = D.inverse_boxes(c["det_boxes"][0, 1, :9], c["augs"][0][1])
    require(inv1[5, 0] == inv1[5, 2] and (inv1[6] < 0).any() and inv1[6, 2] > 256 and inv1[7, 2] < 0 and inv1[7, 1] > 128, "edges: outside the frame")
    inv3 = D.inverse_boxes(c["det_boxes"][0, 3, :1], c["augs"][0][3])
    require((DC.bits(inv1[8]) == DC.bits(inv3[0])).all() and s[0, 1, 8] == s[0, 3, 0], "edges: the same box twice, equal scores")
    lat_inv = D.inverse_boxes(lat, c["augs"][0][4])
    require((DC.bits(lat_inv) == DC.bits(lat)).all(), "edges: the lattice must come back bit for bit")
    require(DC.pair_census(lat, NMS_THRESH)["on_threshold"] > 0, "edges: no lattice pair with IoU exactly NMS_THRESH_TEST")
    full = expected(c, topk=-1)
    require(len(full[0][1]) >= 101 and len(expected(c)[0][1]) == 100, f"edges: {len(full[0][1])} survivors, 101 wanted")
    require(len(full[1][1]) == 0 and full[1][3] == 0, "edges: image 1 must stay empty")
    k = full[0][2].tolist()
    tie = [i for i in range(len(k)) if full[0][1][i] == F32(0.64)]
    require(len(tie) == 2 and tie[1] == tie[0] + 1 and [k[i] for i in tie] == [1, 0], "edges: the tie keeps the concatenation order")
    return c


def ratios_case():
    """non-dyadic geometries: landscape, portrait, and a frame whose ``pre`` is the identity; random fractional boxes"""
    c = _case("ratios", [(64, 107, 96, 160), (107, 64, 160, 96), (75, 50, 75, 50)], (48, 80), 120, True, 16, 8, 100, seed=4)
    g = np.random.RandomState(5)
    for b in range(c["B"]):
        for a, aug in enumerate(c["augs"][b]):
            ha, wa = aug["size"]
            n = (16, 9, 0, 13)[(a + b) % 4]
            xy = g.rand(n, 2) * [wa * 0.8, ha * 0.8]
            wh = g.rand(n, 2) * [wa * 0.5, ha * 0.5] + 1
            _put(c, b, a, np.concatenate([xy, xy + wh], 1), F32(0.05) + g.rand(n).astype(F32) * F32(0.9), g.randint(0, 8, n))
    c["det_scores"][1, 0, 3], c["det_scores"][1, 0, 4] = THR, THR_NEXT
    require([a["size"] for a in c["augs"][0]] == [(48, 80)] * 2 + [(72, 120)] * 2, "ratios: MAX_SIZE must clamp the second size")
    require([a["size"] for a in c["augs"][1]] == [(80, 48)] * 2 + [(120, 72)] * 2, "ratios: the portrait sizes")
    require(all(len(a["transforms"]) == (2 if a["flip"] else 1) for a in c["augs"][2]), "ratios: image 2 has no pre transform")
    return c


def cases():
    return [edges_case(), ratios_case()]
