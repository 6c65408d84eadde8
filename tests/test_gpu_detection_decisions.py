"""The kernels that make the detector's discrete decisions -- csrc/sort.hip (the ranking) and csrc/detect.hip (greedy NMS,
the anchor and ROI matchers, the subsampler, the teacher's NMS strategy switch) -- at their decision edges: ties, values
exactly on a threshold, lists exactly at capacity, the first size past each path switch.

Definitions: torch.sort(descending=True, stable=True) and oracle/box_ops.py (nms, batched_nms, pairwise_iou + matcher,
subsample_labels) on the CPU, never the library.  Inputs: tests/helpers/detection_cases.py, fixed seeds, integer or dyadic
box coordinates, so every comparison below is index-exact or bit-exact; tests/test_detection_cases_host.py holds every
generator to the edge it is named for.  The one exception is the teacher post-processing test, whose boxes and scores come
out of softmax and box decoding and are compared as tests/test_gpu_ops.py compares them; its counts, classes and strategy
flags are exact.

kernel                                   definition                          cases
sfod_segmented_sort_desc                 torch.sort stable descending        n = 1, 2, 4096 | 4097 (one workgroup | two chunks,
                                                                             one key in the second), 131072 | 131073 (4096- |
                                                                             16384-key chunks), 200000; ties, +-0, +-inf, NaNs
sfod_nms                                 OB.nms / OB.batched_nms             lattice boxes with pairs of IoU exactly 7/10, 1/2,
                                                                             9/10; n = 64, 65, 128, 1500, 16448; valid,
                                                                             n_per_image, max_keep, phases, classes, alt + mode
native.frcnn_inference                   om.fast_rcnn_inference              numel_limit = 4c and 4c - 1
sfod_anchor_match[_opt]                  OB.pairwise_iou + OB.matcher        full table (256), none, duplicates, IoU 1, 3/10,
sfod_roi_match[_opt]                                                         7/10, 1/2, a ground truth that overlaps nothing
sfod_subsample_quota (both modes)        OB.subsample_labels                 bin of 1024 | 1025, keys >= 2^31, n = 1, 63, 1024,
                                                                             1025, exact quota, no positives / negatives,
                                                                             quotas where fp32 and double differ
sfod_subsample (the fraction as a float) OB.subsample_labels at its fp32     (300, 0.21) -> 62 and (256, 0.5) -> 128
                                         quota
"""
import pytest
import torch

from helpers import detection_cases as dc
from oracle import box_ops as OB
from oracle import model as om

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(t):
    return None if t is None else t.to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- segmented sort --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 4096, 4097, 131072, 131073, 200000])
def test_segmented_sort_at_its_path_switches_with_nans(native, n):
    """order and values (bit patterns: NaN payloads and the zeros' signs travel with the index) of torch.sort; the workspace
    query pins which chunking served n: 131072 is the last size on 4096-key chunks, 131073 the first on 16384-key ones
    (9 chunks, 200000: 13, so a run without a partner exists at more than one merge level)"""
    keys = dc.sort_case(n)
    assert native.query("sfod_sort_ws_bytes", 3, n) == dc.sort_ws_bytes(3, n)
    ss, si = native.segmented_sort_desc(keys.to(DEV))
    ref_v, ref_i = torch.sort(keys, dim=1, descending=True, stable=True)
    assert torch.equal(si.cpu().long(), ref_i)
    assert torch.equal(_bits(ss.cpu()), _bits(ref_v))


# ---- NMS -------------------------------------------------------------------------------------------------------------------------
def _run_nms(native, case):
    return native.nms(case["boxes"].to(DEV), case["thr"], case["max_keep"], valid=_dev(case["valid"]),
                      n_per_image=_dev(case["npi"]), alt_boxes=_dev(case["alt"]), classes=_dev(case["classes"]),
                      mode=_dev(case["mode"]))


def _check_nms(native, case):
    keep_idx, keep_cnt = _run_nms(native, case)
    got = []
    for b in range(case["boxes"].shape[0]):
        ref = dc.nms_expected(case, b)
        c = keep_cnt[b].item()
        got.append(keep_idx[b, :c].cpu().long().tolist())
        assert c == len(ref), (case["name"], b, c, len(ref))
        assert got[b] == ref, (case["name"], b)
    return got


@pytest.mark.parametrize("name", dc.NMS_NAMES)
def test_nms_on_lattice_boxes_with_pairs_exactly_on_the_threshold(native, name):
    _check_nms(native, dc.nms_cases()[name])


def test_nms_narrow_reduce_on_lattice_boxes(native):
    """n = 16448: 257 column words, the single-wave reduce k_nms_reduce"""
    _check_nms(native, dc.nms_wide_case())


def test_nms_strategies_agree_on_integer_offsets(native):
    """the coordinate trick (alt_boxes, mode 1) and the class test (mode 0, and classes without mode) give one list: the
    offsets are integers, so the shifted boxes have the same intersections and unions"""
    cases = dc.nms_cases()
    lists = [_check_nms(native, cases[k]) for k in ("classes", "alt-mode10", "alt-mode01")]
    assert lists[0] == lists[1] == lists[2]


# ---- teacher post-processing: the strategy switch ---------------------------------------------------------------------------------
@pytest.mark.parametrize("image,delta", [(0, 0), (0, -1), (1, 0), (1, -1)])
def test_teacher_nms_strategy_switches_exactly_at_four_times_the_candidates(native, image, delta):
    """torchvision takes the per-class loop when boxes.numel() = 4c > numel_limit: with the limit at 4c the image with c
    candidates still takes the coordinate trick, at 4c - 1 the loop"""
    t = dc.teacher_case()
    B, P, K = t["B"], t["P"], t["K"]
    limit = 4 * t["cand"][image] + delta
    cfg = om.Cfg(nms_numel_limit=limit)
    scores = torch.cat([t["pred"][b * P: b * P + t["pc"][b], :9] for b in range(B)])
    deltas = torch.cat([t["pred"][b * P: b * P + t["pc"][b], 9:41] for b in range(B)])
    ref = om.fast_rcnn_inference(scores, deltas, [t["props"][b, : t["pc"][b]] for b in range(B)], t["sizes"], cfg)
    out = native.frcnn_inference(t["pred"].to(DEV), K, t["props"].to(DEV), t["pc"].to(DEV),
                                 torch.tensor(t["sizes"], dtype=torch.int32, device=DEV), 0.05, 0.5, 100, 0.8,
                                 numel_limit=limit)
    assert out["cand_count"].tolist() == t["cand"]
    assert out["mode"].tolist() == [0 if 4 * c > limit else 1 for c in t["cand"]]
    assert out["mode"][image].item() == (1 if delta == 0 else 0)
    for b in range(B):
        n = out["det_count"][b].item()
        assert n == len(ref[b]["scores"])
        assert out["det_classes"][b, :n].cpu().long().tolist() == ref[b]["classes"].tolist()
        torch.testing.assert_close(out["det_scores"][b, :n].cpu(), ref[b]["scores"], rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(out["det_boxes"][b, :n].cpu(), ref[b]["boxes"], rtol=1e-5, atol=2e-3)
        pl = om.threshold_bbox(ref[b], 0.8)
        m = out["gt_count"][b].item()
        assert m == len(pl["gt_classes"])
        assert out["gt_classes"][b, :m].cpu().long().tolist() == pl["gt_classes"].tolist()
        torch.testing.assert_close(out["gt_boxes"][b, :m].cpu(), pl["gt_boxes"], rtol=1e-5, atol=2e-3)


# ---- matchers --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("general", [False, True], ids=["sfod_anchor_match", "sfod_anchor_match_opt"])
def test_anchor_match_on_full_tables_ties_and_thresholds(native, general):
    """G = Gcap = 256 | 0 | 256 with one ground truth that overlaps nothing | 3; labels and matched indices of
    OB.matcher([0.3, 0.7], [0, -1, 1], low quality on).  The general entry point with a boundary so wide that it relabels
    nothing."""
    gt, _, cnt, _ = dc.match_gt()
    B = gt.shape[0]
    anchors = OB.grid_anchors(dc.HF, dc.WF, dc.STRIDE, dc.CELL)
    kw = {}
    if general:
        kw = {"boundary_thresh": 4096.0, "sizes": torch.tensor([[144, 176]] * B, dtype=torch.int32, device=DEV)}
    matched, labels = native.anchor_match(dc.CELL.to(DEV), B, dc.HF, dc.WF, dc.STRIDE, gt.to(DEV), cnt.to(DEV), 0.3, 0.7, **kw)
    for b in range(B):
        M = OB.pairwise_iou(gt[b, : cnt[b]], anchors)
        ridx, rlab = OB.matcher(M, [0.3, 0.7], [0, -1, 1], True)
        assert torch.equal(labels[b].cpu(), rlab), b
        assert torch.equal(matched[b].cpu().long(), ridx), b


@pytest.mark.parametrize("lo,hi", [(None, 0.5), (0.3, 0.7)], ids=["sfod_roi_match-0.5", "sfod_roi_match_opt-0.3-0.7"])
def test_roi_match_on_full_tables_ties_and_thresholds(native, lo, hi):
    """ROIs whose best IoU is exactly 1/2 (foreground: >=), 3/10 (ignored: the band's closed lower end), 7/10 (foreground:
    its open upper end) and an arg-max tie between two ground truths of different classes"""
    gt, gcl, cnt, _ = dc.match_gt()
    rois, rc = dc.match_rois()
    B, P, K = rois.shape[0], rois.shape[1], 8
    matched, cls = native.roi_match(rois.to(DEV), rc.to(DEV), gt.to(DEV), gcl.to(DEV), cnt.to(DEV), hi, K, lo=lo)
    for b in range(B):
        m, G = int(rc[b]), int(cnt[b])
        want_cls = torch.full((P,), -2, dtype=torch.int64)
        want_idx = torch.zeros(P, dtype=torch.int64)
        M = OB.pairwise_iou(gt[b, :G], rois[b, :m])
        if lo is None:
            ridx, rlab = OB.matcher(M, [hi], [0, 1], False)
        else:
            ridx, rlab = OB.matcher(M, [lo, hi], [0, -1, 1], False)
        fg = gcl[b, :G].long()[ridx] if G else torch.full((m,), K, dtype=torch.int64)
        want_cls[:m] = torch.where(rlab == 1, fg, torch.where(rlab == -1, torch.tensor(-1), torch.tensor(K)))
        want_idx[:m] = ridx
        assert torch.equal(cls[b].cpu().long(), want_cls), b
        assert torch.equal(matched[b].cpu().long(), want_idx), b


# ---- subsampling -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.SUBSAMPLE_NAMES)
def test_subsample_at_its_capacity_tie_and_quota_edges(native, name):
    case = dc.subsample_cases()[name]
    lab, keys = case["labels"], dc.wrap_keys(case["keys"]).to(DEV)
    B, n = lab.shape
    if case["mode"] == 0:
        assert case["bg"] == 0
        ld = lab.clone().to(DEV)
        _, counts = native.subsample_rpn_(ld, keys, case["num"], case["frac"])
        for b in range(B):
            pos, neg = dc.subsample_expected(case, b)
            ref = torch.full((n,), -1, dtype=torch.int8)
            ref[pos] = 1
            ref[neg] = 0
            assert counts[b].tolist() == [len(pos), len(neg)], b
            assert torch.equal(ld[b].cpu(), ref), b
    else:
        idx, cnt = native.subsample_roi(lab.to(DEV), keys, case["num"], case["frac"], case["bg"])
        for b in range(B):
            fg, bg = dc.subsample_expected(case, b)
            ref = torch.cat([fg, bg]).tolist()
            assert cnt[b].item() == len(ref), b
            assert idx[b, : len(ref)].cpu().long().tolist() == ref, b


@pytest.mark.parametrize("mode", [0, 1])
def test_fraction_entry_point_keeps_its_fp32_product(native, mode):
    """sfod_subsample, the entry point that takes the fraction as a float, stays what it was: the quota is the fp32 product,
    62 for 300 x 0.21 (the definition at a fraction of 62.5 / 300), and the defaults' 128"""
    for num, frac, quota in ((300, 0.21, 62), (256, 0.5, 128)):
        case = dict(dc.subsample_cases()[f"quota-{num}-{frac}-mode{mode}"])
        assert dc.quota_fp32(num, frac) == quota
        lab, keys = case["labels"], dc.wrap_keys(case["keys"]).to(DEV)
        B, n = lab.shape
        case["frac"] = (quota + 0.5) / num
        ld = lab.clone().to(DEV)
        idx = torch.zeros(B, num, dtype=torch.int32, device=DEV)
        cnt = torch.zeros(B, 2, dtype=torch.int32, device=DEV)
        native.call("sfod_subsample", ld, keys, B, n, num, frac, case["bg"], mode, idx if mode else None, cnt)
        for b in range(B):
            pos, neg = dc.subsample_expected(case, b)
            if mode == 0:
                ref = torch.full((n,), -1, dtype=torch.int8)
                ref[pos] = 1
                ref[neg] = 0
                assert cnt[b].tolist() == [len(pos), len(neg)], b
                assert torch.equal(ld[b].cpu(), ref), b
            else:
                ref = torch.cat([pos, neg]).tolist()
                assert cnt.view(-1)[b].item() == len(ref), b
                assert idx[b, : len(ref)].cpu().long().tolist() == ref, b
