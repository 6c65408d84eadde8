"""Inputs of tests/test_gpu_detection_decisions.py: the kernels of csrc/sort.hip and csrc/detect.hip that make the detector's
discrete decisions (ranking, greedy NMS, the two matchers, the subsampler), at the edges where such a kernel goes wrong -- a
tie, a value exactly on a threshold, a list exactly at capacity, the first size past a path switch.

Everything here runs on the CPU from fixed seeds.  Expected outputs come from oracle/box_ops.py and torch.sort, never from the
library.  All box coordinates are integers or dyadic fractions, so every area, intersection and union is exact in fp32 and
every comparison with the oracle is decidable bit for bit.

Each generator checks that its input really sits on the edge it is named for and raises ``EdgeMissed`` otherwise (it never
skips); tests/test_detection_cases_host.py runs every generator without a GPU and records the measured counts.
"""
import functools

import numpy as np
import torch

from oracle import box_ops as OB


class EdgeMissed(AssertionError):
    """a generated input does not contain the edge it is named for"""


def require(cond, what):
    if not cond:
        raise EdgeMissed(what)


def f32(x):
    return np.float32(x)


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32)


# ================================================================================================================================
# NMS: lattice boxes
# ================================================================================================================================
SIZES = (5, 7, 9, 10, 14, 20, 28)      # 7x10 in 10x10: IoU 7/10; 9xk in 10xk: 9/10; 5xk in 10xk: 1/2
GUARD = f32(2.0 ** -20)                # the guard band of nms_row_half: |fma(-thr, union, inter)| <= 2^-20 * union


def lattice_boxes(n, seed, span=40, offset=0.0):
    """n boxes with integer corners in [0, span) and widths / heights from SIZES (``offset`` exists for the host file: a
    lattice shifted by 0.5 has no pair on a threshold)"""
    g = torch.Generator().manual_seed(seed)
    xy = torch.randint(0, span, (n, 2), generator=g)
    wh = torch.tensor(SIZES)[torch.randint(0, len(SIZES), (n, 2), generator=g)]
    b = torch.cat([xy, xy + wh], 1).float()
    b[:, 2:] += offset
    return b


def row_terms(b, i):
    """fp32 (inter, union) of box i against boxes i+1.., in the operation order of OB.nms and nms_row_half"""
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    zero = f32(0)
    w = np.maximum(zero, np.minimum(x2[i], x2[i + 1:]) - np.maximum(x1[i], x1[i + 1:]))
    h = np.maximum(zero, np.minimum(y2[i], y2[i + 1:]) - np.maximum(y1[i], y1[i + 1:]))
    inter = (w * h).astype(np.float32)
    area = ((x2 - x1) * (y2 - y1)).astype(np.float32)
    return inter, ((area[i] + area[i + 1:]) - inter).astype(np.float32)


def decide(inter, uni, thr, rule):
    """suppress decisions of one row.  "div": inter / union > thr in fp32, the definition.  "fma": the sign of
    fma(-thr, union, inter), the kernel's shortcut outside its guard band (computed in double, where a 24-bit by 11-bit
    product plus an integer is exact, then rounded once: the fused operation).  "ge": inter / union >= thr.  "band": inside
    the guard band."""
    thr32 = f32(thr)
    with np.errstate(divide="ignore", invalid="ignore"):
        if rule == "div":
            return inter / uni > thr32
        if rule == "ge":
            return inter / uni >= thr32
        r = (inter.astype(np.float64) - float(thr32) * uni.astype(np.float64)).astype(np.float32)
        if rule == "fma":
            return r > 0
        assert rule == "band"
        return ~(np.abs(r) > GUARD * np.abs(uni))


def greedy_nms(boxes, thr, rule, classes=None):
    """greedy NMS over boxes already in score order with ``rule`` as the pair test -> kept positions (for the preconditions
    only: the definition the GPU suite compares with is OB.nms / OB.batched_nms)"""
    b = np.asarray(boxes, dtype=np.float32)
    n = len(b)
    cl = None if classes is None else np.asarray(classes)
    removed = np.zeros(n, dtype=bool)
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(i)
        if i + 1 == n:
            break
        inter, uni = row_terms(b, i)
        sup = decide(inter, uni, thr, rule)
        if cl is not None:
            sup &= cl[i + 1:] == cl[i]
        removed[i + 1:] |= sup
    return keep


def pair_census(boxes, thr):
    """over all pairs i < j: how many the division and the shortcut decide differently, how many of those lie outside the
    guard band (must be none: there the kernel takes the shortcut), how many have IoU exactly thr's decimal value"""
    b = np.asarray(boxes, dtype=np.float32)
    out = {"pairs": 0, "disagree": 0, "disagree_outside_band": 0, "on_threshold": 0, "list": []}
    num, den = {0.5: (1, 2), 0.7: (7, 10), 0.9: (9, 10), 0.3: (3, 10), 0.6: (3, 5)}[thr]
    for i in range(len(b) - 1):
        inter, uni = row_terms(b, i)
        d = decide(inter, uni, thr, "div") != decide(inter, uni, thr, "fma")
        out["pairs"] += len(inter)
        out["disagree"] += int(d.sum())
        out["disagree_outside_band"] += int((d & ~decide(inter, uni, thr, "band")).sum())
        out["on_threshold"] += int((inter.astype(np.int64) * den == uni.astype(np.int64) * num).sum())
        out["list"] += [(i, i + 1 + int(j)) for j in np.nonzero(d)[0]]
    return out


POOL_N = 1500


@functools.lru_cache(maxsize=None)
def pool(seed):
    """the n = 1500 lattice set and its census at 0.7"""
    b = lattice_boxes(POOL_N, seed)
    return b, pair_census(b, 0.7)


def edge_subset(seed, n, from_end=False):
    """n boxes of pool(seed), chosen pair by pair from the pairs on which the shortcut errs, in the pool's (score) order"""
    b, cen = pool(seed)
    pairs = cen["list"][::-1] if from_end else cen["list"]
    chosen = []
    for i, j in pairs:
        for t in (i, j):
            if t not in chosen and len(chosen) < n:
                chosen.append(t)
    require(len(chosen) == n, f"edge_subset: only {len(chosen)} boxes lie on a disagreeing pair, {n} wanted")
    return b[sorted(chosen)]


def _stack(images, n):
    """images of unequal length -> [B, n, 4] (zero boxes past each live prefix) + the live counts"""
    out = torch.zeros(len(images), n, 4)
    for k, im in enumerate(images):
        out[k, : len(im)] = im
    return out, torch.tensor([len(im) for im in images], dtype=torch.int32)


def _alt(boxes, classes, npi):
    """torchvision's coordinate trick, in OB.batched_nms's own operations, over each image's live boxes"""
    alt = torch.zeros_like(boxes)
    for b in range(boxes.shape[0]):
        m = int(npi[b])
        bx = boxes[b, :m]
        off = classes[b, :m].to(bx) * (bx.max() + torch.tensor(1).to(bx))
        alt[b, :m] = bx + off[:, None]
    return alt


def nms_case(name, images, thr, max_keep=None, valid=None, classes=None, mode=None, n=None, rules=("fma",)):
    """one sfod_nms call.  ``rules``: the wrong pair tests the case must tell from the definition (each checked in
    nms_precondition)"""
    n = n or max(len(im) for im in images)
    boxes, npi = _stack(images, n)
    c = {"name": name, "boxes": boxes, "npi": npi, "thr": thr, "max_keep": max_keep or n, "valid": valid,
         "classes": classes, "mode": mode, "alt": None, "rules": rules}
    if mode is not None:
        c["alt"] = _alt(boxes, classes, npi)
    return c


def _live(case, b):
    m = int(case["npi"][b])
    live = torch.arange(m)
    if case["valid"] is not None:
        live = live[case["valid"][b, :m] != 0]
    return live


def nms_expected(case, b):
    """the definition: OB.nms, or OB.batched_nms in the strategy ``mode`` selects, on image b's live boxes"""
    live = _live(case, b)
    bx = case["boxes"][b][live]
    sc = torch.arange(len(live), 0, -1).float()
    if case["classes"] is None:
        keep = OB.nms(bx, sc, case["thr"])
    else:
        trick = case["mode"] is not None and int(case["mode"][b]) != 0
        keep = OB.batched_nms(bx, sc, case["classes"][b][live], case["thr"], numel_limit=10 ** 9 if trick else 0)
    return live[keep][: case["max_keep"]].tolist()


def nms_with_rule(case, b, rule):
    """the keep list a kernel with ``rule`` as its pair test would give"""
    live = _live(case, b)
    trick = case["mode"] is not None and int(case["mode"][b]) != 0
    bx = (case["alt"] if trick else case["boxes"])[b][live].numpy()
    cl = None if (case["classes"] is None or trick) else case["classes"][b][live].numpy()
    keep = greedy_nms(bx, case["thr"], rule, cl)
    return live[torch.tensor(keep, dtype=torch.int64)][: case["max_keep"]].tolist()


def nms_precondition(case):
    """the restated greedy pass with the division equals the definition; with each wrong rule it gives another list for at
    least one image -> the per-image (expected length, wrong-rule lengths)"""
    B = case["boxes"].shape[0]
    exp = [nms_expected(case, b) for b in range(B)]
    for b in range(B):
        require(nms_with_rule(case, b, "div") == exp[b], f"{case['name']}: the restated greedy pass is not the definition")
    stats = {"kept": [len(e) for e in exp]}
    for rule in case["rules"]:
        wrong = [nms_with_rule(case, b, rule) for b in range(B)]
        require(any(w != e for w, e in zip(wrong, exp)), f"{case['name']}: rule '{rule}' gives the definition's keep lists")
        stats[rule] = [len(w) for w in wrong]
    return stats


NMS_NAMES = ("edge-n64", "edge-n65", "edge-n128", "pool-n1500", "valid-npi", "max_keep-1", "max_keep-block-boundary",
             "progressive", "classes", "alt-mode10", "alt-mode01", "thr-0.5", "thr-0.9")
SEED_A, SEED_B = 18, 26           # of seeds 1..29 the two with the most pairs on which the shortcut errs (112, 113)


@functools.lru_cache(maxsize=None)
def nms_cases():
    a, cen_a = pool(SEED_A)
    b2, cen_b = pool(SEED_B)
    for cen in (cen_a, cen_b):
        require(cen["disagree"] >= 100, f"lattice: {cen['disagree']} pairs decide differently at 0.7, 100 wanted")
        require(cen["disagree_outside_band"] == 0, "lattice: a disagreeing pair lies outside the guard band")
    g = torch.Generator().manual_seed(5)
    cases = []
    # single tile, two tiles with one box in the second, two full tiles: every pair in them is one the shortcut errs on
    for n in (64, 65, 128):
        cases.append(nms_case(f"edge-n{n}", [edge_subset(SEED_A, n), edge_subset(SEED_B, n - 3, from_end=True)], 0.7))
    cases.append(nms_case("pool-n1500", [a, b2[:1437]], 0.7))
    # some boxes empty (valid == 0), the live prefix ending inside a 64-block (1000 = 15 * 64 + 40)
    valid = (torch.rand(2, POOL_N, generator=g) > 0.15).to(torch.uint8)
    cases.append(nms_case("valid-npi", [a, b2[:1000]], 0.7, valid=valid))
    cases.append(nms_case("max_keep-1", [a, b2[:1437]], 0.7, max_keep=1, rules=()))
    # the list fills with the last kept box of 64-block 2 (image 0); image 1 stops inside a block
    full = nms_expected(nms_case("tmp", [a], 0.7), 0)
    at_boundary = sum(1 for k in full if k < 192)
    require(full[at_boundary - 1] < 192 <= full[at_boundary], "max_keep at a block boundary")
    cases.append(nms_case("max_keep-block-boundary", [a, b2[:1437]], 0.7, max_keep=at_boundary))
    # progressive phases (max_keep 100: first phase 512 boxes, second all 1500): image 0 fills its list inside the first
    # phase; image 1 opens with 512 draws from 12 boxes, keeps fewer than 100 of them, and goes on into k_nms_mask_phase
    few = lattice_boxes(12, 99)
    dense = torch.cat([few[torch.randint(0, 12, (512,), generator=g)], b2[: POOL_N - 512 - 37]])
    c = nms_case("progressive", [a, dense], 0.7, max_keep=100)
    e0, e1 = nms_expected(c, 0), nms_expected(c, 1)
    require(len(e0) == 100 and e0[-1] < 512, "progressive: image 0 must fill its list in the first phase")
    require(sum(1 for k in e1 if k < 512) < 100 and len(e1) == 100, "progressive: image 1 must need the second phase")
    require(nms_with_rule(c, 1, "fma") != e1, "progressive: image 1's second phase must meet a pair the shortcut errs on")
    cases.append(c)
    # class-wise: the class-test template on raw boxes; then the teacher's two strategies (mode 1: alt_boxes, the coordinate
    # trick; mode 0: the class test), which on integer offsets must give one list
    cls = torch.randint(0, 4, (2, POOL_N), generator=g).to(torch.int32)
    cases.append(nms_case("classes", [a, b2[:1437]], 0.7, classes=cls))
    for m in ((1, 0), (0, 1)):
        cases.append(nms_case(f"alt-mode{m[0]}{m[1]}", [a, b2[:1437]], 0.7, classes=cls,
                              mode=torch.tensor(m, dtype=torch.int32)))
    # thresholds: 0.5 is exact in fp32 and a pair of IoU 1/2 is kept (strict >); 0.9f < 9/10 like 0.7f < 7/10
    for thr, rules in ((0.5, ("ge",)), (0.9, ("fma",))):
        cen = pair_census(a, thr)
        require(cen["on_threshold"] >= 10, f"lattice: {cen['on_threshold']} pairs of IoU exactly {thr}")
        require(cen["disagree_outside_band"] == 0, f"lattice at {thr}: a disagreeing pair lies outside the guard band")
        cases.append(nms_case(f"thr-{thr}", [a, b2[:1437]], thr, rules=rules))
    require(tuple(c["name"] for c in cases) == NMS_NAMES, "nms_cases: NMS_NAMES is out of date")
    return {c["name"]: c for c in cases}


def nms_wide_case():
    """n = 16 448 = 257 * 64: one column word more than the wide reduce holds, so k_nms_reduce (the narrow reduce) runs.
    Another lattice: corners in [0, 300), so that thousands of boxes are kept"""
    n = 16448
    big = lattice_boxes(n, 21, span=300)
    return nms_case("narrow-reduce-n16448", [big, lattice_boxes(4001, 22, span=300)], 0.7)


# ================================================================================================================================
# segmented sort
# ================================================================================================================================
NAN_BITS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0xFFFFFFFF)      # quiet / signalling, both signs


def sort_chunk(n):
    """the documented chunking: one workgroup up to 4096 keys, 4096-key chunks up to 131 072, 16 384-key chunks beyond"""
    return n if n <= 4096 else (4096 if n <= 131072 else 16384)


def sort_ws_bytes(B, n):
    """include/sfod_hip.h: two u64 key buffers of B x (n rounded up to whole chunks), 256-aligned, + 256"""
    if n <= 4096:
        return 256
    ch = sort_chunk(n)
    NP = (n + ch - 1) // ch * ch
    return (2 * B * NP * 8 + 255) // 256 * 256 + 256


def sort_case(n):
    """three segments: heavy ties; -1 markers, both zeros in both orders, both infinities; the same with NaNs of both signs
    in different chunks (first chunk, a middle one, the very last key)"""
    g = torch.Generator().manual_seed(n)
    keys = torch.randn(3, n, generator=g)
    keys[0] = torch.randint(0, 7, (n,), generator=g).float()
    keys[1, ::5] = -1.0
    if n > 16:
        for r in (1, 2):
            keys[r, 3], keys[r, 7] = 0.0, -0.0                  # +0 before -0 ...
            keys[r, n - 9], keys[r, n - 5] = -0.0, 0.0          # ... and -0 before +0: equal keys, the index decides
            keys[r, 5], keys[r, 9], keys[r, n // 2] = float("inf"), float("-inf"), float("inf")
    kb = keys.view(torch.int32)
    nan_at = [p for p in (1, n // 3, n // 2 + 1, n - 2, n - 1) if 0 <= p < n][-len(NAN_BITS):] if n > 16 else []
    for p, pattern in zip(nan_at, NAN_BITS):
        kb[2, p] = pattern - (1 << 32) if pattern >= 1 << 31 else pattern
    ch = sort_chunk(n)
    if n > 16:
        require(torch.isnan(keys[2]).sum() == len(nan_at), "sort: NaN patterns")
        require((kb[2] < 0)[torch.isnan(keys[2])].any() and (kb[2] >= 0)[torch.isnan(keys[2])].any(), "sort: NaNs of both signs")
        if n > ch:
            require(len({p // ch for p in nan_at}) >= 2, "sort: NaNs in different chunks")
    return keys


# ================================================================================================================================
# matchers
# ================================================================================================================================
# cell anchors S 20x20, T 16x20, W 40x20 on a stride-16 grid.  A ground truth inside T and S has a larger IoU with T, so an
# S anchor can sit exactly on a threshold without being any ground truth's best anchor (which would promote it to 1)
CELL = torch.tensor([[-10.0, -10, 10, 10], [-8, -10, 8, 10], [-20, -10, 20, 10]])
HF, WF, STRIDE = 9, 11, 16                 # 297 anchors: two workgroups
GCAP = 256                                 # == GT_MAX, the matchers' LDS table


def match_gt():
    """-> gt [4, 256, 4], classes [4, 256], counts (256, 0, 256, 3).  Image 0, all at anchor row 0 (y in [-10, 10]):
    the S anchor at x = 0 itself (IoU 1); 14x20 inside S and T at x = 32 (S: 280/400 = 7/10, T: 280/320);
    10x12 at x = 64 (S: 120/400 = 3/10, T: 120/320); the T anchor at x = 96, twice (an arg-max tie at IoU 1);
    10x20 at x = 128 (S: 1/2); 250 lattice boxes at y >= 40.  Image 2: one box that overlaps nothing among 255 lattice
    boxes -- d2's low-quality matching then promotes every anchor whose IoU with it is 0, which is every anchor"""
    g = torch.Generator().manual_seed(31)
    special = torch.tensor([[-10.0, -10, 10, 10], [24, -10, 38, 10], [56, -10, 66, 2], [88, -10, 104, 10],
                            [88, -10, 104, 10], [120, -10, 130, 10]])
    fill = lattice_boxes(GCAP - len(special), 32, span=90)     # y1 < 130: every one overlaps some anchor
    fill[:, [1, 3]] += 40
    perm = torch.randperm(GCAP, generator=g)                  # the specials anywhere in the table
    where = {name: int((perm == k).nonzero()[0, 0]) for k, name in enumerate(("eq", "t07", "t03", "dup_a", "dup_b", "t05"))}
    gt = torch.zeros(4, GCAP, 4)
    gt[0] = torch.cat([special, fill])[perm]
    gt[2] = lattice_boxes(GCAP, 33, span=90)
    gt[2, 200] = torch.tensor([5000.0, 5000, 5100, 5100])
    gt[3, :3] = torch.tensor([[20.0, 30, 48, 50], [20, 30, 48, 50], [100, 90, 120, 118]])
    cls = torch.randint(0, 8, (4, GCAP), generator=g).to(torch.int32)
    cls[0, where["dup_b"]] = (cls[0, where["dup_a"]] + 1) % 8  # the tie decides the class
    return gt, cls, torch.tensor([GCAP, 0, GCAP, 3], dtype=torch.int32), where


def match_rois():
    """[4, 300, 4] with live counts (300, 257, 300, 40): the S anchors of row 0 (IoU exactly 1, 7/10, 3/10, 1/2 with image 0's
    special ground truths), the duplicated ground truth itself, lattice boxes"""
    anchors = OB.grid_anchors(HF, WF, STRIDE, CELL)
    rois = torch.stack([lattice_boxes(300, 40 + b, span=130) for b in range(4)])
    rois[:, :, [1, 3]] += 20
    rois[0, 256:256 + WF] = anchors[0: WF * 3: 3]              # the S anchors of row 0, in the second workgroup
    rois[0, 299] = torch.tensor([88.0, -10, 104, 10])
    return rois, torch.tensor([300, 257, 300, 40], dtype=torch.int32)


def matcher_census(M, thresholds, low_quality):
    """columns of M [G, N] whose maximum is attained by more than one ground truth (with a positive maximum), and per
    threshold the columns whose maximum equals it bit for bit and that low-quality matching does not promote"""
    vals, _ = M.max(dim=0)
    ties = int((((M == vals[None]) & (vals[None] > 0)).sum(0) > 1).sum())
    promoted = torch.zeros(M.shape[1], dtype=torch.bool)
    if low_quality:
        best, _ = M.max(dim=1)
        promoted[torch.nonzero(M == best[:, None], as_tuple=True)[1]] = True
    on = {t: int(((vals.numpy().view(np.uint32) == bits(t)) & ~promoted.numpy()).sum()) for t in thresholds}
    return {"ties": ties, "on": on}


def matcher_preconditions():
    gt, cls, cnt, where = match_gt()
    anchors = OB.grid_anchors(HF, WF, STRIDE, CELL)
    ca = matcher_census(OB.pairwise_iou(gt[0], anchors), (0.3, 0.7), True)
    rois, rc = match_rois()
    cr = matcher_census(OB.pairwise_iou(gt[0], rois[0]), (0.3, 0.5, 0.7), False)
    for who, c, thrs in (("anchors", ca, (0.3, 0.7)), ("rois", cr, (0.3, 0.5, 0.7))):
        require(c["ties"] >= 1, f"matcher {who}: no arg-max tie")
        for t in thrs:
            require(c["on"][t] >= 1, f"matcher {who}: no best IoU equal to {t}f")
    far = OB.pairwise_iou(gt[2], anchors)
    require(int((far.max(dim=1)[0] == 0).sum()) == 1, "matcher anchors: image 2 wants one ground truth without overlap")
    _, lab = OB.matcher(far, [0.3, 0.7], [0, -1, 1], True)
    require(bool((lab == 1).all()), "matcher anchors: the all-zero row must promote every anchor")
    require(bool((gt[0, where["eq"]] == anchors).all(1).any()), "matcher anchors: no ground truth equal to an anchor")
    require(where and int(cnt[0]) == GCAP, "matcher: the table is not full")
    return {"anchors": ca, "rois": cr}


# ================================================================================================================================
# subsampling
# ================================================================================================================================
QUOTA_CASES = ((300, 0.21), (900, 0.13), (450, 0.26))          # int(num * frac) in double: 63, 117, 117; in fp32 one less
QUOTA_DEFAULTS = ((256, 0.5), (512, 0.25))


def quota_double(num, frac):
    return int(num * frac)


def quota_fp32(num, frac):
    return int(f32(num) * f32(frac))


def wrap_keys(keys):
    """uint32 values held in int64 -> the int32 bit patterns the wrappers pass"""
    return torch.where(keys >= 2 ** 31, keys - 2 ** 32, keys).to(torch.int32)


def subsample_expected(case, b):
    """OB.subsample_labels; mode 1 reads -2 (beyond the live prefix) and -1 (ignored) as never sampled"""
    lab = case["labels"][b].long()
    if case["mode"] == 1:
        lab = torch.where(lab == -2, torch.full_like(lab, -1), lab)
    return OB.subsample_labels(lab, case["num"], case["frac"], case["bg"], case["keys"][b])


def selected_bin(case, b, which):
    """(candidates, quota, candidates in the 12-bit histogram bin that holds the quota-th smallest (key, index), its rank
    inside that bin) of the positives (which 0) or negatives (1)"""
    lab = case["labels"][b].long()
    pos = (lab != -1) & (lab != -2) & (lab != case["bg"])
    cand = torch.nonzero(pos if which == 0 else lab == case["bg"]).squeeze(1)
    npos = min(int(pos.sum()), quota_double(case["num"], case["frac"]))
    take = npos if which == 0 else min(len(cand), case["num"] - npos)
    k = case["keys"][b][cand]
    order = torch.argsort(k, stable=True)             # cand ascends: the (key, index) order
    bin_ = int(k[order[take - 1]]) >> 20
    in_bin = (k >> 20) == bin_
    return len(cand), take, int(in_bin.sum()), take - int(((k >> 20) < bin_).sum())


def _keys(g, shape):
    """uniform uint32 keys, one in eight drawn from four values (ties that the index breaks), top bit set in about half"""
    k = torch.randint(0, 2 ** 32, shape, generator=g, dtype=torch.int64)
    few = torch.tensor([7, 2 ** 31, 2 ** 32 - 1, 0x80012345])[torch.randint(0, 4, shape, generator=g)]
    return torch.where(torch.rand(shape, generator=g) < 0.125, few, k)


def _sub(name, mode, labels, keys, num, frac, bg):
    require(int((keys >= 2 ** 31).sum()) > 0 or keys.numel() < 4, f"{name}: no key with the top bit set")
    return {"name": name, "mode": mode, "labels": labels, "keys": keys, "num": num, "frac": frac, "bg": bg}


def _labels(g, B, n, mode, K=8):
    """mode 0: int8 in {-1, 0, 1}; mode 1: int32 classes 0..K (K background) with -1 (ignored) sprinkled in"""
    if mode == 0:
        return torch.randint(-1, 2, (B, n), generator=g).to(torch.int8)
    lab = torch.randint(0, K + 1, (B, n), generator=g)
    lab[torch.rand(B, n, generator=g) < 0.5] = K
    lab[torch.rand(B, n, generator=g) < 0.1] = -1
    return lab.to(torch.int32)


def bin_case(mode, drop=0):
    """the histogram bin that holds the threshold has exactly SS_LIST = 1024 candidates (the list is full) and exactly 1025
    (the first count that falls back to the bitwise search); the threshold is the bin's last but one candidate, so that a
    list that lost any entry but the last ranks another one.  Bin 0x800: keys with the top bit set.
    Image 0: positives 1024, negatives 1025; image 1 the other way round.  ``drop`` (host file): one candidate fewer."""
    g = torch.Generator().manual_seed(70 + mode)
    n, num, frac, bg = 4096, 2200, 0.5, (0 if mode == 0 else 8)
    labels = torch.full((2, n), -1, dtype=torch.int64)
    keys = torch.randint(0x801 << 20, 2 ** 32, (2, n), generator=g, dtype=torch.int64)      # bins above 0x800
    for b, (mp, mn) in enumerate(((1024, 1025), (1025, 1024))):
        perm = torch.randperm(n, generator=g)
        at = 0
        for which, m in ((0, mp), (1, mn)):
            m -= drop if (b, which) == (0, 0) else 0
            below = 1100 - (m - 1)                      # quota 1100 = below + (m - 1): rank m - 1 inside the bin
            idx = perm[at: at + 1900]
            at += 1900
            labels[b, idx] = (1 if mode == 0 else 3) if which == 0 else bg
            keys[b, idx[:below]] = torch.randint(0, 0x800 << 20, (below,), generator=g, dtype=torch.int64)
            inbin = (0x800 << 20) + torch.randint(0, 1 << 20, (m,), generator=g, dtype=torch.int64)
            inbin[: m // 2] = (0x800 << 20) + 77       # half the bin on one key: the index decides
            keys[b, idx[below: below + m]] = inbin
    c = _sub(f"bin-1024-1025-mode{mode}", mode, labels.to(torch.int8 if mode == 0 else torch.int32), keys, num, frac, bg)
    want = {(0, 0): 1024, (0, 1): 1025, (1, 0): 1025, (1, 1): 1024}
    for (b, which), m in want.items():
        ncand, take, got, rank = selected_bin(c, b, which)
        require(take == 1100 and ncand == 1900, f"{c['name']}: quota {take} of {ncand}")
        require(got == m, f"{c['name']}: image {b} which {which}: the selected bin holds {got} candidates, {m} wanted")
        require(rank == m - 1, f"{c['name']}: rank {rank} inside the bin")
    return c


SUBSAMPLE_NAMES = tuple(["bin-1024-1025-mode0", "bin-1024-1025-mode1"] + [
    name.format(m=m) for m in (0, 1) for name in
    [f"n{n}-mode{{m}}" for n in (1, 63, 1024, 1025)] + ["exact-none-mode{m}"] +
    [f"quota-{num}-{frac}-mode{{m}}" for num, frac in QUOTA_CASES + QUOTA_DEFAULTS]])


@functools.lru_cache(maxsize=None)
def subsample_cases():
    cases = [bin_case(0), bin_case(1)]
    for mode in (0, 1):
        g = torch.Generator().manual_seed(80 + mode)
        bg = 0 if mode == 0 else 8
        fg = 1 if mode == 0 else 2
        # n = 1 (idx_bits 1), 63, a power of two, one past it (mode 1: one element per thread, then two)
        for n in (1, 63, 1024, 1025):
            lab = _labels(g, 3, n, mode)
            if n == 1:
                lab[0, 0], lab[1, 0], lab[2, 0] = fg, bg, -1
            cases.append(_sub(f"n{n}-mode{mode}", mode, lab, _keys(g, (3, n)), max(2, n // 8), 0.5, bg))
        # exactly as many candidates as the quota (no threshold search); no positives; no negatives
        n = 700
        lab = torch.full((3, n), -1, dtype=torch.int64)
        perm = torch.randperm(n, generator=g)
        lab[0, perm[:32]], lab[0, perm[32:64]] = fg, bg          # 32 + 32 of num 64
        lab[1, perm[:300]] = bg                                   # no positives: the negatives fill the sample
        lab[2, perm[:300]] = fg                                   # no negatives
        c = _sub(f"exact-none-mode{mode}", mode, lab.to(torch.int8 if mode == 0 else torch.int32), _keys(g, (3, n)), 64, 0.5, bg)
        require(selected_bin(c, 0, 0)[:2] == (32, 32) and selected_bin(c, 0, 1)[:2] == (32, 32), "subsample: exact quota")
        cases.append(c)
        # the quotas on which fp32 and double disagree, and the defaults; n no multiple of 1024, with a dead tail in mode 1
        for num, frac in QUOTA_CASES + QUOTA_DEFAULTS:
            n = 3000
            lab = _labels(g, 2, n, mode)
            if mode == 1:
                lab[:, 2950:] = -2
            lab[1, 1500:] = -1 if mode == 0 else -2
            c = _sub(f"quota-{num}-{frac}-mode{mode}", mode, lab, _keys(g, (2, n)), num, frac, bg)
            ncand, take, _, _ = selected_bin(c, 0, 0)
            require(ncand > take == quota_double(num, frac), f"{c['name']}: the quota does not bind")
            cases.append(c)
    require(tuple(c["name"] for c in cases) == SUBSAMPLE_NAMES, "subsample_cases: SUBSAMPLE_NAMES is out of date")
    return {c["name"]: c for c in cases}


def quota_preconditions():
    for num, frac in QUOTA_CASES:
        require(quota_double(num, frac) == quota_fp32(num, frac) + 1, f"quota ({num}, {frac}): fp32 and double agree")
    for num, frac in QUOTA_DEFAULTS:
        require(quota_double(num, frac) == quota_fp32(num, frac), f"quota default ({num}, {frac}): fp32 and double differ")
    return {(n, f): (quota_double(n, f), quota_fp32(n, f)) for n, f in QUOTA_CASES + QUOTA_DEFAULTS}


# ================================================================================================================================
# teacher post-processing: the NMS strategy switch
# ================================================================================================================================
def teacher_case():
    """the input of test_gpu_ops.py::test_teacher_postprocessing_matches_oracle (other seed) and, from the oracle's own
    operations, the number of candidates (score > 0.05) per image"""
    g = torch.Generator().manual_seed(13)
    B, P, K, ld = 2, 400, 8, 48
    pc = torch.tensor([400, 333], dtype=torch.int32)
    xy = torch.rand(B, P, 2, generator=g) * 900.0
    wh = torch.rand(B, P, 2, generator=g) * 250.0 + 1
    props = torch.cat([xy, xy + wh], 2)
    pred = torch.zeros(B * P, ld)
    pred[:, :9] = torch.randn(B * P, 9, generator=g) * 3
    pred[:, 9:41] = torch.randn(B * P, 32, generator=g) * 0.7
    sizes = [(600, 1200), (590, 1100)]
    cand = []
    for b in range(B):
        sc = torch.softmax(pred[b * P: b * P + int(pc[b]), :9], dim=-1)[:, :-1]
        require(float((sc / 0.05 - 1).abs().min()) > 1e-4, "teacher: a score so close to 0.05 that its side is not decidable")
        cand.append(int((sc > 0.05).sum()))
    require(cand[0] != cand[1] and min(cand) > 0, "teacher: candidate counts")
    return {"B": B, "P": P, "K": K, "pc": pc, "props": props, "pred": pred, "sizes": sizes, "cand": cand}
