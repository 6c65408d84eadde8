"""CPU tests of tests/helpers/detection_cases.py: every input of tests/test_gpu_detection_decisions.py really contains the edge
it is named for.  A GPU test on an input that misses its edge passes whatever the kernel does there, so each generator checks
its own precondition and raises ``EdgeMissed``; this file runs every generator, asserts the counts the suite relies on, plants
two misses (a lattice shifted by 0.5, one candidate dropped from the 1024 bin) and holds the library's host-side answers
(the sort's workspace query, the quota the wrappers pass) to their definitions.  The measured counts are printed (-s) and
recorded in profiles/detection_decisions.txt.
"""
import numpy as np
import pytest
import torch

from helpers import detection_cases as dc
from oracle import box_ops as OB


# ---- NMS -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [dc.SEED_A, dc.SEED_B])
def test_lattice_has_a_hundred_pairs_on_which_the_shortcut_errs_all_inside_the_guard_band(seed):
    boxes, cen = dc.pool(seed)
    print(f"lattice seed {seed}: {cen['pairs']} pairs, {cen['disagree']} decided differently by inter / union > 0.7f and by "
          f"the sign of fma(-0.7f, union, inter), {cen['disagree_outside_band']} of them outside the guard band, "
          f"{cen['on_threshold']} pairs of IoU exactly 7/10")
    assert cen["disagree"] >= 100
    assert cen["disagree_outside_band"] == 0
    assert cen["on_threshold"] == cen["disagree"]           # exactly the pairs of IoU 7/10: 0.7f < 7/10
    b = boxes.numpy()
    assert (b == np.round(b)).all() and b.min() >= 0 and b.max() < 40 + max(dc.SIZES)
    # the keep list with the shortcut's decisions is another one than the definition's
    sc = torch.arange(len(boxes), 0, -1).float()
    ref = OB.nms(boxes, sc, 0.7).tolist()
    short = dc.greedy_nms(b, 0.7, "fma")
    print(f"lattice seed {seed}: OB.nms keeps {len(ref)} boxes, the shortcut alone {len(short)}")
    assert dc.greedy_nms(b, 0.7, "div") == ref
    assert short != ref


def test_the_other_thresholds_agree_except_where_the_fp32_threshold_lies_below_its_decimal():
    """0.5, 0.3f and 0.6f are not below their decimal values (0.5 is exact, the other two round up): the division and the
    shortcut agree on every pair.  0.7f and 0.9f round down: they differ exactly on the pairs of IoU 7/10 and 9/10."""
    boxes, _ = dc.pool(dc.SEED_A)
    for thr, differ in ((0.5, False), (0.3, False), (0.6, False), (0.9, True)):
        cen = dc.pair_census(boxes, thr)
        print(f"thr {thr}: {cen['on_threshold']} pairs exactly on it, {cen['disagree']} decided differently")
        assert cen["disagree_outside_band"] == 0
        assert cen["disagree"] == (cen["on_threshold"] if differ else 0)
        assert cen["on_threshold"] >= (10 if thr in (0.5, 0.9) else 1)          # 0.5 and 0.9 are run on the GPU


def test_a_lattice_shifted_by_half_a_pixel_misses_the_edge():
    cen = dc.pair_census(dc.lattice_boxes(dc.POOL_N, dc.SEED_A, offset=0.5), 0.7)
    assert cen["disagree"] < 100


@pytest.mark.parametrize("name", dc.NMS_NAMES)
def test_every_nms_case_tells_the_wrong_pair_test_from_the_definition(name):
    case = dc.nms_cases()[name]
    stats = dc.nms_precondition(case)
    print(f"{name}: n = {case['boxes'].shape[1]}, live {case['npi'].tolist()}, max_keep {case['max_keep']}: {stats}")
    assert len(set(case["npi"].tolist())) > 1                        # unequal live counts
    if name.startswith("edge-"):
        assert case["boxes"].shape[1] == int(name[6:])
    if name == "valid-npi":
        assert int(case["npi"][1]) % 64 != 0 and (case["valid"] == 0).any()
    if name == "progressive":
        assert 2 * case["max_keep"] + 96 <= 512 and 512 * 5 // 4 < case["boxes"].shape[1]      # phases: 512 boxes, then all
    if case["alt"] is not None:
        live = int(case["npi"][0])
        assert (case["alt"][0, :live] == case["alt"][0, :live].round()).all()                  # integer offsets


def test_the_narrow_reduce_case_has_257_column_words():
    case = dc.nms_wide_case()
    assert (case["boxes"].shape[1] + 63) // 64 == 257
    print("narrow reduce:", dc.nms_precondition(case))


# ---- segmented sort --------------------------------------------------------------------------------------------------------------
def test_sort_cases_hold_both_zeros_both_infinities_and_nans_of_both_signs_in_different_chunks():
    for n in (4096, 4097, 131072, 131073, 200000):
        keys = dc.sort_case(n)                                       # raises if the NaNs are missing or share a chunk
        kb = keys.view(torch.int32)
        assert (kb[2] == -(1 << 31)).any() and (keys[2] == float("inf")).any() and (keys[2] == float("-inf")).any()
        neg0 = torch.nonzero(kb[2] == -(1 << 31)).squeeze(1)
        pos0 = torch.nonzero(kb[2] == 0).squeeze(1)
        assert neg0.min() < pos0.max() and pos0.min() < neg0.max()   # each zero once ahead of the other
    assert torch.isnan(dc.sort_case(4097)[2, 4096])                  # the second chunk's only key is a NaN
    assert dc.sort_chunk(131072) == 4096 and dc.sort_chunk(131073) == 16384
    assert [-(-n // 16384) for n in (131073, 200000)] == [9, 13]


def test_sort_workspace_query_follows_the_documented_chunking(sfod):
    lib = sfod.native.load()
    for n in (1, 4096, 4097, 16384, 131072, 131073, 200000):
        assert lib.sfod_sort_ws_bytes(3, n) == dc.sort_ws_bytes(3, n), n


# ---- matchers --------------------------------------------------------------------------------------------------------------------
def test_matcher_sets_hold_a_tie_and_best_ious_equal_to_each_threshold_bit_for_bit():
    stats = dc.matcher_preconditions()
    print("matcher sets:", stats)
    gt, cls, cnt, where = dc.match_gt()
    assert cnt.tolist() == [dc.GCAP, 0, dc.GCAP, 3] and dc.GCAP == 256
    assert torch.equal(gt[0, where["dup_a"]], gt[0, where["dup_b"]]) and cls[0, where["dup_a"]] != cls[0, where["dup_b"]]
    rois, rc = dc.match_rois()
    assert rois.shape[1] > 256 and len(set(rc.tolist())) > 1         # two workgroups, unequal live counts
    for t in (0.3, 0.5, 0.7):                                        # the quotients the generators rely on
        num = {0.3: 3, 0.5: 5, 0.7: 7}[t]
        assert dc.bits(np.float32(num) / np.float32(10)) == dc.bits(t)


# ---- subsampling -----------------------------------------------------------------------------------------------------------------
def test_bin_cases_fill_the_histogram_bin_to_1024_and_1025():
    for mode in (0, 1):
        case = dc.bin_case(mode)
        got = {(b, w): dc.selected_bin(case, b, w) for b in (0, 1) for w in (0, 1)}
        print(f"{case['name']}: (candidates, quota, in the selected bin, rank in it) = {got}")
        assert sorted(v[2] for v in got.values()) == [1024, 1024, 1025, 1025]
        assert int((case["keys"] >= 2 ** 31).sum()) > 1000


def test_dropping_one_candidate_from_the_1024_bin_is_noticed():
    with pytest.raises(dc.EdgeMissed, match="1023 candidates, 1024 wanted"):
        dc.bin_case(0, drop=1)


def test_subsample_cases_cover_their_edges():
    cases = dc.subsample_cases()
    assert tuple(cases) == dc.SUBSAMPLE_NAMES
    for name, c in cases.items():
        B, n = c["labels"].shape
        assert c["keys"].min() >= 0 and c["keys"].max() < 2 ** 32
        if n >= 63:
            assert int((c["keys"] >= 2 ** 31).sum()) > 0, name
        w = dc.wrap_keys(c["keys"])
        assert torch.equal(w.to(torch.int64) % (1 << 32), c["keys"])     # the int32 bit patterns are the uint32 keys
    assert {c["labels"].shape[1] for c in cases.values()} >= {1, 63, 1024, 1025}
    ex = cases["exact-none-mode1"]
    assert [len(x) for x in dc.subsample_expected(ex, 1)] == [0, 64]     # no positives: the negatives fill the sample
    assert [len(x) for x in dc.subsample_expected(ex, 2)] == [32, 0]     # no negatives


def test_quota_cases_differ_between_fp32_and_double_and_the_wrapper_passes_the_double_one(sfod):
    stats = dc.quota_preconditions()
    print("quota (double, fp32):", stats)
    assert stats[(300, 0.21)] == (63, 62) and stats[(900, 0.13)] == (117, 116) and stats[(450, 0.26)] == (117, 116)
    assert stats[(256, 0.5)] == (128, 128) and stats[(512, 0.25)] == (128, 128)
    for num, frac in dc.QUOTA_CASES + dc.QUOTA_DEFAULTS:
        assert sfod.native.positive_quota(num, frac) == int(num * frac)
    differ = sum(int(num * (k / 100)) != dc.quota_fp32(num, k / 100) for num in range(1, 2049) for k in range(101))
    print(f"quota: {differ} (num <= 2048, fraction k / 100) pairs differ between double and fp32")
    assert differ > 0
    with pytest.raises(ValueError, match="POSITIVE_FRACTION"):
        sfod.native.positive_quota(256, 1.5)


def test_subsample_entry_points_refuse_a_quota_outside_the_sample(sfod):
    """host-side argument checks, before any launch: the count form refuses pos_quota > num, the fraction form a fraction
    outside [0, 1] or NaN (whose conversion to int is undefined)"""
    lib = sfod.native.load()
    EBADARG = -1000
    assert lib.sfod_subsample_quota(None, None, 1, 8, 4, 5, 0, 0, None, None, None) == EBADARG
    assert lib.sfod_last_error() == b"bad argument: subsample: the positive quota exceeds num"
    assert lib.sfod_subsample_quota(None, None, 1, 8, 4, -1, 0, 0, None, None, None) == EBADARG
    for frac in (1.5, -0.25, float("nan"), float("inf")):
        assert lib.sfod_subsample(None, None, 1, 8, 4, frac, 0, 0, None, None, None) == EBADARG
        assert lib.sfod_last_error() == b"bad argument: subsample: pos_frac must be in [0, 1]"


def test_oracle_subsample_orders_keys_as_uint32():
    """keys >= 2^31, given as uint32 values or as int32 bit patterns, rank above every key below 2^31"""
    labels = torch.tensor([1, 1, 1, 0, 0, 0])
    keys = torch.tensor([2 ** 32 - 1, 5, 2 ** 31, 2 ** 31 + 1, 2 ** 31 - 1, 7], dtype=torch.int64)
    for k in (keys, dc.wrap_keys(keys)):
        pos, neg = OB.subsample_labels(labels, 4, 0.5, 0, k)
        assert pos.tolist() == [1, 2] and neg.tolist() == [4, 5]


# ---- teacher ---------------------------------------------------------------------------------------------------------------------
def test_teacher_case_counts_its_candidates():
    t = dc.teacher_case()
    print("teacher candidates per image:", t["cand"])
    assert t["cand"][0] != t["cand"][1]                  # a limit on one image's switch is off the other's
    for c in t["cand"]:
        assert 0 < c < t["P"] * t["K"]
