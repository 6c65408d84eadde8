"""CPU tests of ``TEST.AUG``: the config keys and their validation (modeling/tta_options.py), the plan builder against
hand-computed cases, the numpy restatement of Detectron2's rule (tests/helpers/tta_definitions.py) against second
formulations, the built inputs of the GPU suite (tests/helpers/tta_cases.py: every generator checks its own edges), planted
faults that those inputs must tell from the definition, and the argument refusals of ``sfod_tta_merge`` (the library loads
without a GPU; a refused call never reaches a launch)."""
import os

import numpy as np
import pytest
import torch

from helpers import tta_cases as C
from helpers import tta_definitions as D

F32 = np.float32
SFOD_EBADARG = -1000
D2_SIZES = (400, 500, 600, 700, 800, 900, 1000, 1100, 1200)


def _cfg(sfod, **aug):
    cfg = sfod.config.setup_cfg(None, [])
    cfg.defrost()
    for k, v in aug.items():
        setattr(cfg.TEST.AUG, k, v)
    return cfg


# ---- config ------------------------------------------------------------------------------------------------------------------
def test_config_defaults_are_detectron2s(sfod):
    aug = sfod.config.setup_cfg(None, []).TEST.AUG
    assert dict(aug) == {"ENABLED": False, "MIN_SIZES": D2_SIZES, "MAX_SIZE": 4000, "FLIP": True}
    opt = sfod.modeling.tta_options.TTAOptions(sfod.config.setup_cfg(None, []))          # d2's defaults run: 18 x 100
    assert (opt.min_sizes, opt.max_size, opt.flip, opt.num_aug, opt.max_det) == (D2_SIZES, 4000, True, 18, 100)
    assert sfod.modeling.tta_options.MERGE_CAPACITY >= 18 * 100
    assert (sfod.modeling.tta_options.MERGE_CAPACITY, sfod.modeling.tta_options.MAX_AUGMENTATIONS,
            sfod.modeling.tta_options.TABLE_ROW) == (sfod.native.TTA_MAX_CAND, sfod.native.TTA_MAX_AUG, sfod.native.TTA_ROW)


def test_a_yaml_that_sets_test_aug_loads(sfod, tmp_path):
    path = os.path.join(str(tmp_path), "tta.yaml")
    with open(path, "w") as f:
        f.write("TEST:\n  AUG:\n    ENABLED: True\n    MIN_SIZES: (300, 450)\n    MAX_SIZE: 900\n    FLIP: False\n")
    cfg = sfod.config.setup_cfg(path, ["TEST.AUG.MAX_SIZE", "800"])
    assert dict(cfg.TEST.AUG) == {"ENABLED": True, "MIN_SIZES": (300, 450), "MAX_SIZE": 800, "FLIP": False}
    opt = sfod.modeling.tta_options.TTAOptions(cfg)
    assert (opt.min_sizes, opt.flip, opt.num_aug) == ((300, 450), False, 2)


@pytest.mark.parametrize("key,value,named", [
    ("MIN_SIZES", (), "TEST.AUG.MIN_SIZES"), ("MIN_SIZES", (400, 0), "TEST.AUG.MIN_SIZES"), ("MIN_SIZES", (-5,), "TEST.AUG.MIN_SIZES"),
    ("MIN_SIZES", (400.5,), "TEST.AUG.MIN_SIZES"), ("MIN_SIZES", (400.0,), "TEST.AUG.MIN_SIZES"), ("MIN_SIZES", (True,), "TEST.AUG.MIN_SIZES"),
    ("MIN_SIZES", "400", "TEST.AUG.MIN_SIZES"), ("MAX_SIZE", 0, "TEST.AUG.MAX_SIZE"), ("MAX_SIZE", -1, "TEST.AUG.MAX_SIZE"),
    ("MAX_SIZE", 4000.0, "TEST.AUG.MAX_SIZE"), ("FLIP", 1, "TEST.AUG.FLIP"), ("FLIP", "horizontal", "TEST.AUG.FLIP"),
    ("FLIP", None, "TEST.AUG.FLIP")])
def test_validation_names_the_key(sfod, key, value, named):
    with pytest.raises(ValueError, match=named.replace(".", r"\.")):
        sfod.modeling.tta_options.validate_tta_cfg(_cfg(sfod, **{key: value}))


def test_validation_of_capacity_and_proposals(sfod):
    T = sfod.modeling.tta_options
    cfg = _cfg(sfod)
    cfg.TEST.DETECTIONS_PER_IMAGE = T.MERGE_CAPACITY // 18
    assert T.TTAOptions(cfg).num_aug * T.TTAOptions(cfg).max_det <= T.MERGE_CAPACITY           # the largest that fits
    cfg.TEST.DETECTIONS_PER_IMAGE = T.MERGE_CAPACITY // 18 + 1
    with pytest.raises(ValueError, match=r"TEST\.AUG\.MIN_SIZES.*TEST\.AUG\.FLIP.*TEST\.DETECTIONS_PER_IMAGE"):
        T.TTAOptions(cfg)
    cfg.TEST.AUG.FLIP = False                                      # half the augmentations: fits again
    assert T.TTAOptions(cfg).num_aug == 9
    with pytest.raises(ValueError, match=r"TEST\.AUG\.MIN_SIZES"):
        T.TTAOptions(_cfg(sfod, MIN_SIZES=tuple(range(100, 100 + T.MAX_AUGMENTATIONS // 2 + 1))))
    cfg = _cfg(sfod)
    cfg.MODEL.LOAD_PROPOSALS = True
    with pytest.raises(ValueError, match=r"MODEL\.LOAD_PROPOSALS"):
        T.TTAOptions(cfg)
    cfg = _cfg(sfod)
    cfg.TEST.DETECTIONS_PER_IMAGE = 0
    with pytest.raises(ValueError, match=r"TEST\.DETECTIONS_PER_IMAGE"):
        T.TTAOptions(cfg)


# ---- the plan builder against hand-computed cases -----------------------------------------------------------------------------
def _row(wa, ha, flip, rx1, ry1, rx2, ry2):
    return tuple(float(F32(v)) for v in (wa, ha, flip, rx1, ry1, rx2, ry2, 0.0))


@pytest.mark.parametrize("flip", [True, False])
def test_plan_of_a_64x107_tensor_of_a_96x160_frame(sfod, flip):
    """48: 0.75 x (64, 107) = (48, 80.25) -> (48, 80).  64: the tensor's own size.  80: 1.25 x (64, 107) = (80, 133.75); the
    long side exceeds 120, so x 120 / 133.75: (71.775.., 120) -> (72, 120)."""
    opt = sfod.modeling.tta_options.TTAOptions(_cfg(sfod, MIN_SIZES=(48, 64, 80), MAX_SIZE=120, FLIP=flip))
    p = opt.plan(64, 107, 96, 160)
    assert p.hw == (64, 107) and p.native_hw == (96, 160) and p.sizes == ((48, 80), (64, 107), (72, 120))
    rep = 2 if flip else 1
    assert len(p.table) == 3 * rep
    rows = [(80, 48, 107 / 80, 64 / 48), (107, 64, 1.0, 1.0), (120, 72, 107 / 120, 64 / 72)]
    want = tuple(_row(wa, ha, f, rx, ry, 160 / 107, 1.5) for (wa, ha, rx, ry) in rows for f in range(rep))
    assert p.table == want
    assert p.table[1 * rep][3:5] == (1.0, 1.0)                                   # 64: the identity-size augmentation
    assert opt.plan(64, 107, 96, 160) is p                                         # cached per (h, w, H0, W0)
    assert opt.plan(64, 107, 64, 107).table[0][5:7] == (1.0, 1.0)                 # no pre transform: ratios 1


def test_plan_of_a_portrait_frame_and_sizes_that_follow_the_tensor_not_the_frame(sfod):
    opt = sfod.modeling.tta_options.TTAOptions(_cfg(sfod, MIN_SIZES=(48, 64, 80), MAX_SIZE=120, FLIP=True))
    p = opt.plan(107, 64, 160, 96)
    assert p.sizes == ((80, 48), (107, 64), (120, 72))
    assert p.table[4] == _row(72, 120, 0, 64 / 72, 107 / 120, 1.5, 160 / 107) and p.table[5][2] == 1.0
    # the sizes follow the test-size tensor, not the native frame: another frame changes the second ratio pair only
    q = opt.plan(64, 107, 100, 100)
    assert q.sizes == ((48, 80), (64, 107), (72, 120)) and q.table[0][5:7] == (float(F32(100 / 107)), float(F32(100 / 64)))
    assert q.table[0][:5] == opt.plan(64, 107, 96, 160).table[0][:5]
    with pytest.raises(ValueError, match="empty frame"):
        opt.plan(0, 107, 96, 160)


def test_plans_agree_with_the_definitions_augmentation_list(sfod):
    opt = sfod.modeling.tta_options.TTAOptions(_cfg(sfod, MIN_SIZES=(37, 48, 80, 131), MAX_SIZE=150, FLIP=True))
    for geom in ((64, 107, 96, 160), (107, 64, 160, 96), (75, 50, 75, 50), (600, 1200, 1024, 2048), (33, 500, 66, 1000)):
        p = opt.plan(*geom)
        augs = D.augmentations(*geom, (37, 48, 80, 131), 150, True)
        assert [a["size"] for a in augs[::2]] == list(p.sizes) and len(augs) == len(p.table)
        assert (C._table([augs], [geom])[0] == np.asarray(p.table, dtype=F32)).all()
    assert D.output_shape(64, 107, 80, 120) == sfod.data.weak_augment.resize_shortest_edge_shape(64, 107, 80, 120) == (72, 120)


# ---- the definition ----------------------------------------------------------------------------------------------------------
def test_inverse_of_a_forward_transformed_box_returns_the_box():
    """Forward and back a coordinate passes 4 multiplications by ratios that are themselves rounded once, and under a flip two
    subtractions from w_a: 10 roundings of at most 2^-24 relative each, on magnitudes bounded by the larger frame in play."""
    g = np.random.RandomState(0)
    for (h, w, H0, W0) in ((64, 107, 96, 160), (107, 64, 160, 96), (75, 50, 75, 50)):
        for aug in D.augmentations(h, w, H0, W0, (48, 64, 80), 120, True):
            xy = g.rand(50, 2) * [W0 * 0.7, H0 * 0.7]
            box = np.concatenate([xy, xy + g.rand(50, 2) * [W0 * 0.3, H0 * 0.3]], 1).astype(F32)
            fwd = D.forward_boxes(box, aug)
            assert (fwd[:, 0] <= fwd[:, 2]).all() and (fwd[:, 1] <= fwd[:, 3]).all()          # also after a flip
            assert fwd[:, 2].max() <= aug["size"][1] * (1 + 1e-6) and fwd[:, 3].max() <= aug["size"][0] * (1 + 1e-6)
            back = D.inverse_boxes(fwd, aug)
            bound = 10 * 2.0 ** -24 * max(H0, W0, *aug["size"])
            assert np.abs(back.astype(np.float64) - box).max() <= bound


def test_apply_box_is_what_it_says_on_a_hand_case():
    b = np.array([[10, 4, 30, 20]], dtype=F32)
    assert D.apply_box(("hflip", 64), b).tolist() == [[34, 4, 54, 20]]
    assert D.apply_box(("resize", 32, 64, 64, 96), b).tolist() == [[15, 8, 45, 40]]
    aug = D.augmentations(64, 128, 128, 256, (32,), 4000, True)[1]
    assert aug["transforms"] == [("resize", 128, 256, 64, 128), ("resize", 64, 128, 32, 64), ("hflip", 64)]
    assert D.inverse_boxes(b, aug).tolist() == [[136, 16, 216, 80]]                     # (64 - 30, 64 - 10) x 2 x 2; y x 2 x 2
    z = D.inverse_boxes(np.array([[20, 4, 20, 12]], dtype=F32), aug)
    assert z[0, 0] == z[0, 2] == 176


def test_one_identity_augmentation_is_fast_rcnn_inference_single_image():
    g = np.random.RandomState(2)
    n, K, hw = 60, 8, (90, 120)
    xy = g.rand(n, 2) * [100, 70] - 5
    boxes = np.concatenate([xy, xy + g.rand(n, 2) * 60], 1).astype(F32)
    scores, classes = g.rand(n).astype(F32), g.randint(0, K, n)
    scores[5], boxes[7, 1], scores[9], scores[10] = np.nan, np.inf, C.THR, C.THR_NEXT
    aug = D.augmentations(*hw, *hw, (90,), 4000, False)
    assert len(aug) == 1 and aug[0]["transforms"] == [("resize", 90, 120, 90, 120)]
    got = D.tta_image([(boxes, scores, classes)], aug, hw, K, 0.5, 100)
    s2d = np.zeros((n, K + 1), dtype=F32)
    s2d[np.arange(n), classes] = scores
    want = D.fast_rcnn_inference_single_image(boxes, s2d, hw, 1e-8, 0.5, 100)
    assert C.same([got], [want]) and got[3] == n - 3 and 0 < len(got[1]) < n - 3
    # ... and that function against the torch formulation it restates (oracle/box_ops.py's clip and NMS on torch's masks)
    tb, ts = torch.from_numpy(boxes), torch.from_numpy(s2d)
    valid = torch.isfinite(tb).all(dim=1) & torch.isfinite(ts).all(dim=1)
    tb, ts = D.OB.clip_boxes(tb[valid], hw), ts[valid][:, :-1]
    mask = ts > 1e-8
    inds = mask.nonzero()
    keep = D.OB.batched_nms(tb[inds[:, 0]], ts[mask], inds[:, 1], 0.5)[:100]
    assert torch.equal(torch.from_numpy(got[0]), tb[inds[:, 0]][keep]) and torch.equal(torch.from_numpy(got[1]), ts[mask][keep])
    assert got[2].tolist() == inds[:, 1][keep].tolist()


# ---- the built inputs and the planted faults ----------------------------------------------------------------------------------
def test_generators_hold_their_edges_and_candidates_agree_with_the_merge():
    for case in C.cases():                                        # raises EdgeMissed otherwise
        exp = C.expected(case)
        for b in range(case["B"]):
            cb, cs, ck, n = C.expected_candidates(case, b)
            assert n == exp[b][3] and ((cs == -1) | (cs > C.THR)).all() and (cb[cs == -1] == 0).all()
            # the candidates, concatenated and merged, are the image's detections
            live = cs >= 0
            s2d = np.zeros((int(live.sum()), case["K"] + 1), dtype=F32)
            s2d[np.arange(len(s2d)), ck[live]] = cs[live]
            again = D.fast_rcnn_inference_single_image(cb[live], s2d, tuple(int(v) for v in case["sizes"][b]), 1e-8,
                                                       case["nms_thresh"], case["topk"])
            assert C.same([again], [exp[b]])
    edges = C.edges_case()
    assert (edges["B"], edges["A"], edges["cap"], edges["K"]) == (2, 6, 100, 8)


@pytest.mark.parametrize("fault", D.FAULTS)
def test_planted_faults_are_caught_by_the_built_inputs(fault):
    """each wrong rule gives other detections or another candidate count on at least one case: the comparison the GPU suite
    applies (``tta_cases.same``: bits of boxes and scores, classes, counts) tells it from the definition"""
    caught = [c["name"] for c in C.cases() if not C.same(C.expected(c), C.expected(c, fault=fault))]
    assert caught, fault
    cand = [c["name"] for c in C.cases() for b in range(c["B"])
            if any((DC_bits(x) != DC_bits(y)).any() for x, y in zip(C.expected_candidates(c, b), C.expected_candidates(c, b, fault)))]
    assert cand, fault


def DC_bits(x):
    x = np.asarray(x)
    return x.astype(F32).view(np.uint32) if x.dtype.kind == "f" else x.astype(np.int64)


# ---- the library's refusals ----------------------------------------------------------------------------------------------------
def test_tta_merge_refuses_bad_arguments_before_any_launch(sfod):
    lib = sfod.native.load()
    import ctypes
    buf = ctypes.create_string_buffer(4096)
    P = ctypes.addressof(buf)
    names = ["det_boxes", "det_scores", "det_classes", "det_count", "aug_table", "image_sizes", "B", "A", "cap", "K", "score_thresh",
             "cand_boxes", "cand_scores", "cand_classes", "cand_count", "stream"]
    valid = [P, P, P, P, P, P, 2, 6, 100, 8, 1e-8, P, P, P, P, None]
    bad = [(n, None) for n in names[:6] + names[11:15]] + [("B", 0), ("B", -1), ("B", 65536), ("A", 0), ("A", -3), ("A", 65),
                                                            ("cap", 0), ("cap", -100), ("cap", 683), ("cap", 2 ** 31 - 1), ("K", 0),
                                                            ("K", -8), ("score_thresh", float("nan")), ("score_thresh", float("inf"))]
    for key, val in bad:
        a = list(valid)
        a[names.index(key)] = val
        assert lib.sfod_tta_merge(*a) == SFOD_EBADARG, (key, val)
        assert lib.sfod_last_error().startswith(b"bad argument: tta_merge"), (key, val)
    names2 = ["cand_boxes", "cand_classes", "sorted_idx", "cand_count", "B", "n", "numel_limit", "s_boxes", "s_alt_boxes", "s_classes",
              "mode", "maxcoord_ws", "stream"]
    valid2 = [P, P, P, P, 2, 600, 20000, P, P, P, P, P, None]
    for key, val in [(n, None) for n in names2[:4] + names2[7:12]] + [("B", 0), ("B", -2), ("n", 0), ("n", -600), ("numel_limit", -1)]:
        a = list(valid2)
        a[names2.index(key)] = val
        assert lib.sfod_frcnn_prepare_nms_cls(*a) == SFOD_EBADARG, (key, val)
        assert lib.sfod_last_error().startswith(b"bad argument: frcnn_prepare_nms_cls"), (key, val)


def test_the_wrapper_refuses_what_has_no_inference_path(sfod):
    class NoHeads(torch.nn.Module):
        roi_heads = None

        def inference(self, x):
            return x

    with pytest.raises(TypeError, match="inference"):
        sfod.modeling.GeneralizedRCNNWithTTA(sfod.config.setup_cfg(None, []), NoHeads())
    with pytest.raises(ValueError, match=r"TEST\.AUG\.FLIP"):
        sfod.modeling.GeneralizedRCNNWithTTA(_cfg(sfod, FLIP=2), NoHeads())
