"""COCOeval's matching for the device path, on the host (no GPU): the case generators' self-checks, the numpy producer of
``sfod_coco_match``'s format (tests/helpers/coco_match_definitions.py) against ``COCOevalBBox.evaluate()`` -- the definition --
on every case, ``NewCOCOEvaluator(device_match=True)``'s rebuild + ``accumulate`` + ``summarize`` against the host evaluator,
the ``SFOD.COCO_EVAL_DEVICE`` key, the C entry point's refusals, and the merge of two gloo ranks' compact arrays."""
import importlib
import multiprocessing as mp
import os
import sys
import threading

import numpy as np
import pytest
import torch
import torch.distributed as dist

from helpers import coco_match_cases as C
from helpers import coco_match_definitions as Def

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOT = os.path.join(ROOT, "configs", "faster_rcnn_VGG_cityscapes_foggy_adaptive_teacher_source_free.yaml")
SMALL = ["MODEL.DEVICE", "cpu", "SFOD.SYNTHETIC.HEIGHT", "64", "SFOD.SYNTHETIC.WIDTH", "128", "INPUT.MIN_SIZE_TEST", "32",
         "DATASETS.TEST", "('synthetic_cityscapes_foggy_val',)", "SFOD.SYNTHETIC.NUM_TEST_IMAGES", "4", "TEST.IMS_PER_BATCH", "3",
         "SFOD.SYNTHETIC.BOXES_PER_IMAGE", "5"]
CASES = C.all_cases()
IDS = [c["name"] for c in CASES]
A, T = len(C.AREA_RNG), len(C.IOU_THRS)


@pytest.fixture(scope="module")
def produced():
    """every case's packed arrays and the producer's answer, computed once"""
    out = {}
    for c in CASES:
        a = C.pack(c["images"], C.D_CAP, c.get("G"))
        out[c["name"]] = (a, Def.coco_match(a, c["K"], C.IOU_THRS, C.AREA_RNG))
    return out


def test_constants_are_the_evaluators(sfod):
    E = sfod.evaluation
    assert np.array_equal(E.IOU_THRS, C.IOU_THRS) and E.AREA_RNG == C.AREA_RNG
    assert (E.COCO_DET_CAP, E.COCO_GT_CAP) == (C.D_CAP, C.G_CAP) == (sfod.native.COCO_MAX_DET, sfod.native.COCO_MAX_GT)
    assert C.G_CAP >= 256 and A * T <= sfod.native.COCO_MAX_BITS


def test_generators_hold_their_edges():
    assert len(CASES) == 13 and all(len(c["images"]) <= 4 for c in CASES)
    assert len(C.too_many_ground_truths()[0][1]) == C.G_CAP + 1
    assert max(len(d) for c in CASES for d, _ in c["images"]) == C.D_CAP
    assert {max(len(g) for _, g in c["images"]) for c in CASES} >= {63, 64, 65, C.G_CAP}
    assert {c["K"] for c in CASES} >= {1, 80}


def _bit(words, a, t):
    return ((words >> np.uint64(a * T + t)) & np.uint64(1)).astype(bool)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_producer_equals_the_definition_per_image(sfod, produced, case):
    """``_eval_imgs`` entry by entry: dtMatches != 0, dtIgnore, the order of dtScores, count(gtIgnore == 0)"""
    arrs, (rank, match, ignore, npig) = produced[case["name"]]
    gt_anns, dt_anns, img_ids = C.to_coco(case["images"])
    K, I0 = case["K"], len(img_ids)
    ev = sfod.evaluation.COCOevalBBox(gt_anns, dt_anns, range(K), img_ids)
    ev.evaluate()
    assert len(ev._eval_imgs) == K * A * I0
    hits = 0
    for k in range(K):
        for a in range(A):
            for i in range(I0):
                e = ev._eval_imgs[k * A * I0 + a * I0 + i]
                n = int(arrs["det_count"][i])
                idx = np.nonzero(arrs["det_classes"][i, :n] == k)[0]
                idx = idx[np.argsort(rank[i, idx])]
                assert sorted(rank[i, idx].tolist()) == list(range(len(idx)))
                if e is None:
                    assert len(idx) == 0 and npig[i, k, a] == 0
                    continue
                assert np.array_equal(np.array(e["dtScores"], dtype=np.float64), arrs["det_scores"][i, idx].astype(np.float64),
                                      equal_nan=True), (k, a, i)
                assert np.count_nonzero(e["gtIgnore"] == 0) == npig[i, k, a]
                for t in range(T):
                    assert np.array_equal(e["dtMatches"][t] != 0, _bit(match[i, idx], a, t)), (k, a, i, t)
                    assert np.array_equal(e["dtIgnore"][t].astype(bool), _bit(ignore[i, idx], a, t)), (k, a, i, t)
                hits += int((e["dtMatches"] != 0).sum())
    for i in range(I0):                                   # slots in no category: rank -1, empty words
        n = int(arrs["det_count"][i])
        dead = np.ones(C.D_CAP, dtype=bool)
        dead[:n] = (arrs["det_classes"][i, :n] < 0) | (arrs["det_classes"][i, :n] >= K)
        assert (rank[i, dead] == -1).all() and not match[i, dead].any() and not ignore[i, dead].any()
    assert hits > 0, "a case without a single match pins nothing"


def test_the_named_edges_decide_as_the_definition_says(produced):
    """the outcomes the cases were built for, read from the producer's words (which the test above ties to the definition)"""
    _, (_, match, ignore, _) = produced["threshold_edges"]
    for i in range(10):                                   # detection 2i sits ON threshold i, detection 2i + 1 just below it
        assert [bool(_bit(match[0, 2 * i:2 * i + 1], 0, t)[0]) for t in range(T)] == [t <= i for t in range(T)]
        assert [bool(_bit(match[0, 2 * i + 1:2 * i + 2], 0, t)[0]) for t in range(T)] == [t < i for t in range(T)]
    _, (rank, match, _, _) = produced["tied_scores"]
    assert rank[0, :6].tolist() == [1, 2, 0, 4, 3, 0]                       # NaN last, the tie in index order
    assert _bit(match[0, 0:1], 0, 8)[0] and not _bit(match[0, 1:2], 0, 0)[0]        # detection 0 took the ground truth at 0.9
    assert _bit(match[0, 4:5], 0, 9)[0] and not _bit(match[0, 3:4], 0, 0)[0]        # score 0.1 beats the NaN's exact box
    _, (_, match, _, _) = produced["tied_iou"]
    assert _bit(match[0, 1:2], 0, 9)[0]                                     # the earlier ground truth was left for detection 1
    _, (_, match, ignore, npig) = produced["crowd"]
    assert all(_bit(match[0, :3], 0, 9)) and all(_bit(ignore[0, :3], 0, 9))         # three detections on one crowd region
    assert _bit(match[0, 3:4], 0, 2)[0] and not _bit(ignore[0, 3:4], 0, 2)[0]       # the break: IoU 0.6 on the counted one
    assert _bit(match[0, 3:4], 0, 3)[0] and _bit(ignore[0, 3:4], 0, 3)[0]           # above 0.6 only the crowd one is left
    assert _bit(match[0, 4:5], 0, 0)[0] and _bit(ignore[0, 4:5], 0, 0)[0] and npig[0, 2].tolist() == [0, 0, 0, 0]
    assert npig[0, 3].tolist() == [1, 0, 1, 0] and _bit(ignore[0, 5:6], 1, 0)[0] and not _bit(ignore[0, 5:6], 2, 0)[0]
    _, (_, match, ignore, npig) = produced["area_edges"]
    assert npig[0, 0].tolist() == [5, 3, 3, 1]            # 1024 and 9216 count on both sides; the 500 field is small
    assert [bool(_bit(ignore[0, 5:6], a, 0)[0]) for a in range(A)] == [False, False, False, True]
    assert [bool(_bit(ignore[0, 6:7], a, 0)[0]) for a in range(A)] == [False, True, False, False]
    assert [bool(_bit(ignore[0, 7:8], a, 0)[0]) for a in range(A)] == [False, False, True, True]


def _host_results(sfod, images, K):
    ev = sfod.evaluation.NewCOCOEvaluator("cases", C.to_dataset_dicts(images), [f"c{k}" for k in range(K)], distributed=False)
    ev.process(*C.instances(sfod, images, "cpu"))
    return ev.evaluate()


def _fed_from_producer(sfod, images, K, arrs, out, ids=None, distributed=False, all_images=None):
    ev = sfod.evaluation.NewCOCOEvaluator("cases", C.to_dataset_dicts(all_images or images), [f"c{k}" for k in range(K)],
                                          distributed=distributed, device_match=True)
    rank, match, ignore, npig = out
    t = torch.from_numpy
    ev.add_matched(ids if ids is not None else list(range(len(images))), t(arrs["det_scores"]), t(arrs["det_classes"]), t(arrs["det_count"]),
                   t(rank), t(match.view(np.int64)), t(ignore.view(np.int64)), t(npig))
    return ev


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rebuild_accumulate_summarize_equal_the_host_evaluator(sfod, produced, case):
    arrs, out = produced[case["name"]]
    K = case["K"]
    gt_anns, dt_anns, img_ids = C.to_coco(case["images"])
    host = sfod.evaluation.COCOevalBBox(gt_anns, dt_anns, range(K), img_ids)
    host.evaluate()
    host.accumulate()
    host.summarize()
    ev = _fed_from_producer(sfod, case["images"], K, arrs, out)
    res = ev.evaluate()
    assert np.array_equal(ev.coco_eval.eval["precision"], host.eval["precision"])
    assert np.array_equal(ev.coco_eval.eval["recall"], host.eval["recall"])
    assert np.array_equal(ev.coco_eval.stats, host.stats)
    assert (host.eval["precision"] > -1).any()
    assert str(res) == str(_host_results(sfod, case["images"], K)) and list(res) == ["bbox"]
    assert set(ev.timings) == {"copy_s", "rebuild_s", "accumulate_s"}


def test_unprocessed_images_and_empty_sets_follow_the_host_path(sfod):
    images = C.random_images(3, 6, 3)
    arrs = C.pack(images[:4], C.D_CAP)
    out = Def.coco_match(arrs, 3, C.IOU_THRS, C.AREA_RNG)
    ev = _fed_from_producer(sfod, images[:4], 3, arrs, out, all_images=images)       # images 4 and 5 are never processed
    host = sfod.evaluation.NewCOCOEvaluator("cases", C.to_dataset_dicts(images), ["c0", "c1", "c2"], distributed=False)
    host.process(*C.instances(sfod, images[:4], "cpu"))
    assert str(ev.evaluate()) == str(host.evaluate())
    none = [([], g) for _, g in images[:2]]                                          # no detection at all: the NaN table
    arrs = C.pack(none, C.D_CAP)
    ev = _fed_from_producer(sfod, none, 3, arrs, Def.coco_match(arrs, 3, C.IOU_THRS, C.AREA_RNG))
    assert str(ev.evaluate()) == str(_host_results(sfod, none, 3)) and "nan" in str(ev.evaluate())
    fresh = sfod.evaluation.NewCOCOEvaluator("cases", C.to_dataset_dicts(images), ["c0", "c1", "c2"], distributed=False, device_match=True)
    assert fresh.evaluate() == {}                                                    # nothing processed, as on the host
    arrs = C.pack(images[:4], C.D_CAP)
    mixed = _fed_from_producer(sfod, images[:4], 3, arrs, out, all_images=images)
    mixed.process(*C.instances(sfod, images[4:], "cpu", first_id=4))                 # a host batch beside matched ones: refused, not dropped
    with pytest.raises(ValueError, match="cannot be mixed"):
        mixed.evaluate()


def test_ground_truth_table_and_its_cap(sfod):
    E = sfod.evaluation
    images = CASES[4]["images"]                                                      # area_edges: a field that is not w * h
    ev = E.NewCOCOEvaluator("cases", C.to_dataset_dicts(images), ["c0"], device_match=True)
    assert ev._gt_f64.dtype == np.float64 and ev._gt_f64[2].tolist() == [300.0, 0.0, 40.0, 40.0, 500.0]
    assert ev._gt_rows[0].tolist() == list(range(5)) and ev._gt_i32.dtype == np.int32
    at_cap = [([], C.too_many_ground_truths()[0][1][:C.G_CAP])]
    E.NewCOCOEvaluator("cases", C.to_dataset_dicts(at_cap), ["c0"], device_match=True)
    over = [([], [])] * 7 + C.too_many_ground_truths()
    with pytest.raises(ValueError, match=r"image 7 .*257.*host path"):
        E.NewCOCOEvaluator("cases", C.to_dataset_dicts(over), ["c0"], device_match=True)
    E.NewCOCOEvaluator("cases", C.to_dataset_dicts(over), ["c0"])                    # the host path takes it


class _Echo(torch.nn.Module):
    """detections = the ground truth, some of it shifted, at the frame's native size"""

    def __init__(self, sfod):
        super().__init__()
        self.sfod = sfod

    def forward(self, batched_inputs):
        S = self.sfod.structures
        outs = []
        for d in batched_inputs:
            inst = S.Instances((d["height"], d["width"]))
            boxes = d["instances"].gt_boxes.tensor.clone() * (d["width"] / d["image"].shape[2])
            boxes[::3, 0] += 3.3
            inst.pred_boxes = S.Boxes(boxes)
            inst.scores = torch.linspace(0.95, 0.35, len(boxes))
            inst.pred_classes = d["instances"].gt_classes
            outs.append({"instances": inst})
        return outs


def test_coco_eval_device_key(sfod, monkeypatch):
    E, T_ = sfod.evaluation, sfod.engine.BaseTrainer
    name = "synthetic_cityscapes_foggy_val"
    cfg = sfod.config.setup_cfg(HOT, SMALL)
    assert cfg.SFOD.COCO_EVAL_DEVICE is False
    made = []
    init = E.NewCOCOEvaluator.__init__

    def spy(self, *a, **k):
        made.append((len(a), dict(k)))
        init(self, *a, **k)
    monkeypatch.setattr(E.NewCOCOEvaluator, "__init__", spy)

    def forbidden(*a, **k):
        raise AssertionError("the key is off: nothing of the device path may be called")
    for attr in ("_build_gt_table", "_process_device", "_evaluate_matched", "add_matched"):
        monkeypatch.setattr(E.NewCOCOEvaluator, attr, forbidden)
    monkeypatch.setattr(sfod.native, "coco_match", forbidden)
    ev = T_.build_evaluator(cfg, name)
    assert type(ev) is E.NewCOCOEvaluator and ev._device_match is False and not hasattr(ev, "_gt_rows") and not hasattr(ev, "_matched")
    assert made == [(3, {"output_dir": None})]                                       # today's call, argument for argument
    off = T_.test(cfg, _Echo(sfod))
    monkeypatch.undo()
    on_cfg = sfod.config.setup_cfg(HOT, SMALL + ["SFOD.COCO_EVAL_DEVICE", "True"])
    on = T_.build_evaluator(on_cfg, name)
    assert type(on) is E.NewCOCOEvaluator and on._device_match is True and len(on._gt_rows) == 4
    both = T_.build_evaluator(sfod.config.setup_cfg(HOT, SMALL + ["SFOD.COCO_EVAL_DEVICE", "True", "SFOD.EVALUATORS", "('coco', 'f1')"]), name)
    assert [type(e) for e in both._evaluators] == [E.NewCOCOEvaluator, E.F1Evaluator] and both._evaluators[0]._device_match is True
    assert str(T_.test(on_cfg, _Echo(sfod))) == str(off)                             # host tensors: the host path, whatever the key says
    for bad in ("1", "'yes'", "None", "0.0"):
        with pytest.raises(ValueError, match=r"SFOD\.COCO_EVAL_DEVICE"):
            T_.build_evaluator(sfod.config.setup_cfg(HOT, SMALL + ["SFOD.COCO_EVAL_DEVICE", bad]), name)
    cfg = cfg.clone()
    cfg.defrost()
    cfg.SFOD.COCO_EVAL_DEVICE = 1
    with pytest.raises(ValueError, match=r"SFOD\.COCO_EVAL_DEVICE"):
        T_.build_evaluator(cfg, name)


def test_entry_point_refuses_broken_arguments_without_a_gpu(sfod):
    import ctypes
    lib = sfod.native.load()
    proto = sfod.native.parse_header()["sfod_coco_match"]
    assert len(proto[1]) == 22 and proto[1][9:13] == [ctypes.c_int] * 4 and proto[1][13] is ctypes.c_void_p
    failures = []

    def body():      # sfod_last_error is per thread: the messages provoked here stay out of the other tests' thread
        try:
            buf = ctypes.create_string_buffer(1 << 12)
            P = (ctypes.addressof(buf) + 63) // 64 * 64
            thr, rng = (ctypes.c_double * 64)(*([0.5] * 64)), (ctypes.c_double * 128)(*([0.0, 1e10] * 64))
            names = ["det_boxes", "det_scores", "det_classes", "det_count", "gt_boxes", "gt_area", "gt_classes", "gt_iscrowd", "gt_count",
                     "B", "D", "G", "K", "iou_thrs", "T", "area_rng", "A", "rank", "match", "ignore", "npig", "stream"]
            valid = [P] * 9 + [2, 100, 256, 8, ctypes.addressof(thr), 10, ctypes.addressof(rng), 4, P, P, P, P, None]
            sentinel = bytes(buf)

            def refused(changes):
                a = list(valid)
                for key, val in changes.items():
                    a[names.index(key)] = val
                assert lib.sfod_coco_match(*a) == -1000 and lib.sfod_last_error(), changes
                assert bytes(buf) == sentinel
            for changes in ({"A": 5, "T": 13}, {"A": 65, "T": 1}, {"A": 1, "T": 65}, {"A": 0}, {"T": 0}, {"D": 101}, {"D": 0}, {"D": -4},
                            {"G": 257}, {"G": 0}, {"K": 0}, {"K": -1}, {"B": -1}):
                refused(changes)
            for key in names[:9] + ["iou_thrs", "area_rng", "rank", "match", "ignore", "npig"]:
                refused({key: None})
            for bad in (float("nan"), float("inf"), float("-inf")):
                for arr, key, at in ((thr, "iou_thrs", 9), (rng, "area_rng", 0), (rng, "area_rng", 7)):
                    keep, arr[at] = arr[at], bad
                    refused({})
                    arr[at] = keep
            thr[10] = float("nan")                                                    # beyond T: never read
            a = list(valid)
            a[names.index("B")] = 0                                                   # an empty batch is a valid call: nothing is launched
            assert lib.sfod_coco_match(*a) == 0
            a[names.index("A")], a[names.index("T")] = 8, 8                           # 64 bits exactly
            assert lib.sfod_coco_match(*a) == 0
        except BaseException as e:      # noqa: BLE001 -- handed to the test's thread
            failures.append(e)
    before = lib.sfod_last_error()
    th = threading.Thread(target=body)
    th.start()
    th.join()
    if failures:
        raise failures[0]
    assert lib.sfod_last_error() == before


def test_compact_arrays_and_their_merge(sfod):
    E = sfod.evaluation
    images = C.random_images(11, 5, 3)
    arrs = C.pack(images, C.D_CAP)
    rank, match, ignore, npig = Def.coco_match(arrs, 3, C.IOU_THRS, C.AREA_RNG)
    whole = E.coco_compact(list(range(5)), arrs["det_count"], arrs["det_scores"], arrs["det_classes"], rank, match, ignore, npig)
    n = int(arrs["det_count"].sum())
    assert n > 0 and all(len(whole[k]) == n for k in ("det_image", "det_class", "det_score", "det_rank", "det_match", "det_ignore"))
    assert whole["det_match"].dtype == np.uint64 and whole["npig"].shape == (5, 3, A) and whole["image_id"] == list(range(5))
    parts = [E.coco_compact(list(range(s.start, s.stop)), arrs["det_count"][s], arrs["det_scores"][s], arrs["det_classes"][s], rank[s], match[s],
                            ignore[s], npig[s]) for s in (slice(0, 3), slice(3, 5))]
    merged = E.coco_compact_merge(parts)
    assert merged["image_id"] == whole["image_id"]
    for k in whole:
        if k != "image_id":
            assert np.array_equal(merged[k], whole[k], equal_nan=k == "det_score"), k


def _rank_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sfod = importlib.import_module("simple-sfod_amd")
    images = C.random_images(7, 7, 3)
    share = slice(0, 4) if rank == 0 else slice(4, 7)
    arrs = C.pack(images[share], C.D_CAP)
    ev = _fed_from_producer(sfod, images[share], 3, arrs, Def.coco_match(arrs, 3, C.IOU_THRS, C.AREA_RNG),
                            ids=list(range(share.start, share.stop)), distributed=True, all_images=images)
    q.put((rank, str(ev.evaluate())))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_merge_their_compact_arrays_on_rank0(sfod):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 37500 + os.getpid() % 2000
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert res[1] == "{}"                                                            # only the main process gets results
    whole = _host_results(sfod, C.random_images(7, 7, 3), 3)
    assert res[0] == str(whole) and whole["bbox"]["AP"] > 0
