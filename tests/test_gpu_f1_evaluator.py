"""``sfod_f1_count`` on the device: the reference's recorded per-image counts (tests/golden/f1_ref.npz, three parameter sets,
images up to the 100 x 100 capacity), the hand cases of tests/helpers/f1_cases.py, ``F1Evaluator.process`` on device
``Instances`` against the host rule, no synchronisation before ``evaluate()``, and run-to-run identity.  Everything compared
is an integer (or a float made of integers on the host): the gate is equality."""
import os

import numpy as np
import pytest
import torch

from helpers import f1_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f1_ref.npz")


def _dev(arrs):
    return {k: torch.from_numpy(v).to(DEV) for k, v in arrs.items()}


def _count(native, a, K, params):
    return native.f1_count(a["det_boxes"], a["det_scores"], a["det_classes"], a["det_count"], a["gt_boxes"], a["gt_classes"],
                           a["gt_count"], a["scale"], a["clip_size"], K, params[0], int(params[1]), params[2])


def test_fixture_counts_in_batches_of_8_at_full_capacity(native):
    z = np.load(GOLDEN)
    imgs = C.fixture_images(z)
    assert max(z["nd"]) == 100 and max(z["ng"]) == 100 and any(n == 100 and g == 100 for n, g in zip(z["nd"], z["ng"]))
    batches = [(i, _dev(C.pack_arrays(imgs[i:i + 8], 100, 100))) for i in range(0, len(imgs), 8)]
    for p, params in enumerate(z["params"]):
        got = torch.cat([_count(native, a, 8, params) for _, a in batches]).cpu().numpy()
        for i, img in enumerate(imgs):              # class_number = 8 on the device; the reference ran K of the image
            assert (got[i, :img[0]] == z["counts"][p, i, :img[0]]).all(), (p, i, got[i].tolist(), z["counts"][p, i].tolist())


def test_hand_cases_and_padding_on_the_device(sfod, native):
    for case in C.HAND_CASES:
        for poison in (False, True):
            a = C.pack(case["images"], 7, 5, poison=poison)
            got = _count(native, _dev(a), case["K"], case["params"]).sum(dim=0).cpu().numpy()
            assert got.tolist() == case["counts"], (case["name"], poison, got.tolist())
            ev = sfod.evaluation.F1Evaluator(case["K"], *case["params"])
            t = {k: torch.from_numpy(v) for k, v in a.items()}
            ev.process_batched(t["det_boxes"], t["det_scores"], t["det_classes"], t["det_count"],
                               sfod.modeling.batched.BatchedGT(t["gt_boxes"], t["gt_classes"], t["gt_count"], None),
                               t["scale"], t["clip_size"])
            assert (ev.accumulated() == got).all(), case["name"]


def _instances(sfod, imgs, device, factor):
    """dicts as ``inference_on_dataset`` hands them over: ground truth at the loader's size, detections at a native size
    ``factor`` times larger (as ``GeneralizedRCNN.inference`` returns them)"""
    S = sfod.structures
    inputs, outputs = [], []
    for i, (_, db, ds, dc, gb, gc, (h, w)) in enumerate(imgs):
        gi = S.Instances((h, w))
        gi.gt_boxes = S.Boxes(torch.from_numpy(gb).reshape(-1, 4).to(device))
        gi.gt_classes = torch.from_numpy(gc).long().to(device)
        oi = S.Instances((int(h * factor), int(w * factor)))
        oi.pred_boxes = S.Boxes((torch.from_numpy(db).reshape(-1, 4) * factor).to(device))
        oi.scores = torch.from_numpy(ds).to(device)
        oi.pred_classes = torch.from_numpy(dc).long().to(device)
        inputs.append({"image_id": i, "instances": gi})
        outputs.append({"instances": oi})
    return inputs, outputs


def test_process_on_device_instances_equals_the_host_path_without_a_synchronisation(sfod, native):
    z = np.load(GOLDEN)
    imgs = C.fixture_images(z)[-24:]
    host, dev = sfod.evaluation.F1Evaluator(8, 0.3, 100, 0.05), sfod.evaluation.F1Evaluator(8, 0.3, 100, 0.05)
    batches = [(_instances(sfod, imgs[i:i + 8], "cpu", 1.7), _instances(sfod, imgs[i:i + 8], DEV, 1.7)) for i in range(0, 24, 8)]
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")          # raises a Python error at a synchronising call; faults nothing
    try:
        for _, (inputs, outputs) in batches:
            dev.process(inputs, outputs)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    for (inputs, outputs), _ in batches:
        host.process(inputs, outputs)
    assert dev._dev is not None and dev._dev.is_cuda and dev._dev.dtype == torch.int64 and not dev._host.any()
    assert (dev.accumulated() == host.accumulated()).all() and host.accumulated().sum() > 0
    rd, rh = dev.evaluate(), host.evaluate()
    assert rd == rh and list(rd) == ["F1 Score"] and 0 < rd["F1 Score"] < 1
    assert dev.counts.dtype == np.int64 and dev.counts.shape == (8, 3) and (dev.counts == host.counts).all()


def test_two_launches_give_identical_counts(native):
    z = np.load(GOLDEN)
    first_full = int(np.nonzero((z["nd"] == 100) & (z["ng"] == 100))[0][0])
    a = _dev(C.pack_arrays(C.fixture_images(z)[first_full:first_full + 8], 100, 100))
    first, second = _count(native, a, 8, (0.3, 100, 0.05)), _count(native, a, 8, (0.3, 100, 0.05))
    assert torch.equal(first, second) and int(first.sum()) > 0
