"""The mosaic on the device: ``sfod_mosaic_u8`` (four Pillow-exact up-scales + paste on a 114 canvas + 2x2 halving in one
launch; include/sfod_hip.h) through ``native.mosaic_u8``, the ``MosaicLoader`` on ``cuda`` for the three variants, and two
steps of each of the four source trainers.

The yardstick of every image is the numpy + Pillow definition of tests/helpers/mosaic_definitions.py (pinned to the reference
by tests/test_mosaic_host.py); the comparison is ``np.array_equal`` -- uint8, no tolerance."""
import importlib

import numpy as np
import pytest
import torch

from helpers import mosaic_definitions as D
from helpers.mosaic_cases import bits, case_inputs
from helpers import weak_augment_replay as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _tiles(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8) for h, w in shapes]


def _geometry(mapped, native):
    """the definition's geometry for four (h0, w0) / (Hk, Wk): -> up_hw, rects, out_hw"""
    up, rects = [], []
    for k in range(4):
        _, (h, w) = D.tile_geometry(*mapped[k], *native[k])
        up.append((h, w))
        rects.append(D.rectangles(k, w, h, *native[k]))
    return up, rects, tuple(native[0])


def _golden_case(name):
    tiles, _, _, native = case_inputs(name)
    return [torch.from_numpy(t.copy()) for t in tiles], native


# name -> (tiles on the host, native sizes): golden cases (a)-(c), (f), (g) and the shapes at which the kernel takes another path
def _cases():
    out = {n: _golden_case(n) for n in ("a_exact", "b_letterbox_h", "c_letterbox_w", "f_smaller_native", "g_identity")}
    out["width_129"] = (_tiles([(23, 80)] * 4, 1), [(37, 129)] * 4)              # output width no multiple of 4 or 16, odd height
    out["40x200"] = (_tiles([(25, 125)] * 4, 2), [(40, 200)] * 4)                # several workgroup tiles, the last one partial
    out["down_4x"] = (_tiles([(160, 200)] * 4, 3), [(40, 50)] * 4)               # 9 taps per axis: the generic body
    out["mixed"] = (_tiles([(40, 100), (20, 50), (60, 75), (30, 75)], 4), [(40, 100), (40, 100), (30, 50), (40, 100)])
    return out


CASES = _cases()


@pytest.mark.parametrize("name", list(CASES))
def test_mosaic_kernel_equals_the_definition(native, name):
    tiles, nat = CASES[name]
    up, rects, out_hw = _geometry([tuple(t.shape[1:]) for t in tiles], nat)
    want = D.compose([t.numpy() for t in tiles], up, rects, out_hw)
    got = native.mosaic_u8([t.to(DEV) for t in tiles], up, rects, out_hw)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3,) + out_hw
    assert np.array_equal(got.cpu().numpy(), want), name
    if name == "g_identity":
        assert all(u == tuple(t.shape[1:]) for u, t in zip(up, tiles))
    if name == "down_4x":
        assert native._axis_tabs(torch.device(DEV), 160, 40)[2] > 6


@pytest.mark.parametrize("name", ["b_letterbox_h", "40x200", "width_129"])
def test_tiles_passed_at_canvas_scale_take_the_identity_body(native, name):
    """the ``wq_new`` route: the tiles are up-scaled first (the existing resize launch), then enter the kernel without tables
    -- the same image as the fused call, and as the definition"""
    tiles, nat = CASES[name]
    up, rects, out_hw = _geometry([tuple(t.shape[1:]) for t in tiles], nat)
    ups = [native.resize_bilinear_u8(t.to(DEV), h, w) for t, (h, w) in zip(tiles, up)]
    got = native.mosaic_u8(ups, up, rects, out_hw)
    want = D.compose([t.numpy() for t in tiles], up, rects, out_hw)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(D.compose([u.cpu().numpy() for u in ups], up, rects, out_hw, upscaled=True), want)
    # another fill value, fewer than four tiles: the rest of the canvas is the fill
    got = native.mosaic_u8(ups[:2], up[:2], rects[:2], out_hw, fill=7)
    assert np.array_equal(got.cpu().numpy(), D.compose([u.cpu().numpy() for u in ups[:2]], up[:2], rects[:2], out_hw, 7, upscaled=True))


@pytest.mark.parametrize("why", ["paste-leaves-canvas", "extents-differ", "window-leaves-tile", "negative-origin", "fill-256"])
def test_bad_rectangles_are_refused_and_the_output_stays_untouched(native, why):
    tiles, nat = CASES["a_exact"]
    up, rects, out_hw = _geometry([tuple(t.shape[1:]) for t in tiles], nat)
    rects = [list(map(list, r)) for r in rects]
    fill = 114
    if why == "paste-leaves-canvas":
        rects[3][0][2] += 1
        rects[3][1][2] += 1
    elif why == "extents-differ":
        rects[1][1][3] -= 1
    elif why == "window-leaves-tile":
        rects[2][0] = [0, 31, 48, 64]
        rects[2][1] = [0, 0, 48, 33]
    elif why == "negative-origin":
        rects[0][0][0], rects[0][1][0] = -1, -1
    else:
        fill = 256
    out = torch.full((3,) + out_hw, 0xA5, dtype=torch.uint8, device=DEV)
    with pytest.raises(native.NativeLibraryError, match="sfod_mosaic_u8 failed with code -1000"):
        native.mosaic_u8([t.to(DEV) for t in tiles], up, rects, out_hw, fill=fill, out=out)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())


# ---- loader ------------------------------------------------------------------------------------------------------------------
SMALL = ["OUTPUT_DIR", "", "SEED", "5", "SFOD.SYNTHETIC.HEIGHT", "64", "SFOD.SYNTHETIC.WIDTH", "128", "SFOD.SYNTHETIC.NUM_IMAGES", "8",
         "SFOD.SYNTHETIC.BOXES_PER_IMAGE", "3", "SOLVER.IMS_PER_BATCH", "2", "INPUT.MIN_SIZE_TRAIN", "(40,)"]


@pytest.mark.parametrize("variant", D.VARIANTS)
def test_device_loader_equals_the_cpu_replay_of_its_plans(sfod, native, variant, monkeypatch):
    """Eight 64 x 128 frames mapped to 40 x 80: six items of the device loader, each replayed on the host from its recorded
    plan -- the mapped tiles come from the CPU loader's mapper under the same draws, the strong-augmentation parameters and
    noises recorded in the item go through ``StrongAugmentation.apply`` again."""
    aug = importlib.import_module("simple-sfod_amd.data.augment").StrongAugmentation
    calls = []
    o_mosaic = native.mosaic_u8
    monkeypatch.setattr(native, "mosaic_u8", lambda *a, **k: (calls.append(1), o_mosaic(*a, **k))[1])
    cfg = sfod.config.setup_cfg(R.SRC_YAML, SMALL)
    dev = sfod.data.MosaicLoader(cfg, torch.device(DEV), variant=variant)
    cpu = sfod.data.MosaicLoader(sfod.config.setup_cfg(R.SRC_YAML, SMALL + ["MODEL.DEVICE", "cpu"]), torch.device("cpu"), variant="mosaic")
    assert dev.dataset.device_resize and not cpu.dataset.device_resize
    mapped_log = []
    o_compose = cpu.compose
    cpu.compose = lambda mapped, indices=None: (mapped_log.append(mapped), o_compose(mapped, indices))[1]
    items, plain = [], []
    while len(items) < 6:
        items += next(dev)
        plain += next(cpu)
    torch.cuda.synchronize()
    assert len(calls) >= 6
    for d, c, mapped in zip(items, plain, mapped_log):
        plan = d["mosaic_plan"]
        assert plan.indices == c["mosaic_plan"].indices and d["image"].is_cuda and d["instances"].gt_boxes.tensor.is_cuda
        tiles = [m["image"].numpy() for m in mapped]
        record = list(d.get("strong_params", []))
        assert len(record) == {"mosaic": 0, "mosaic_wq": 1, "mosaic_wq_new": 4}[variant]

        def strong(hwc):
            params, noises = record.pop(0)
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(hwc).transpose(2, 0, 1))).to(DEV)
            return aug.apply(t, params, noises).cpu().numpy().transpose(1, 2, 0)
        want = D.mosaic(tiles, [m["instances"].gt_boxes.tensor.numpy() for m in mapped],
                        [m["instances"].gt_classes.numpy() for m in mapped], [(64, 128)] * 4, variant, strong=strong)
        assert np.array_equal(d["image"].cpu().numpy(), want["image"])
        assert np.array_equal(bits(d["instances"].gt_boxes.tensor.cpu().numpy()), bits(want["boxes"]))
        assert np.array_equal(d["instances"].gt_classes.cpu().numpy(), want["classes"])
        assert (d["height"], d["width"]) == (128, 256) and d["instances"].image_size == (128, 256)
        assert tuple(d["image"].shape) == (3, 64, 128)
        if variant == "mosaic":          # the CPU path itself (numpy / Pillow composition) gives the same item
            assert np.array_equal(c["image"].numpy(), want["image"])


# ---- trainers ------------------------------------------------------------------------------------------------------------------
LOSSES = ["loss_box_reg", "loss_cls", "loss_rpn_cls", "loss_rpn_loc"]


def _two_steps(sfod, name):
    cfg = sfod.config.setup_cfg(R.SRC_YAML, SMALL + ["TRAINER", name, "SOLVER.MAX_ITER", "2", "SOLVER.CHECKPOINT_PERIOD", "0",
                                                     "SFOD.EVAL_HOOK", "False", "TEST.EVAL_PERIOD", "0", "SFOD.DETERMINISTIC", "True"])
    torch.manual_seed(cfg.SEED)
    tr = sfod.engine.get_trainer_class(cfg)(cfg)
    before = tr.optimizer.flat.param.clone()
    steps = []
    for it in range(2):
        tr.iter = it
        tr.run_step()
        tr.scheduler.step()
        rec = tr.storage.flush()
        steps.append([float(rec[k]) for k in LOSSES])
    torch.cuda.synchronize()
    return tr, before, steps


@pytest.mark.parametrize("name", ["base_mosaic", "base_mosaic_wq", "base_mosaic_wq_new", "base_wq"])
def test_each_source_trainer_runs_two_steps_reproducibly(sfod, native, name):
    tr, before, steps = _two_steps(sfod, name)
    mos = importlib.import_module("simple-sfod_amd.data.mosaic")
    assert type(tr) is sfod.engine.trainer.TRAINERS[name] and tr.data_loader.batch == 2
    assert isinstance(tr.data_loader, mos.StrongLoader if name == "base_wq" else mos.MosaicLoader)
    assert all(np.isfinite(v) for s in steps for v in s), steps
    assert not torch.equal(before, tr.optimizer.flat.param)
    _, _, again = _two_steps(sfod, name)
    assert again == steps, (steps, again)
