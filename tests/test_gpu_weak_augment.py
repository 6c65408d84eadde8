"""The weak-augmentation options on the device: ``sfod_resize_bilinear_u8_opt`` (crop window + Pillow-exact bilinear resize +
horizontal / vertical flip in one launch; include/sfod_hip.h) through ``native.weak_augment_u8``, the loaders under INPUT.CROP,
multi-scale INPUT.MIN_SIZE_TRAIN and INPUT.RANDOM_FLIP vertical, and a trainer whose batch shapes change from step to step.

The yardstick of every image is Pillow called here on the numpy-sliced window, then ``np.flip``
(tests/helpers/weak_augment_replay.py); the comparison is ``np.array_equal`` -- uint8, no tolerance.
"""
import numpy as np
import pytest
import torch

from helpers import weak_augment_replay as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (C, H, W, y0, x0, ch, cw, h, w)
CASES = [
    (3, 48, 80, 0, 0, 48, 80, 30, 50),            # full window, tiled body
    (3, 48, 80, 5, 7, 37, 61, 23, 38),            # interior window, odd everything
    (3, 48, 80, 11, 73, 37, 7, 19, 4),            # the window ends at the tensor's last byte with cw < 8: the 8-byte clamp
    (3, 40, 200, 4, 9, 30, 150, 20, 100),         # more than one 64-wide tile, last tile partial, window pitch != cw
    (3, 40, 70, 3, 5, 20, 33, 50, 83),            # up-scaling (3 taps)
    (3, 200, 150, 10, 20, 180, 120, 45, 30),      # 4x down-scaling: ksize_v > 6, the generic body
    (1, 33, 47, 2, 3, 29, 41, 17, 24),            # C != 3
    (3, 64, 130, 0, 1, 64, 129, 64, 129),         # identity scale at an odd byte offset: the copy path, unaligned
]
_frames = {}


def frame(C, H, W):
    """one random frame per shape: (host numpy, device tensor), made once"""
    if (C, H, W) not in _frames:
        img = torch.randint(0, 256, (C, H, W), generator=torch.Generator().manual_seed(C * 1000003 + H * 1009 + W), dtype=torch.uint8)
        _frames[C, H, W] = (img.numpy(), img.to(DEV))
    return _frames[C, H, W]


@pytest.mark.parametrize("flip_mode", [0, 1, 2])
@pytest.mark.parametrize("case", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_opt_kernel_equals_pillow_on_the_window_then_flip(native, case, flip_mode):
    C, H, W, y0, x0, ch, cw, h, w = case
    host, dev = frame(C, H, W)
    ref = R.pillow_weak(host, (y0, x0, ch, cw), (h, w), flip_mode)
    got = native.weak_augment_u8(dev, (y0, x0, ch, cw), (h, w), flip_mode)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (C, h, w)
    assert np.array_equal(got.cpu().numpy(), ref)
    if (y0, x0, ch, cw) == (0, 0, H, W):
        assert torch.equal(native.weak_augment_u8(dev, None, (h, w), flip_mode), got)        # window None = the whole frame


@pytest.mark.parametrize("shape", [(3, 48, 80, 30, 50), (3, 200, 150, 50, 37)], ids=["tiled", "generic"])
def test_old_entry_point_is_the_opt_call_with_the_full_window(native, shape):
    """``native.resize_bilinear_u8(img, h, w, flip)`` == sfod_resize_bilinear_u8_opt by name with (0, 0, H, W) and flip_mode =
    flip, bitwise -- and both equal Pillow."""
    C, H, W, h, w = shape
    host, dev = frame(C, H, W)
    hb, hk, ksh = native._axis_tabs(dev.device, W, w)
    vb, vk, ksv = native._axis_tabs(dev.device, H, h)
    for flip in (False, True):
        old = native.resize_bilinear_u8(dev, h, w, flip=flip)
        out = torch.empty_like(old)
        native.call("sfod_resize_bilinear_u8_opt", dev, out, C, H, W, 0, 0, H, W, h, w, hb, hk, ksh, vb, vk, ksv, int(flip))
        assert torch.equal(old, out)
        assert np.array_equal(old.cpu().numpy(), R.pillow_weak(host, None, (h, w), int(flip)))


@pytest.mark.parametrize("window,flip_mode", [((20, 7, 37, 61), 0), ((5, 30, 37, 61), 0), ((-1, 7, 37, 61), 0), ((5, 7, 37, 61), 3),
                                              ((5, 7, 0, 61), 0)],
                         ids=["rows-leave", "columns-leave", "negative-origin", "flip-mode-3", "empty-window"])
def test_bad_windows_and_flip_modes_are_refused_before_the_launch(native, window, flip_mode):
    """The wrapper raises the project's error and the output buffer, pre-filled with a sentinel, stays untouched."""
    _, dev = frame(3, 48, 80)
    out = torch.full((3, 23, 38), 0xA5, dtype=torch.uint8, device=DEV)
    with pytest.raises(native.NativeLibraryError, match="sfod_resize_bilinear_u8_opt failed with code -1000"):
        native.weak_augment_u8(dev, window, (23, 38), flip_mode, out=out)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())


# ---- loaders ---------------------------------------------------------------------------------------------------------------
def _loader(sfod, *extra, labeled=False, yaml=R.HOT_YAML):
    cfg = sfod.config.setup_cfg(yaml, R.LOADER_OPTS + list(extra))
    return sfod.data.TwoCropLoader(cfg, torch.device(DEV), labeled=labeled)


def _take(loader, n):
    items = []
    while len(items) < n:
        batch = next(loader)
        items += batch if loader.labeled else batch[1]
    torch.cuda.synchronize()
    return items


def test_device_loader_items_equal_the_pillow_replay_of_their_plans(sfod, native, monkeypatch):
    """Eight 96 x 160 frames, MIN_SIZE_TRAIN (32, 48) "range", CROP relative_range [0.6, 0.7], RANDOM_FLIP vertical, SEED 3: 16
    items, each replayed from its recorded plan on the host -- images bit-equal to Pillow, boxes equal to the float32 cast of
    the float64 rule, at least one box lost to the filter; every image is ONE sfod_resize_bilinear_u8_opt launch."""
    import importlib
    syn = importlib.import_module("simple-sfod_amd.data.synthetic")
    names = []
    o_call = native.call

    def call(name, *a, **k):
        names.append(name)
        return o_call(name, *a, **k)
    monkeypatch.setattr(native, "call", call)
    ld = _loader(sfod)
    assert ld.dataset.device_resize and tuple(ld.dataset.items[0]["image"].shape) == (3, R.FRAME_H, R.FRAME_W)
    items = _take(ld, 16)
    assert all(d["image"].is_cuda and d["instances"].gt_boxes.tensor.is_cuda and d["instances"].gt_classes.is_cuda for d in items)
    dropped = R.check_items_against_the_replay(syn, items, R.LOADER_SEED)
    print(f"[weak augment loader] 16 items, {dropped} boxes dropped by the filter, "
          f"{len({tuple(d['image'].shape) for d in items})} different shapes")
    assert dropped >= 1
    assert {d["weak_plan"].flip_mode for d in items} == {0, 2}
    assert len({tuple(d["image"].shape) for d in items}) >= 4
    assert all(32 <= min(d["image"].shape[1:]) <= 48 for d in items)
    assert set(names) == {"sfod_resize_bilinear_u8_opt"} and len(names) >= 16          # (the prefetch maps one batch ahead)


def test_vertical_flip_alone_on_the_device(sfod, native):
    """RANDOM_FLIP vertical, everything else at its default: frames at 32 x 53, about half of them with their rows mirrored."""
    import importlib
    ld = _loader(sfod, "INPUT.MIN_SIZE_TRAIN", "(32,)", "INPUT.MIN_SIZE_TRAIN_SAMPLING", "choice", "INPUT.CROP.ENABLED", "False")
    items = _take(ld, 8)
    assert {d["weak_plan"].flip_mode for d in items} == {0, 2} and all(tuple(d["image"].shape) == (3, 32, 53) for d in items)
    R.check_items_against_the_replay(importlib.import_module("simple-sfod_amd.data.synthetic"), items, R.LOADER_SEED)


def test_multi_scale_and_no_resize_on_the_device(sfod, native):
    """MIN_SIZE_TRAIN (0, 40) "choice" with an absolute crop and a horizontal flip: 0 keeps the crop's size (the copy path of
    the kernel), 40 resizes it."""
    import importlib
    ld = _loader(sfod, "INPUT.MIN_SIZE_TRAIN", "(0, 40)", "INPUT.MIN_SIZE_TRAIN_SAMPLING", "choice", "INPUT.CROP.TYPE", "absolute",
                 "INPUT.CROP.SIZE", "[64, 129]", "INPUT.RANDOM_FLIP", "horizontal", labeled=True)
    items = _take(ld, 16)
    assert {tuple(d["image"].shape) for d in items} == {(3, 64, 129), (3, 40, 81)}
    assert {d["weak_plan"].flip_mode for d in items} == {0, 1}
    R.check_items_against_the_replay(importlib.import_module("simple-sfod_amd.data.synthetic"), items, R.LOADER_SEED)


def test_two_device_loaders_with_one_seed_yield_identical_batches(sfod, native):
    a, b = _loader(sfod), _loader(sfod)
    for _ in range(4):
        (sa, wa), (sb, wb) = next(a), next(b)
        torch.cuda.synchronize()
        assert len(wa) == len(wb) == 2
        for x, y in zip(wa + sa, wb + sb):
            assert x["image_id"] == y["image_id"] and x["weak_plan"] == y["weak_plan"] and torch.equal(x["image"], y["image"])
            assert torch.equal(x["instances"].gt_boxes.tensor, y["instances"].gt_boxes.tensor)
            assert torch.equal(x["instances"].gt_classes, y["instances"].gt_classes)


def test_trainer_steps_survive_batch_shapes_that_change_every_step(sfod, native):
    """Three BaseTrainer iterations (the source-only yaml, its own arithmetic mode, two frames per step) on the loader case
    above: finite losses and at least two different batch tensor shapes among the three steps -- the prefetch, the table
    cache and the per-shape workspaces see a new shape on every step."""
    cfg = sfod.config.setup_cfg(R.SRC_YAML, R.LOADER_OPTS + ["SOLVER.MAX_ITER", "3", "SOLVER.CHECKPOINT_PERIOD", "0",
                                                             "SFOD.EVAL_HOOK", "False"])
    torch.manual_seed(cfg.SEED)
    tr = sfod.engine.BaseTrainer(cfg)
    assert not tr.data_loader.weak.default and tr.data_loader.dataset.device_resize
    shapes, batches, steps = [], [], []
    o_pre, o_write = tr.model.preprocess_image, tr._write_metrics

    def preprocess_image(batched_inputs, *a, **k):
        out = o_pre(batched_inputs, *a, **k)
        batches.append([tuple(d["image"].shape) for d in batched_inputs])
        shapes.append(tuple(out.tensor.shape))
        return out

    def write_metrics(metrics_dict, *a, **k):
        steps.append({key: float(v.detach()) for key, v in metrics_dict.items() if key[:4] == "loss"})
        return o_write(metrics_dict, *a, **k)
    tr.model.preprocess_image, tr._write_metrics = preprocess_image, write_metrics
    tr.train()
    torch.cuda.synchronize()
    print(f"[weak augment trainer] frames per step {batches}, batch tensors {shapes}, losses {steps}")
    assert len(steps) == 3 and tr.iter == 2
    for rec in steps:
        assert sorted(rec) == ["loss_box_reg", "loss_cls", "loss_rpn_cls", "loss_rpn_loc"] and all(np.isfinite(v) for v in rec.values()), rec
    assert all(np.isfinite(v) for k, v in tr.storage.history[-1].items() if "loss" in k)
    assert len(shapes) == 3 and len(set(shapes)) >= 2
