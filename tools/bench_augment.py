"""Strong-augmentation throughput on one MI355X: per-kernel time on a 3x600x1200 uint8 frame and
frames/s of the sampled pipeline (the mix of transforms build_strong_augmentation draws).  One JSON line.

--weak: the weak augmentation instead -- frames/s of the default path's launch (``native.resize_bilinear_u8`` with a flip on
every other frame, 1024x2048 -> 600x1200), and, where the tree has them, one crop + resize + vertical-flip launch at that size
(``native.weak_augment_u8``) and the host time of the coefficient-table builder for a never-seen shape.  --root DIR imports the
package from another checkout (A/B against a parent tree in one session)."""
import importlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)


def timed(fn, n=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3          # us


def weak(nat, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    img = torch.randint(0, 256, (3, 1024, 2048), generator=g, device=dev, dtype=torch.uint8)
    it = iter(range(10 ** 9))
    windows = [timed(lambda: nat.resize_bilinear_u8(img, 600, 1200, flip=bool(next(it) & 1)), n=400) for _ in range(3)]
    us = sorted(windows)[1]
    out = {"metric": "weak augmentation frames/s (resize 3x1024x2048 -> 600x1200 uint8, flip on every other frame)",
           "value": round(1e6 / us, 1), "unit": "frames/s", "us_per_frame": round(us, 2),
           "us_per_frame_windows": [round(v, 2) for v in windows], "n_gpus": 1, "data": "synthetic"}
    if hasattr(nat, "weak_augment_u8"):
        win = (50, 100, 922, 1843)                                     # a 0.9 x 0.9 crop
        out["crop_resize_vflip_us"] = [round(timed(lambda: nat.weak_augment_u8(img, win, (600, 1199), 2), n=400), 2) for _ in range(3)]
        out["window_copy_vflip_us"] = round(timed(lambda: nat.weak_augment_u8(img, win, win[2:], 2), n=100), 2)
        ts = []
        for k in range(20):                                            # never-seen (in, out) pairs: both axes of one frame
            t0 = time.perf_counter()
            nat.pil_bilinear_coeffs_np(1843 - k, 1199)
            nat.pil_bilinear_coeffs_np(922 - k, 600)
            ts.append((time.perf_counter() - t0) * 1e3)
        out["table_builder_host_ms_per_new_shape"] = round(sorted(ts)[len(ts) // 2], 3)
        t0 = time.perf_counter()
        nat.pil_bilinear_coeffs(1843, 1199)
        nat.pil_bilinear_coeffs(922, 600)
        out["table_builder_loop_version_host_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    print(json.dumps(out))


def main():
    sfod = importlib.import_module("simple-sfod_amd")
    nat = sfod.native
    dev = torch.device("cuda:0")
    if "--weak" in sys.argv:
        return weak(nat, dev)
    H, W = 600, 1200
    img = torch.randint(0, 256, (3, H, W), dtype=torch.uint8, device=dev)
    nbytes = 3 * H * W
    res = {}
    res["jitter4_us"] = timed(lambda: nat.aug_color(img, [(0, 1.1), (1, 0.8), (2, 1.3), (3, 0.05)]))
    res["jitter_no_contrast_us"] = timed(lambda: nat.aug_color(img, [(0, 1.1), (2, 1.3), (3, 0.05)]))
    res["grayscale_us"] = timed(lambda: nat.aug_color(img, [(4, 0.0)]))
    res["blur_us"] = timed(lambda: nat.aug_gaussian_blur(img, 1.5))
    noise = torch.randn(3, 250, 400, device=dev)
    tmp = img.clone()
    res["erase_250x400_us"] = timed(lambda: nat.aug_erase_(tmp, 10, 20, 250, 400, noise))
    aug = sfod.data.StrongAugmentation(torch.Generator().manual_seed(0))
    params = [aug.sample(H, W) for _ in range(64)]
    it = iter(range(10 ** 9))
    us = timed(lambda: aug.apply(img, params[next(it) % 64]), n=256)
    res = {k: round(v, 1) for k, v in res.items()}
    print(json.dumps({"metric": "strong augmentation frames/s (sampled transform mix, 3x600x1200 uint8)",
                      "value": round(1e6 / us, 1), "unit": "frames/s", "us_per_frame": round(us, 1), "n_gpus": 1,
                      "kernels": res,
                      "hbm_GBps_jitter4": round(2 * nbytes * (1 + 0.5) / res["jitter4_us"] / 1e3, 1),
                      "hbm_GBps_blur": round(2 * nbytes * 6 / res["blur_us"] / 1e3, 1), "data": "synthetic"}))


if __name__ == "__main__":
    main()
