"""``bench.py`` as it is run for every change: a plain run prints the headline line and nothing that only ``--full``
measures, and ``--dump-outputs`` writes what the last timed step computed (bounded, float32 / float64 only)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(tmp_path, out):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--dump-outputs", str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()[-4000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_timed_step(tmp_path):
    out = tmp_path / "dump"
    d = _plain_run(tmp_path, out)
    assert d["config"]["deterministic"] is True
    assert d["steps"] == 3 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert d["unit"] == "images/s" and d["higher_is_better"] is True and d["dtype"] == "bf16x3"
    assert abs(d["ms_per_step"] - 1000.0 * d["timed_region_s"] / 3) < 0.01 * d["ms_per_step"]
    assert abs(d["value"] - 8 * 3 / d["timed_region_s"]) < 0.01 * d["value"]
    for k in ("roofline", "gpu_fill", "cpu_baseline", "other_shapes", "other_parity_modes", "reduced_precision_mode",
              "gpu_telemetry", "exchange"):
        assert k not in d, k

    files = sorted(os.listdir(out))
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
    a = {f[:-4]: np.load(out / f) for f in files if f.endswith(".npy")}
    assert len(a) == len(files)
    for name in ("total_loss", "loss_cls_pseudo", "loss_box_reg_pseudo", "roi_head.num_pseudo_proposals", "pseudo_boxes",
                 "pseudo_classes", "pseudo_count", "student_params", "student_grad", "teacher_params"):
        assert name in a, name
    for name, v in a.items():
        assert v.dtype in (np.float32, np.float64), (name, v.dtype)
        assert np.isfinite(v).all(), name
    # the dumped scalars are the last step's: the line's ``losses`` (the storage's last values) say the same
    for k in ("loss_cls_pseudo", "loss_rpn_cls_pseudo", "roi_head/num_pseudo_proposals"):
        assert abs(float(a[k.replace("/", ".")]) - d["losses"][k]) < 1e-4, k
    count = a["pseudo_count"]
    assert count.shape == (8,) and abs(count.mean() - float(a["roi_head.num_pseudo_proposals"])) < 1e-3
    assert a["pseudo_boxes"].shape[:1] == (8,) and a["pseudo_boxes"].shape[2] == 4
    assert not a["pseudo_boxes"][np.arange(a["pseudo_boxes"].shape[1])[None, :] >= count[:, None]].any()
    assert a["student_params"].shape == a["student_grad"].shape == a["teacher_params"].shape
    assert np.abs(a["student_grad"]).max() > 0


@pytest.mark.gpu
def test_two_runs_with_the_same_arguments_write_the_same_outputs(tmp_path):
    """Seeded inputs, the same planted head, and a step without float atomics (SFOD.DETERMINISTIC): every file of
    --dump-outputs -- losses, pseudo labels, parameter / gradient samples -- has the same bits in a second run."""
    a, b = tmp_path / "a", tmp_path / "b"
    da, db = _plain_run(tmp_path, a), _plain_run(tmp_path, b)
    assert da["config"]["planted_labels"] == db["config"]["planted_labels"]
    assert da["losses"] == db["losses"]
    files = sorted(os.listdir(a))
    assert files == sorted(os.listdir(b)) and files
    for f in files:
        assert np.array_equal(np.load(a / f), np.load(b / f)), f
