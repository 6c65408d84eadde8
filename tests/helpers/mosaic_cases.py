"""Access to tests/golden/mosaic_ref.npz (recorded by tools/record_mosaic_golden.py from the reference), shared by
tests/test_mosaic_host.py and tests/test_gpu_mosaic.py: the file is read once."""
import importlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
CASES = ("a_exact", "b_letterbox_h", "c_letterbox_w", "d_one_empty", "d_all_empty", "e_clip", "f_smaller_native", "g_identity")
_gold = {}


def gold():
    if not _gold:
        with np.load(os.path.join(GOLDEN, "mosaic_ref.npz")) as z:
            _gold.update({k: z[k] for k in z.files})
    return _gold


def case_inputs(name):
    g = gold()
    return ([g[f"{name}/tile{k}"] for k in range(4)], [g[f"{name}/boxes{k}"] for k in range(4)],
            [g[f"{name}/classes{k}"] for k in range(4)], [tuple(int(v) for v in hw) for hw in g[f"{name}/native"]])


def mosaic_module():
    return importlib.import_module("simple-sfod_amd.data.mosaic")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
