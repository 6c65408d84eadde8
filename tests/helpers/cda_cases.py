"""Inputs of the conditional DA Faster R-CNN tests, shared by tools/record_cda_golden.py and the tests: tests/helpers/da_cases.py
(imported and extended here) plus closed-form class logits, so that the fixture (tests/golden/cda_ref.npz) only has to hold
results.  Only tests/ and tools/record_cda_golden.py import this module.
"""
import torch

from helpers import da_cases as C
from helpers.da_cases import (MAP, STRIDE, N_ROWS, N_PAD, WEIGHT_SETS, POOLERS, PROBE, hashed, as_f32_values,      # noqa: F401
                              probe_indices, roi_rows, dropout_masks)

NUM_CLASSES = 8                                      # the yaml's; C = K + 1 columns of logits
# (weight set, domain label, entropy conditioning, mode) recorded for each case, pooler 0
RUNS = tuple((k, label, ent, mode) for k, label in ((0, 0), (1, 1)) for ent in (False, True) for mode in ("train", "eval"))
PAD_ROWS = tuple(int(i) * 8 + 5 for i in range(N_PAD))      # the padding rows of ``da_cases.roi_rows``
KERNEL_SHAPES = ((2, 8), (9, 32), (9, 1024), (21, 72))      # (C, D) of the kernel tests


def run_name(k, label, ent, mode):
    return f"w{k}/l{label}/e{int(ent)}/{mode}"


def scores(rows, ncls, seed, nan_padding=False):
    """[rows, ncls] fp32 class logits in [-4, 4) with the rows a softmax / entropy kernel can get wrong: row 0 all equal
    (maximum entropy), row 1 one logit 80 above the rest (the others' p ~ 1e-35), row 2 logits around +-80 (exp overflows
    without the maximum subtracted; the low ones' p is an exact zero in fp32: log(0 + 1e-5)), row 4 all equal but one.  ``nan_padding``: NaN on the padding rows of
    ``da_cases.roi_rows`` (their outputs are zeros whatever the logits hold)."""
    s = hashed((rows, ncls), seed, 4.0)
    s[0] = 1.25
    s[1] = hashed((ncls,), seed + 1, 1.0)
    s[1, ncls // 2] += 80.0
    s[2] = hashed((ncls,), seed + 2, 1.0) + 80.0 * torch.where(torch.arange(ncls) % 2 == 0, 1.0, -1.0).double()
    s[4] = -0.5
    s[4, ncls - 1] = 2.0
    s = s.float()
    if nan_padding:
        s[[r for r in PAD_ROWS if r < rows]] = float("nan")
    return s


def small_case(seed=1):
    """``da_cases.small_case`` (D = 32) with class logits [N_ROWS, 9] and the conditioned head's fc1 [1024, 288]"""
    c = C.small_case(seed)
    ncls = NUM_CLASSES + 1
    c["scores"] = scores(N_ROWS, ncls, seed + 50, nan_padding=True)
    c["w_ins"] = C.ins_head_weights(32 * ncls, seed + 60, 0.08)
    return c


def model_case(seed=101):
    """``da_cases.model_case`` (D = 1024) with class logits [N_ROWS, 9] and the conditioned head's fc1 [1024, 9216]"""
    c = C.model_case(seed)
    ncls = NUM_CLASSES + 1
    c["scores"] = scores(N_ROWS, ncls, seed + 50, nan_padding=True)
    c["w_ins"] = C.ins_head_weights(1024 * ncls, seed + 60, 0.05)
    return c
