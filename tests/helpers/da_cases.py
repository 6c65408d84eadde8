"""Inputs of the DA Faster R-CNN tests, shared by tools/record_da_golden.py and the tests: everything is a closed-form function
of integers (no random generator), so the recorder and a test on another machine build bit-identical tensors and the
fixture (tests/golden/da_ref.npz) only has to hold results.  Only tests/ and tools/record_da_golden.py import this module.
"""
import torch

M31 = 2147483647
MAP = (2, 5, 7)                  # B, Hf, Wf of the feature map; stride 32: images of 160 x 224
STRIDE = 32
N_ROWS, N_PAD = 80, 10           # ROI rows (more than one wavefront of ROIs), padding rows among them
WEIGHT_SETS = ((0.01, 0.1, 0.1), (0.25, 0.5, 2.0))      # (w_i, w_n, w_c): the reference's defaults and one other set
POOLERS = ((7, 0, True), (14, 2, False))                # (pooled, sampling_ratio, aligned)
SMALL_RUNS = ((0, 0, 0, "train"), (1, 1, 1, "train"), (0, 1, 0, "eval"))      # (weight set, domain label, pooler, mode) recorded
MODEL_RUNS = ((0, 0), (1, 1))                                                 # (weight set, domain label), pooler 0, training mode
PROBE = 128                      # elements kept of a recorded tensor larger than this (``probe_indices``)


def hashed(shape, seed, scale=1.0):
    """float64 tensor of ``shape``, values in [-scale, scale): integer arithmetic on the element index (exact everywhere),
    one division"""
    n = 1
    for s in shape:
        n *= int(s)
    i = torch.arange(n, dtype=torch.int64)
    v = (i * 2654435761 + int(seed) * 40503 + 12345) % M31
    v = ((v * v) % M31 * 48271 + i) % M31
    return ((v.double() / float(M31)) - 0.5).reshape(shape) * (2.0 * scale)


def as_f32_values(t):
    """the float64 tensor holding exactly the fp32 roundings of ``t``: what both the device (fp32) and the float64 reference use"""
    return t.float().double()


def probe_indices(numel, seed=7):
    """the element positions recorded of a large gradient tensor: all of it up to PROBE elements, else PROBE hashed ones"""
    if numel <= PROBE:
        return torch.arange(numel)
    i = torch.arange(PROBE, dtype=torch.int64)
    return ((i * 2654435761 + seed) % M31 * 48271 % M31) % numel


def roi_rows(seed):
    """[N_ROWS, 5] fp32 (batch index, x1, y1, x2, y2) on 160 x 224 images: N_PAD padding rows interleaved (every 8th row from
    row 3), and among the live ones the five shapes the consistency kernel can get wrong: inside the map, reaching outside
    every border, narrower than a pixel (adaptive grid 1), the whole image (adaptive grid > 1), degenerate (x2 == x1)."""
    B, Hf, Wf = MAP
    H, W = Hf * STRIDE, Wf * STRIDE
    u = hashed((N_ROWS, 5), seed) * 0.5 + 0.5                              # [0, 1)
    x1, y1 = u[:, 0] * (W - 40), u[:, 1] * (H - 40)
    bw, bh = 12 + u[:, 2] * (W * 0.6), 12 + u[:, 3] * (H * 0.6)
    rois = torch.stack([(u[:, 4] * B).floor(), x1, y1, torch.minimum(x1 + bw, torch.tensor(float(W))),
                        torch.minimum(y1 + bh, torch.tensor(float(H)))], 1)
    special = torch.tensor([[0, 40.0, 50.0, 150.0, 120.0],               # inside the map
                            [1, -70.0, -60.0, 300.0, 230.0],             # outside every border
                            [0, 100.0, 30.0, 110.5, 130.0],              # narrower than a feature-map pixel
                            [1, 0.0, 0.0, 224.0, 160.0],                 # the whole image
                            [0, 64.0, 20.0, 64.0, 90.0]], dtype=torch.float64)      # x2 == x1
    rois[:5] = special
    pad = torch.arange(N_PAD) * 8 + 5
    rois[pad] = torch.tensor([-1.0, 0, 0, 0, 0], dtype=torch.float64)
    assert int((rois[:, 0] >= 0).sum()) == N_ROWS - N_PAD
    return rois.float()


def dropout_masks(rows, seed):
    """the four masks of one domain's two DAInsHead evaluations: ((ins fc1, ins fc2), (cons fc1, cons fc2)), uint8 [rows, 1024]"""
    m = [(hashed((rows, 1024), seed + k) >= 0).to(torch.uint8) for k in range(4)]
    return (m[0], m[1]), (m[2], m[3])


def img_head_weights(C, seed, scale=0.05):
    return {"conv1.weight": as_f32_values(hashed((512, C, 1, 1), seed, scale)), "conv1.bias": as_f32_values(hashed((512,), seed + 1, scale)),
            "conv2.weight": as_f32_values(hashed((1, 512, 1, 1), seed + 2, scale)), "conv2.bias": as_f32_values(hashed((1,), seed + 3, scale))}


def ins_head_weights(D, seed, scale=0.05):
    return {"fc1.weight": as_f32_values(hashed((1024, D), seed, scale)), "fc1.bias": as_f32_values(hashed((1024,), seed + 1, scale)),
            "fc2.weight": as_f32_values(hashed((1024, 1024), seed + 2, scale)), "fc2.bias": as_f32_values(hashed((1024,), seed + 3, scale)),
            "fc3.weight": as_f32_values(hashed((1, 1024), seed + 4, scale)), "fc3.bias": as_f32_values(hashed((1,), seed + 5, scale))}


def box_head_weights(C, pooled, seed, D=1024):
    k = C * pooled * pooled
    return {"fc1.weight": as_f32_values(hashed((D, k), seed, (3.0 / k) ** 0.5)), "fc1.bias": as_f32_values(hashed((D,), seed + 1, 0.1)),
            "fc2.weight": as_f32_values(hashed((D, D), seed + 2, (3.0 / D) ** 0.5)), "fc2.bias": as_f32_values(hashed((D,), seed + 3, 0.1))}


def small_case(seed=1):
    """The host tests' case: C = 16 feature channels, D = 32 box features given directly (no box head)."""
    B, Hf, Wf = MAP
    return {"feat": as_f32_values(hashed((B, 16, Hf, Wf), seed, 1.0)), "box_features": as_f32_values(hashed((N_ROWS, 32), seed + 1, 1.0)),
            "rois": roi_rows(seed + 2), "w_img": img_head_weights(16, seed + 10, 0.2), "w_ins": ins_head_weights(32, seed + 20, 0.08),
            "masks": dropout_masks(N_ROWS, seed + 30)}


def model_case(seed=101):
    """The device tests' case, at the smallest sizes the GEMM path takes: features 2 x 512 x 5 x 7, box features
    [80, 1024] read from a fixed 2-FC box head (pooled 7)."""
    B, Hf, Wf = MAP
    return {"feat": as_f32_values(hashed((B, 512, Hf, Wf), seed, 1.0)), "rois": roi_rows(seed + 2),
            "w_box": box_head_weights(512, 7, seed + 40), "w_img": img_head_weights(512, seed + 10, 0.05),
            "w_ins": ins_head_weights(1024, seed + 20, 0.05), "masks": dropout_masks(N_ROWS, seed + 30)}
