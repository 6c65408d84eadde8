"""Print what the five forward-convolution queries of the library answer over a grid of layer shapes, or (``--wgrad``) the
three weight-gradient queries.

    SFOD_HIP_LIB=path/to/libsfod_hip.so python tools/dump_conv_plans.py [--wgrad] [--every N] > plans.txt

Host logic only: no GPU call, no torch.  Two builds whose outputs are identical byte for byte plan every swept layer the
same way; ``--every N`` keeps each N-th row of the grid (and every hostile row), which is how the fixture
tests/golden/conv_fwd_plans.txt was thinned.  One row:

    algo B H W Cin Cout ksize dt : fwd_algo stats_blocks bnin_supported dgrad_bnred_blocks scratch_bytes x 4

``algo`` is the sfod_set_conv_algo setting of the sweep (sfod_set_gemm_tile is 0 throughout); the four scratch answers are
for (out_dt, with_stats) = (fp32, 0), (fp32, 1), (bf16, 0), (bf16, 1).

``--wgrad`` (the fixture tests/golden/conv_wgrad_plans.txt): the same grid under every sfod_set_conv_algo 0..4, sfod_set_wgrad3x3_pipe
0 / 1 / 2 and sfod_set_deterministic 0 / 1, with three row strides of dy per shape.  One row:

    algo pipe det B H W Cin Cout ksize lddy dt : wgrad_ws_bytes wgrad_oihw_supported first_wgrad_bn_supported

(the last for pool = 0, y_dt = fp32).  The hostile rows are asked under both deterministic settings only; the CHUNKED
shapes, under every setting, are kept whatever ``--every`` says.
"""
import ctypes
import itertools
import os
import sys

F32, BF16, BF16X3, F16X3 = 0, 1, 2, 3
BATCHES = (1, 2, 8)
MAPS = ((1, 1), (7, 7), (18, 37), (37, 75), (64, 64), (75, 150), (150, 300), (300, 600), (600, 1200), (1024, 2048))
CHANNELS = (1, 3, 5, 8, 15, 32, 64, 128, 256, 512, 1024, 2048, 4096, 25088)
# linear layers are rows x 1 x 1: the ROI head's row counts for one and eight frames
ROWS = (512, 4096)
# negative, zero, products past 2^31 (B, H, W, Cin, Cout, ksize)
HOSTILE = ((-1, 64, 64, 64, 64, 3), (1, -64, 64, 64, 64, 3), (1, 64, 64, -8, 64, 1), (1, 64, 64, 64, -64, 3),
           (1, 64, 64, 64, 64, -1), (0, 64, 64, 64, 64, 3), (1, 0, 64, 64, 64, 1), (8, 64, 64, 0, 64, 3),
           (8, 64, 64, 64, 0, 3), (1, 64, 64, 64, 64, 0), (1, 64, 64, 64, 64, 9), (65536, 65536, 1, 8, 8, 1),
           (8, 46341, 46341, 64, 64, 3), (1, 64, 64, 2 ** 31 - 70000, 64, 3), (1, 64, 64, 64, 2 ** 31 - 70000, 3),
           (2 ** 31 - 1, 1, 1, 64, 64, 1), (4096, 512, 1, 2 ** 20, 8, 1))
# weight gradient: hostile row strides of dy on a served shape (B, H, W, Cin, Cout, ksize, lddy)
HOSTILE_LDDY = ((8, 64, 64, 64, 64, 3, -8), (8, 64, 64, 64, 64, 3, 2 ** 31 - 1))
# bf16x3 3x3 layers (lddy = Cout) that the halo-patch weight gradient walks in sub-batches -- its 32-bit byte offsets allow
# fewer than 2^29 elements of x / dy per launch -- with the images per sub-batch.  The first four have a remainder that
# wants more slabs than a full sub-batch; the last two are controls (even halves; one sub-batch, the first layer's form)
CHUNKED = ((9, 750, 1333, 8, 64, (5, 4)), (7, 608, 1216, 8, 128, (4, 3)), (9, 750, 1333, 64, 64, (5, 4)),
           (13, 800, 1333, 8, 64, (7, 6)), (8, 1024, 2048, 64, 64, (4, 4)), (2, 750, 1333, 8, 64, (2,)))


def load(path=None):
    lib = ctypes.CDLL(path or os.environ["SFOD_HIP_LIB"])
    lib.sfod_conv_fwd_scratch_bytes.restype = ctypes.c_int64
    lib.sfod_conv_wgrad_ws_bytes.restype = ctypes.c_int64
    return lib


def shapes():
    for B, (H, W), cin, cout, ks in itertools.product(BATCHES, MAPS, CHANNELS, CHANNELS, (1, 3)):
        yield B, H, W, cin, cout, ks
    for R, cin, cout in itertools.product(ROWS, CHANNELS, CHANNELS):
        yield R, 1, 1, cin, cout, 1


def answers(lib, B, H, W, cin, cout, ks, dt):
    """the five queries on one shape, as the text after the colon of a row"""
    e = (B, H, W, cin, cout)
    out = [lib.sfod_conv_fwd_algo(*e, ks, dt), lib.sfod_conv_stats_blocks(*e, ks, dt),
           lib.sfod_conv_fwd_bnin_supported(*e, dt), lib.sfod_conv_dgrad_bnred_blocks(*e, dt)]
    out += [lib.sfod_conv_fwd_scratch_bytes(*e, ks, dt, odt, ws) for odt in (F32, BF16) for ws in (0, 1)]
    return " ".join(str(v) for v in out)


def rows(lib, every=1):
    lib.sfod_set_gemm_tile(0)
    try:
        for algo in (0, 1, 2):
            lib.sfod_set_conv_algo(algo)
            grid = itertools.product(shapes(), (F32, BF16, BF16X3, F16X3))
            picked = (r for i, r in enumerate(grid) if i % every == 0)
            for shape, dt in itertools.chain(picked, itertools.product(HOSTILE, (F32, BF16, BF16X3, F16X3))):
                yield "%d %d %d %d %d %d %d %d : %s" % ((algo,) + shape + (dt, answers(lib, *shape, dt)))
    finally:
        lib.sfod_set_conv_algo(0)


def wgrad_answers(lib, B, H, W, cin, cout, ks, lddy, dt):
    """the three weight-gradient queries on one shape, as the text after the colon of a row"""
    return "%d %d %d" % (lib.sfod_conv_wgrad_ws_bytes(B, H, W, cin, cout, ks, lddy, dt),
                         lib.sfod_conv_wgrad_oihw_supported(B, H, W, cin, cout, ks, lddy, dt),
                         lib.sfod_conv_first_wgrad_bn_supported(B, H, W, cin, cout, 0, dt, F32))


def wgrad_set(lib, algo, pipe, det):
    lib.sfod_set_conv_algo(algo)
    lib.sfod_set_wgrad3x3_pipe(pipe)
    lib.sfod_set_deterministic(det)


def wgrad_rows(lib, every=1, hostile=HOSTILE):
    """``hostile``: the hostile shapes to ask (a library from before conv_wgrad_plan divides by zero on those with pixels
    but no input channels, no output channels or ksize 0: leave them out to sweep it)"""
    det_before = lib.sfod_get_deterministic()
    row = lambda knobs, e: "%d %d %d %d %d %d %d %d %d %d %d : %s" % (knobs + e + (wgrad_answers(lib, *e),))
    lib.sfod_set_first_wgrad_fused(1)
    try:
        i = 0
        for knobs in itertools.product((0, 1, 2, 3, 4), (0, 1, 2), (0, 1)):
            wgrad_set(lib, *knobs)
            for (B, H, W, cin, cout, ks), dt in itertools.product(shapes(), (F32, BF16, BF16X3, F16X3)):
                for lddy in (cout, (cout + 7) // 8 * 8, (cout + 7) // 8 * 8 + 8):
                    if i % every == 0:
                        yield row(knobs, (B, H, W, cin, cout, ks, lddy, dt))
                    i += 1
            for B, H, W, cin, cout, _ in CHUNKED:
                yield row(knobs, (B, H, W, cin, cout, 3, cout, BF16X3))
        for det in (0, 1):
            wgrad_set(lib, 0, 2, det)
            for e, dt in itertools.product([h + (h[4],) for h in hostile] + list(HOSTILE_LDDY), (F32, BF16, BF16X3, F16X3)):
                yield row((0, 2, det), e + (dt,))
    finally:
        wgrad_set(lib, 0, 2, det_before)


if __name__ == "__main__":
    every = int(sys.argv[sys.argv.index("--every") + 1]) if "--every" in sys.argv else 1
    for r in (wgrad_rows if "--wgrad" in sys.argv else rows)(load(), every):
        sys.stdout.write(r + "\n")
