"""Print what the five forward-convolution queries of the library answer over a grid of layer shapes.

    SFOD_HIP_LIB=path/to/libsfod_hip.so python tools/dump_conv_plans.py [--every N] > plans.txt

Host logic only: no GPU call, no torch.  Two builds whose outputs are identical byte for byte plan every swept layer the
same way; ``--every N`` keeps each N-th row of the grid (and every hostile row), which is how the fixture
tests/golden/conv_fwd_plans.txt was thinned.  One row:

    algo B H W Cin Cout ksize dt : fwd_algo stats_blocks bnin_supported dgrad_bnred_blocks scratch_bytes x 4

``algo`` is the sfod_set_conv_algo setting of the sweep (sfod_set_gemm_tile is 0 throughout); the four scratch answers are
for (out_dt, with_stats) = (fp32, 0), (fp32, 1), (bf16, 0), (bf16, 1).
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


def load(path=None):
    lib = ctypes.CDLL(path or os.environ["SFOD_HIP_LIB"])
    lib.sfod_conv_fwd_scratch_bytes.restype = ctypes.c_int64
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


if __name__ == "__main__":
    every = int(sys.argv[sys.argv.index("--every") + 1]) if "--every" in sys.argv else 1
    sys.stdout.write("".join(r + "\n" for r in rows(load(), every)))
