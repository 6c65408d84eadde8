"""The forward-convolution planner of the library, host side only (no kernel runs): the shape queries answer what the
recorded table says, a launch whose real ldy / out_dt would write another number of statistics blocks than
sfod_conv_stats_blocks promises is refused, and the process-wide A/B knobs are read back through the queries
(sfod_set_bn_finalize_fused has no query that depends on it: tests/test_gpu_ops.py reads it back through the launch)."""
import ctypes
import importlib.util
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EBADARG = -1000


@pytest.fixture(scope="module")
def lib(sfod):
    lib = sfod.native.load()
    lib.sfod_conv_wgrad_ws_bytes.restype = ctypes.c_int64
    return lib


@pytest.fixture(scope="module")
def dump():
    spec = importlib.util.spec_from_file_location("dump_conv_plans", os.path.join(HERE, "..", "tools", "dump_conv_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_queries_reproduce_the_recorded_plans(lib, dump):
    """tests/golden/conv_fwd_plans.txt: every 211th row of tools/dump_conv_plans.py's sweep (and every hostile row), as the
    library answered before the five queries became readers of one plan.  Each row is asked again from its own extents."""
    with open(os.path.join(HERE, "golden", "conv_fwd_plans.txt")) as f:
        table = [line.rstrip("\n") for line in f]
    assert len(table) >= 800
    assert {r.split(" : ")[1].split()[0] for r in table} == {"0", "1", "2", "3", "4"}      # every answer of sfod_conv_fwd_algo occurs
    lib.sfod_set_gemm_tile(0)
    wrong, err_before = [], lib.sfod_last_error()
    try:
        for row in table:
            asked, want = row.split(" : ")
            algo, *extents = (int(v) for v in asked.split())
            lib.sfod_set_conv_algo(algo)
            got = dump.answers(lib, *extents)
            if got != want:
                wrong.append((asked, want, got))
    finally:
        lib.sfod_set_conv_algo(0)
    assert not wrong, wrong[:10]
    assert lib.sfod_last_error() == err_before          # a query reports nothing, hostile extents included


def test_wgrad_queries_reproduce_the_recorded_plans(lib, dump):
    """tests/golden/conv_wgrad_plans.txt: every 4871st row of tools/dump_conv_plans.py --wgrad (and every hostile and CHUNKED
    row), as the library answered before the three weight-gradient queries became readers of one plan.  (The 24 hostile
    rows with no input channels, no output channels or ksize 0 are recorded as "0 0 0": that library divided by zero on
    them.)  Each row is asked again from its own extents and reproduces the recorded text -- but for a batch that the
    halo-patch kernel walks in sub-batches: there sfod_conv_wgrad_ws_bytes is the largest need of any sub-batch, where the
    recording has the first one's, which a smaller remainder can exceed."""
    with open(os.path.join(HERE, "golden", "conv_wgrad_plans.txt")) as f:
        table = [line.rstrip("\n") for line in f]
    assert len(table) >= 1000
    answers = [tuple(int(v) for v in r.split(" : ")[1].split()) for r in table]
    dets = [int(r.split()[2]) for r in table]
    assert (0, 0, 0) in answers                                                    # not served / nothing to do
    assert any(ws > 0 and oihw == 1 for ws, oihw, _ in answers)                    # halo patch
    assert any(ws > 0 and oihw == 0 and det for (ws, oihw, _), det in zip(answers, dets))      # deterministic slabs
    assert not any(ws > 0 and oihw == 0 and not det for (ws, oihw, _), det in zip(answers, dets))
    assert {a[1] for a in answers} == {0, 1} and {a[2] for a in answers} == {0, 1}
    chunked = {c[:5]: c[5] for c in dump.CHUNKED}
    wrong, moved, err_before = [], set(), lib.sfod_last_error()
    det_before = lib.sfod_get_deterministic()
    try:
        for row in table:
            asked, want = row.split(" : ")
            algo, pipe, det, *e = (int(v) for v in asked.split())
            dump.wgrad_set(lib, algo, pipe, det)
            got = dump.wgrad_answers(lib, *e)
            subs = chunked.get(tuple(e[:5])) if e[5:] == [3, e[4], dump.BF16X3] else None
            if subs and got.split()[1] == "1":
                B, H, W, cin, cout, ks, lddy, dt = e
                need = max(lib.sfod_conv_wgrad_ws_bytes(n, H, W, cin, cout, ks, lddy, dt) for n in subs)
                if got.split()[1:] != want.split()[1:] or int(got.split()[0]) != need:
                    wrong.append((asked, want, got, need))
                if got != want:
                    moved.add(tuple(e[:5]))
            elif got != want:
                wrong.append((asked, want, got))
    finally:
        dump.wgrad_set(lib, 0, 2, det_before)
    assert not wrong, wrong[:10]
    assert moved >= set(c[:5] for c in dump.CHUNKED[:4]), moved       # the four whose remainder wants more than a full sub-batch
    assert lib.sfod_last_error() == err_before          # a query reports nothing, hostile extents included


def _first_layer_launch(lib, stats, buffers):
    """sfod_conv_fwd_scratch on 1 x 64 x 64, 8 -> 64, 3x3: bf16 operands but an fp32 output"""
    x, w, y = buffers
    return lib.sfod_conv_fwd_scratch(x, w, None, None, y, 1, 64, 64, 8, 64, 3, 64, 0, stats, 1, 0, None, ctypes.c_int64(0), None)


def test_launch_refuses_a_statistics_buffer_the_query_sized_for_another_kernel(sfod, lib):
    """sfod_conv_stats_blocks sees neither ldy nor out_dt.  For a bf16 first layer it answers for the first-layer kernel
    (16 blocks here), which does not write fp32: the generic kernel would write 32 blocks + counts into that buffer.  The
    launch is refused before anything runs, and names the query; without statistics the same launch is planned as before."""
    import torch
    n = sfod.native
    assert lib.sfod_conv_fwd_algo(1, 64, 64, 8, 64, 3, n.BF16) == 3
    assert lib.sfod_conv_stats_blocks(1, 64, 64, 8, 64, 3, n.BF16) == 16 != (64 * 64 + 127) // 128
    if torch.cuda.is_available():       # the second launch runs where it can: real operands
        x = torch.zeros(1, 64, 64, 8, dtype=torch.bfloat16, device="cuda")
        w = torch.zeros(64, 9 * 8, dtype=torch.bfloat16, device="cuda")
        y = torch.empty(1, 64, 64, 64, dtype=torch.float32, device="cuda")
        buffers = tuple(ctypes.c_void_p(t.data_ptr()) for t in (x, w, y))
    else:
        host = ctypes.create_string_buffer(64)
        buffers = (ctypes.c_void_p(ctypes.addressof(host)),) * 3
    dummy_stats = ctypes.create_string_buffer(64)       # never dereferenced: the call is refused on the host
    rc = _first_layer_launch(lib, ctypes.c_void_p(ctypes.addressof(dummy_stats)), buffers)
    assert rc == EBADARG
    assert b"sfod_conv_stats_blocks" in lib.sfod_last_error()
    rc = _first_layer_launch(lib, None, buffers)
    # (the error text is sticky: it speaks of this call only where this call failed -- without a GPU, at the launch)
    assert rc != EBADARG and (rc == 0 or b"sfod_conv_stats_blocks" not in lib.sfod_last_error())
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        assert rc == 0 and n.last_conv_kernel() == "k_conv_fwd<bf16_t,float,2,1,0,2,2,0,128>"
    # the dense default the query assumes is served as before (refused later or not at all, never by this check)
    assert lib.sfod_conv_first_supported(1, 64, 64, 8, 64, n.BF16, 64) == 1


CONV3 = (8, 150, 300, 256, 256)         # conv3_2 of a teacher batch: the planner's 256 x 128 halo-patch shape


def test_conv_algo_setter(sfod, lib):
    n = sfod.native
    try:
        assert lib.sfod_conv_fwd_algo(*CONV3, 3, n.BF16X3) == 2
        assert lib.sfod_set_conv_algo(1) == 0
        assert lib.sfod_conv_fwd_algo(*CONV3, 3, n.BF16X3) == 1
        assert lib.sfod_conv_fwd_bnin_supported(*CONV3, n.BF16X3) == 0
        assert lib.sfod_conv_stats_blocks(*CONV3, 3, n.BF16X3) == (8 * 150 * 300 + 127) // 128
        lib.sfod_set_conv_algo(2)
        assert lib.sfod_conv_fwd_algo(1, 7, 7, 64, 64, 3, n.BF16X3) == 2        # 1 automatically: fewer than 8 tiles
        for other in (0, 3, -1):                                                  # anything else is the planner's choice
            lib.sfod_set_conv_algo(other)
            assert lib.sfod_conv_fwd_algo(1, 7, 7, 64, 64, 3, n.BF16X3) == 1
            assert lib.sfod_conv_fwd_algo(*CONV3, 3, n.BF16X3) == 2
    finally:
        lib.sfod_set_conv_algo(0)


def test_conv3x3_variant_setter(sfod, lib):
    """1..9 force a workgroup shape, every other value means the planner's choice"""
    n = sfod.native
    blocks = lambda: lib.sfod_conv_stats_blocks(*CONV3, 3, n.BF16X3)
    bnin = lambda: lib.sfod_conv_fwd_bnin_supported(*CONV3, n.BF16X3)
    try:
        lib.sfod_set_conv3x3_variant(0)
        assert (blocks(), bnin()) == (1440, 1)
        seen = {}
        for v in range(1, 10):
            assert lib.sfod_set_conv3x3_variant(v) == 0
            seen[v] = (blocks(), bnin())
        assert seen[1] == (720, 0)                                # 512-pixel tiles
        assert seen[5] == (1440, 1) and seen[6] == (1440, 1)      # the 256 x 128 shape on 16x16x32 MFMAs: the BatchNorm-input form's
        assert all(seen[v] == (1440, 0) for v in (2, 3, 7, 9))    # 256-pixel tiles of another kernel
        for v in (10, -1, 1 << 20):                               # not 9, not 1: auto
            lib.sfod_set_conv3x3_variant(v)
            assert (blocks(), bnin()) == (1440, 1)
    finally:
        lib.sfod_set_conv3x3_variant(0)


def test_conv3x3_m16_setter(sfod, lib):
    """0 off, 1 / 2 the two 16x16x32 forms; out-of-range values mean 1"""
    n = sfod.native
    bnin = lambda: lib.sfod_conv_fwd_bnin_supported(*CONV3, n.BF16X3)
    try:
        for v, want in ((0, 0), (1, 1), (0, 0), (2, 1), (0, 0), (3, 1), (0, 0), (-1, 1)):
            assert lib.sfod_set_conv3x3_m16(v) == 0
            assert bnin() == want, v
    finally:
        lib.sfod_set_conv3x3_m16(1)


def test_gemm_tile_setter(sfod, lib):
    """0 the planner's choice, 1..8 a forced shape (5: the 256 x 256 tile that sfod_conv_fwd_algo reports as 4, operand pairs
    only); out-of-range values mean 0"""
    n = sfod.native
    fc = (512, 1, 1, 1024, 1024, 1)
    try:
        lib.sfod_set_gemm_tile(0)
        assert lib.sfod_conv_fwd_algo(*fc, n.BF16X3) == 1
        for t, want in ((5, 4), (0, 1), (5, 4), (3, 1), (5, 4), (9, 1), (5, 4), (-1, 1), (8, 1)):
            assert lib.sfod_set_gemm_tile(t) == 0
            assert lib.sfod_conv_fwd_algo(*fc, n.BF16X3) == want, t
        lib.sfod_set_gemm_tile(5)
        assert lib.sfod_conv_fwd_algo(*fc, n.BF16) == 1 and lib.sfod_conv_fwd_algo(*fc, n.F32) == 1     # no such tile there
    finally:
        lib.sfod_set_gemm_tile(0)


def test_deterministic_setter(lib):
    """any non-zero value switches it on; the generic weight gradient then asks for slabs"""
    prev = lib.sfod_get_deterministic()
    fc = (512, 1, 1, 1024, 1024, 1, 1024, 2)
    try:
        for v, want in ((0, 0), (1, 1), (0, 0), (7, 1), (0, 0), (-3, 1)):
            assert lib.sfod_set_deterministic(v) == 0
            assert lib.sfod_get_deterministic() == want
            assert (lib.sfod_conv_wgrad_ws_bytes(*fc) > 0) == bool(want)
    finally:
        lib.sfod_set_deterministic(prev)


def test_wgrad3x3_pipe_setter(lib):
    """2 (and every out-of-range value) the 64 x 64-block kernel on 128-pixel tiles, 1 / 0 the 256-pixel loops: other slabs"""
    shape = (2, 20, 30, 128, 64, 3, 64, 2)
    try:
        for v, want in ((2, 5898240), (1, 7077888), (2, 5898240), (0, 7077888), (3, 5898240), (0, 7077888), (-1, 5898240)):
            assert lib.sfod_set_wgrad3x3_pipe(v) == 0
            assert lib.sfod_conv_wgrad_ws_bytes(*shape) == want, v
    finally:
        lib.sfod_set_wgrad3x3_pipe(2)
