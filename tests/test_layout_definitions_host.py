"""CPU tests of the layout definitions (tests/helpers/layout_definitions.py), of the comparison the GPU suite applies
(tests/helpers/layout_cases.py::assert_bytes) and of the two argument refusals of csrc/elementwise.hip.

1. every definition against a second formulation: explicit index loops in numpy on tiny shapes, integer arithmetic for the
   roundings; the weight scale against oracle/split_precision.py and against its stated window;
2. planted faults, in the manner of tests/test_definition_checker.py: each applied to a correct packed tensor must fail the
   comparison of tests/test_gpu_layout_definition.py;
3. sfod_cast with a storage type it does not serve and the fc packer / unpacker with K % chw_c != 0 return SFOD_EBADARG
   before any launch (the library loads without a GPU).
"""
import math

import numpy as np
import pytest
import torch

from helpers import layout_cases as lc
from helpers import layout_definitions as ld
from oracle import split_precision as sp

SFOD_EBADARG = -1000
INF, NAN = float("inf"), float("nan")


# ---- 1. second formulations ------------------------------------------------------------------------------------------------
def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)


def _bf16_loop(x):
    """round to nearest even on the integer pattern: add 0x7fff + the kept part's lowest bit, cut 16 bits"""
    out = []
    for b in _bits(x).reshape(-1):
        if (b & 0x7FFFFFFF) > 0x7F800000:
            out.append(0x7FFF)                      # NaN (canonical)
        else:
            out.append(((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF)
    return np.array(out, dtype=np.int64)


def _special():
    return torch.tensor([0.0, -0.0, 1.0, 1e-30, -3e38, 65504.0, 2.0 ** -126, 1 + 2.0 ** -12, NAN, 70000.0, -131000.0, 65519.9,
                         2.0 ** -20, INF, -INF, -65504.0, 65519.99, 0.1, -1 / 3, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -9, 3.3e38, 1e-3, 255.5])


def test_bf16_rounds_to_nearest_even():
    x = torch.cat([_special(), lc.distinct_values((64,), seed=1)])
    got = ld.canonical(ld.encode(x, "bf16"), "bf16").view(torch.int16).numpy().astype(np.int64) & 0xFFFF
    assert np.array_equal(got, _bf16_loop(x.numpy()))
    assert torch.equal(ld.bf16(x).view(torch.bfloat16)[:8], x.bfloat16()[:8])


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_pairs_layout_and_values(fmt):
    """8 hi then 8 lo per group; the values of oracle/split_precision.py::split_pairs; unpairs = fp32(hi) + fp32(lo)."""
    x = torch.cat([_special(), lc.distinct_values((40,), seed=2)])
    assert x.numel() % 8 == 0
    bits = ld.pairs(x, fmt)
    hi, lo = sp.split_pairs(x, fmt)
    t = torch.bfloat16 if fmt == "bf16" else torch.float16
    for i in range(x.numel()):
        g, j = divmod(i, 8)
        h = bits[16 * g + j:16 * g + j + 1].view(t).double()
        l = bits[16 * g + 8 + j:16 * g + 8 + j + 1].view(t).double()
        for got, want in ((h, hi[i]), (l, lo[i])):
            assert (torch.isnan(got) and torch.isnan(want)) or (got == want and torch.signbit(got) == torch.signbit(want)), (i, got, want)
        back = ld.unpairs(bits, fmt)[i]
        want = (h.float() + l.float())[0]
        assert (torch.isnan(back) and torch.isnan(want)) or back == want
    if fmt == "f16":
        v = ld.unpairs(bits, fmt)
        assert v[4] == -65504.0 and v[9] == 65504.0 and v[13] == 65504.0 and v[14] == -65504.0 and torch.isnan(v[8])
        lo16 = bits.reshape(-1, 16)[:, 8:].reshape(-1)
        assert all(int(lo16[i]) & 0x7FFF == 0 for i in (4, 9, 10, 13, 14))            # saturated: lo = 0


def test_weight_scale_against_the_oracle_and_its_window():
    g = torch.Generator().manual_seed(0)
    for e in list(range(-125, 127, 7)) + [-14, -3, 0, 13, 14]:
        for m in (1.0, 1.5, 2.0 - 2.0 ** -23):
            w = torch.rand(50, generator=g) * 0.5 * 2.0 ** e
            w[7] = -m * 2.0 ** e                                # the maximum, negative
            s = ld.weight_scale(w)
            amax = float(w.abs().max())
            assert ld.weight_scale_bits(w) == int(_bits([amax])[0])
            want_exp = 13 - math.floor(math.log2(amax))
            if -119 <= want_exp <= 119:                      # inside the clamp [8, 246] of the biased exponent
                assert s == sp.weight_scale(w)
                assert 2.0 ** 13 <= amax * s < 2.0 ** 14
            else:
                assert s == 2.0 ** max(min(want_exp, 119), -119)
    assert ld.scale_from_bits(int(_bits([2.0 ** -120])[0])) == 2.0 ** 119            # asks for 260, gets 246
    assert ld.scale_from_bits(int(_bits([2.0 ** 120])[0])) == 2.0 ** -107
    assert ld.scale_from_bits(int(_bits([3.0e38])[0])) == 2.0 ** -114                # the largest binade: far from the lower clamp
    for special, word in ((torch.zeros(8), 0), (torch.tensor([1e-40, -2e-40]), int(_bits([2e-40])[0])),
                          (torch.tensor([1.0, -INF]), 0x7F800000), (torch.tensor([INF, NAN, 1.0]), 0x7FC00000)):
        assert ld.weight_scale_bits(special) == word
        assert ld.weight_scale(special) == 1.0
    assert sp.weight_scale(torch.zeros(8)) == 1.0 and sp.weight_scale(torch.tensor([1.0, INF])) == 1.0


@pytest.mark.parametrize("rot", [False, True])
@pytest.mark.parametrize("ks", [1, 3])
def test_conv_weight_layout_against_index_loops(ks, rot):
    cout, cin, taps = 5, 3, ks * ks
    w = lc.distinct_values((cout, cin, ks, ks), seed=3)
    pad = 8
    rows, inner = (cin, cout) if rot else (cout, cin)
    want = np.zeros((rows, taps, pad), dtype=np.float32)
    wn = w.numpy().reshape(cout, cin, taps)
    for co in range(cout):
        for ci in range(cin):
            for tap in range(taps):
                if rot:
                    want[ci][tap][co] = wn[co][ci][taps - 1 - tap]
                else:
                    want[co][tap][ci] = wn[co][ci][tap]
    got = ld.conv_weight(w, pad, rot)
    assert got.shape == (rows, taps, pad) and np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
    if not rot:
        back = ld.conv_wgrad(got, cout, cin, ks)
        assert torch.equal(back, w)
        junk = got.clone()
        junk[:, :, cin:] = 7.0                                  # pad columns never arrive in the gradient
        assert torch.equal(ld.conv_wgrad(junk, cout, cin, ks), w)


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("chw_c", [0, 3])
def test_fc_weight_layout_against_index_loops(chw_c, transpose):
    n, c, pp = 4, 3, 5
    k = c * pp
    w = lc.distinct_values((n, k), seed=4)
    inner = n if transpose else k
    ldim = inner + 3
    want = np.zeros((k if transpose else n, ldim), dtype=np.float32)
    wn = w.numpy()
    for r in range(n):
        for ch in range(c):
            for p in range(pp):
                kp = p * c + ch if chw_c else ch * pp + p
                if transpose:
                    want[kp][r] = wn[r][ch * pp + p]
                else:
                    want[r][kp] = wn[r][ch * pp + p]
    got = ld.fc_weight(w, chw_c, transpose, ldim)
    assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
    if not transpose:
        junk = got.clone()
        junk[:, k:] = 7.0
        assert torch.equal(ld.fc_wgrad(junk, n, k, chw_c, ldim), w)


def test_encode_is_the_storage_of_each_type():
    x = lc.distinct_values((16,), seed=5, amp=2.0 ** -4)
    assert torch.equal(ld.encode(x, "fp32").view(torch.float32), x)
    assert torch.equal(ld.encode(x, "bf16").view(torch.bfloat16), x.bfloat16())
    assert torch.equal(ld.encode(x, "bf16x3").view(torch.int16), ld.pairs(x, "bf16"))
    s = ld.weight_scale(x)
    assert s == 2.0 ** 17
    assert torch.equal(ld.encode(x, "f16x3", s).view(torch.int16), ld.pairs(x * s, "f16"))
    for dt in ld.DTS:
        back = ld.decode(ld.encode(x, dt), dt)
        assert (back - x).abs().max() <= x.abs().max() * (2.0 ** -8 if dt == "bf16" else 2.0 ** -16)


# ---- 2. planted faults -----------------------------------------------------------------------------------------------------
def _guarded(want):
    return torch.cat([want, torch.full((lc.GUARD,), lc.SENTINEL, dtype=torch.uint8)])


def _passes(raw, want, dt):
    lc.assert_bytes(raw, want, 0, dt, "planted")


@pytest.fixture(scope="module")
def conv():
    w = lc.distinct_values((40, 33, 3, 3), seed=6, amp=2.0 ** -4)
    return w, 40       # rotated: [33, 9, 40]; normal below: [40, 9, 40]


def test_correct_tensors_pass(conv):
    w, pad = conv
    for dt in ld.DTS:
        s = ld.weight_scale(w) if dt == "f16x3" else 1.0
        for rot in (False, True):
            want = ld.encode(ld.conv_weight(w, pad, rot), dt, s)
            _passes(_guarded(want), want, dt)


@pytest.mark.parametrize("dt", ld.DTS)
def test_taps_not_flipped_under_rot180(conv, dt):
    w, pad = conv
    want = ld.encode(ld.conv_weight(w, pad, True), dt)
    got = ld.encode(ld.conv_weight(w, pad, True).flip(1), dt)
    with pytest.raises(AssertionError, match="differ from the definition"):
        _passes(_guarded(got), want, dt)


@pytest.mark.parametrize("dt", ld.DTS)
def test_c_and_p_left_unpermuted(dt):
    w = lc.distinct_values((8, 6 * 4), seed=7, amp=2.0 ** -4)
    want = ld.encode(ld.fc_weight(w, 6, False, 24), dt)
    got = ld.encode(ld.fc_weight(w, 0, False, 24), dt)
    with pytest.raises(AssertionError, match="differ from the definition"):
        _passes(_guarded(got), want, dt)


@pytest.mark.parametrize("dt", ["bf16x3", "f16x3"])
def test_hi_and_lo_of_one_group_swapped(conv, dt):
    w, pad = conv
    want = ld.encode(ld.conv_weight(w, pad, False), dt)
    got = want.clone().view(torch.int16).reshape(-1, 16)
    got[123] = torch.cat([got[123, 8:], got[123, :8]])
    with pytest.raises(AssertionError, match=r"16 of \d+ 16-bit halves differ"):
        _passes(_guarded(got.reshape(-1).view(torch.uint8)), want, dt)


@pytest.mark.parametrize("dt", ld.DTS)
def test_one_pad_column_not_zero(conv, dt):
    w, pad = conv
    layout = ld.conv_weight(w, pad, False)
    want = ld.encode(layout, dt)
    layout[17, 4, 39] = -0.0                                    # even a negative zero in a pad column is a difference
    with pytest.raises(AssertionError, match="differ from the definition"):
        _passes(_guarded(ld.encode(layout, dt)), want, dt)


@pytest.mark.parametrize("dt", ld.DTS)
def test_one_element_beyond_the_end_written(conv, dt):
    w, pad = conv
    want = ld.encode(ld.conv_weight(w, pad, False), dt)
    raw = _guarded(want)
    raw[want.numel() + 2] = 0
    with pytest.raises(AssertionError, match="1 bytes behind the tensor were written, the first 2 bytes past its end"):
        _passes(raw, want, dt)
    raw = torch.cat([torch.full((32,), lc.SENTINEL, dtype=torch.uint8), _guarded(want)])
    raw[31] = 0
    with pytest.raises(AssertionError, match="1 bytes in front of the tensor were written"):
        lc.assert_bytes(raw, want, 32, dt, "planted")


def test_scale_off_by_one_binade(conv):
    w, pad = conv
    s = ld.weight_scale(w)
    want = ld.encode(ld.conv_weight(w, pad, False), "f16x3", s)
    for wrong in (2 * s, s / 2):
        with pytest.raises(AssertionError, match="differ from the definition"):
            _passes(_guarded(ld.encode(ld.conv_weight(w, pad, False), "f16x3", wrong)), want, "f16x3")


@pytest.mark.parametrize("dt", ld.DTS)
def test_one_32x32_tile_transposed(dt):
    w = lc.distinct_values((64, 64, 3, 3), seed=8, amp=2.0 ** -4)
    layout = ld.conv_weight(w, 64, False)                       # [co, tap, ci]
    want = ld.encode(layout, dt)
    layout[32:, 5, :32] = layout[32:, 5, :32].t().clone()
    with pytest.raises(AssertionError, match="differ from the definition"):
        _passes(_guarded(ld.encode(layout, dt)), want, dt)


def test_a_nan_matches_a_nan_of_any_payload_and_nothing_else():
    x = torch.ones(8)
    x[3] = NAN
    want = ld.encode(x, "f16x3")
    got = want.clone().view(torch.int16)
    got[3], got[11] = 0x7E01, -0x01FF                           # other payloads, one with the sign set
    _passes(_guarded(got.view(torch.uint8)), want, "f16x3")
    got[3] = 0x7C00                                             # an infinity is not a NaN
    with pytest.raises(AssertionError, match="1 of 16 16-bit halves differ"):
        _passes(_guarded(got.view(torch.uint8)), want, "f16x3")


def test_inputs_are_distinct_with_non_zero_low_halves():
    v = lc.distinct_values((1000, 32 * 49), seed=7, amp=2.0 ** -6)
    assert v.unique().numel() == v.numel() and bool((v > 0).any()) and bool((v < 0).any())
    for fmt, s in (("bf16", 1.0), ("f16", ld.weight_scale(v))):
        b = ld.pairs(v * s, fmt).reshape(-1, 16)
        assert bool(((b & 0x7FFF) != 0).all())
        if fmt == "bf16":                                       # zero or normal: no subnormal bf16 half
            assert bool((((b >> 7) & 0xFF) != 0).all())


# ---- 3. the two refusals ---------------------------------------------------------------------------------------------------
def test_cast_refuses_storage_types_it_does_not_serve(sfod):
    n = sfod.native
    lib = n.load()
    for src, dst in ((4, n.F32), (n.F32, 4), (-1, n.BF16), (n.BF16, 7), (n.BF16X3, 9)):
        assert lib.sfod_cast(None, None, 8, src, dst, None) == SFOD_EBADARG
        assert lib.sfod_last_error() == b"bad argument: cast: unknown storage type"
    for src, dst in ((n.BF16, n.BF16X3), (n.F16X3, n.BF16), (n.BF16, n.F16X3), (n.BF16X3, n.BF16)):
        assert lib.sfod_cast(None, None, 8, src, dst, None) == SFOD_EBADARG
        assert lib.sfod_last_error() == b"bad argument: cast: operand pairs convert from / to fp32 and each other only"
    # what the modules call stays served: nothing to do for an empty tensor, and no refusal
    served = [(n.F32, n.BF16), (n.BF16, n.F32), (n.F32, n.F32), (n.BF16, n.BF16), (n.F32, n.BF16X3), (n.F32, n.F16X3),
              (n.BF16X3, n.F32), (n.F16X3, n.F32), (n.BF16X3, n.BF16X3), (n.F16X3, n.F16X3), (n.F16X3, n.BF16X3), (n.BF16X3, n.F16X3)]
    for src, dst in served:
        assert lib.sfod_cast(None, None, 0, src, dst, None) == 0


def test_fc_packers_refuse_a_k_that_chw_c_does_not_divide(sfod):
    n = sfod.native
    lib = n.load()
    for k, c in ((10, 3), (1024, 48), (7, 8)):
        assert lib.sfod_pack_fc_weight_ld_ws(None, None, None, 4, k, c, 0, 1024, n.F32, None) == SFOD_EBADARG
        assert lib.sfod_last_error() == b"bad argument: pack_fc_weight: K is not a multiple of chw_c"
        assert lib.sfod_pack_fc_weight_ld(None, None, 4, k, c, 1, 8, n.BF16X3, None) == SFOD_EBADARG
        assert lib.sfod_last_error() == b"bad argument: pack_fc_weight: K is not a multiple of chw_c"
        assert lib.sfod_unpack_fc_wgrad_ld(None, None, 4, k, c, 1024, 1, None) == SFOD_EBADARG
        assert lib.sfod_last_error() == b"bad argument: unpack_fc_wgrad: K is not a multiple of chw_c"
        assert lib.sfod_unpack_fc_wgrad(None, None, 4, k, c, 0, None) == SFOD_EBADARG
