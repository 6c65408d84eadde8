"""The layout and conversion kernels of csrc/elementwise.hip against their INDEX definitions, bit for bit: the casts
(sfod_cast, sfod_cast_pairs_both), the weight maximum and per-tensor SFOD_F16X3 scale, the conv weight packers (single and
multi), the three fc weight packers, and the conv / fc weight-gradient unpackers.

Definitions: tests/helpers/layout_definitions.py (written from include/sfod_hip.h and csrc/common.h, torch on the CPU, never
the library).  Inputs and the comparison: tests/helpers/layout_cases.py -- distinct values with non-zero low halves, the
destination inside a sentinel-filled buffer, every byte of the tensor (pad columns included) held to the definition and every
byte around it to the sentinel.  tests/test_layout_definitions_host.py plants faults into that comparison.

The tests that compare these kernels with each other (pack(dt) == cast(pack(fp32)), multi == single) stay where they are; they
cannot see an error the fp32 packing shares.  Shapes are the smallest that reach each branch; the comments say which.
"""
import pytest
import torch

from helpers import layout_cases as lc
from helpers import layout_definitions as ld

pytestmark = pytest.mark.gpu
DEV = "cuda"
CODE = {"fp32": 0, "bf16": 1, "bf16x3": 2, "f16x3": 3}          # SFOD_F32 ... SFOD_F16X3
GRID = 4096 * 256                                              # ew_grid: at most 4096 workgroups of 256 threads
INF, NAN = float("inf"), float("nan")


def _up(n, m):
    return (n + m - 1) // m * m


def _clear_saturation(native):
    """the half producers' saturation flags are process-wide: leave them cleared for whatever runs next"""
    w = torch.zeros(1, dtype=torch.int32, device=DEV)
    native.call("sfod_f16x3_poll", w)
    return int(w.item())


# ---- casts -----------------------------------------------------------------------------------------------------------------
def _check_cast(native, x, src_dt, dst_dt, lead_elems=0, label=""):
    """x fp32 (CPU, flat): stored as src_dt, converted by sfod_cast, every byte held to encode(decode(.), dst_dt)."""
    n = x.numel()
    src_bytes = ld.encode(x, src_dt)
    src = lc.to_device_bytes(src_bytes, DEV, lead_elems * ld.ELEM_BYTES[src_dt])
    want = ld.encode(ld.decode(src_bytes, src_dt), dst_dt)
    out = lc.Guarded(n * ld.ELEM_BYTES[dst_dt], DEV, lead_elems * ld.ELEM_BYTES[dst_dt])
    native.call("sfod_cast", src, out.dst, n, CODE[src_dt], CODE[dst_dt])
    out.check(want, dst_dt, f"cast {src_dt} -> {dst_dt} n={n} offset={lead_elems} {label}")


PLAIN_CASTS = [("fp32", "bf16"), ("bf16", "fp32"), ("fp32", "fp32"), ("bf16", "bf16")]
PAIR_CASTS = [("fp32", "bf16x3"), ("fp32", "f16x3"), ("bf16x3", "fp32"), ("f16x3", "fp32"), ("bf16x3", "bf16x3"),
              ("f16x3", "f16x3"), ("f16x3", "bf16x3"), ("bf16x3", "f16x3")]       # the last two: the re-split of fp32(hi + lo)


@pytest.mark.parametrize("src_dt,dst_dt", PLAIN_CASTS, ids=lambda v: v)
def test_plain_casts_match_their_definition(native, src_dt, dst_dt):
    """k_cast, the four combinations the dispatch serves.  n = 1 (one lane), 255 / 257 (one workgroup short of / one element
    past a full one), 4096 * 256 + 1 (one element past the grid cap: the stride loop's second trip); an element offset of 3
    inside a larger buffer (2- and 4-byte aligned only)."""
    for n, off in ((1, 0), (255, 0), (257, 3), (GRID + 1, 0)):
        _check_cast(native, lc.distinct_values((n,), seed=1), src_dt, dst_dt, off)


@pytest.mark.parametrize("src_dt,dst_dt", PAIR_CASTS, ids=lambda v: v)
def test_pair_casts_match_their_definition(native, src_dt, dst_dt):
    """k_cast8, all eight instantiations.  n = 8 (one group), 8 x 37 at an element offset of 8 in both buffers (32-byte-aligned
    groups that are not allocation-aligned), 8 x (4096 * 256 + 3): three groups past the grid cap, the second trip."""
    for n, off in ((8, 0), (8 * 37, 8), (8 * (GRID + 3), 0)):
        _check_cast(native, lc.distinct_values((n,), seed=2), src_dt, dst_dt, off)


def test_cast_pairs_both_matches_the_two_single_casts_definitions(native):
    """k_cast8_both: one pass, half pairs and bf16 pairs, each against the definition of its own single cast."""
    for n, off in ((8, 0), (8 * 37, 8), (8 * (GRID + 3), 0)):
        x = lc.distinct_values((n,), seed=3)
        src = lc.to_device_bytes(ld.encode(x, "fp32"), DEV, off * 4)
        h, b = lc.Guarded(n * 4, DEV, off * 4), lc.Guarded(n * 4, DEV, off * 4)
        native.call("sfod_cast_pairs_both", src, h.dst, b.dst, n)
        h.check(ld.encode(x, "f16x3"), "f16x3", f"cast_pairs_both n={n}: half pairs")
        b.check(ld.encode(x, "bf16x3"), "bf16x3", f"cast_pairs_both n={n}: bf16 pairs")


def test_casts_of_special_values(native):
    """The special values of tests/test_gpu_bf16x3.py and tests/test_gpu_f16x3.py::test_cast_*: signed zeros, 1e-30 (half: both
    halves 0), -3e38 and 70000 / -131000 / 65519.9 / infinities (half: exactly +-65504, lo 0), 65504 itself, 2^-126, 2^-20 (a
    subnormal half hi), 1 + 2^-12, NaN (stays NaN in both halves)."""
    v = torch.tensor([0.0, -0.0, 1.0, 1e-30, -3e38, 65504.0, 2.0 ** -126, 1 + 2.0 ** -12,
                      NAN, 70000.0, -131000.0, 65519.9, 2.0 ** -20, INF, -INF, -65504.0])
    for dst_dt in ("bf16x3", "f16x3", "bf16"):
        _check_cast(native, v, "fp32", dst_dt, label="special values")
    want_h = ld.decode(ld.encode(v, "f16x3"), "f16x3")
    assert want_h[4] == -65504.0 and want_h[9] == 65504.0 and want_h[10] == -65504.0 and want_h[11] == 65504.0
    assert want_h[13] == 65504.0 and want_h[14] == -65504.0 and torch.isnan(want_h[8])       # the definition saturates as documented
    for src_dt, dst_dt in (("f16x3", "fp32"), ("bf16x3", "fp32"), ("f16x3", "bf16x3"), ("f16x3", "f16x3"), ("bf16x3", "bf16x3")):
        _check_cast(native, v, src_dt, dst_dt, label="special values")
    h, b = lc.Guarded(16 * 4, DEV), lc.Guarded(16 * 4, DEV)
    native.call("sfod_cast_pairs_both", v.to(DEV), h.dst, b.dst, 16)
    h.check(ld.encode(v, "f16x3"), "f16x3", "cast_pairs_both special values: half pairs")
    b.check(ld.encode(v, "bf16x3"), "bf16x3", "cast_pairs_both special values: bf16 pairs")
    _clear_saturation(native)


def test_saturation_word_rises_exactly_for_values_beyond_halfs_range(native):
    """sfod_f16x3_poll after a cast to half pairs: raised by a finite or infinite value beyond +-65504, not by NaN, not by
    +-65504 itself; the poll clears it."""
    above = torch.nextafter(torch.tensor(65504.0), torch.tensor(INF)).item()

    def polled(values):
        x = torch.ones(8)
        x[:len(values)] = torch.tensor(values)
        _check_cast(native, x, "fp32", "f16x3", label=f"saturation {values}")
        return _clear_saturation(native)

    _clear_saturation(native)                                   # whatever ran before
    assert polled([65504.0, -65504.0, NAN, 0.0, 1e-30]) == 0
    for v in (above, -above, 70000.0, -3e38, INF, -INF):
        assert polled([v]) == 1, v
        assert _clear_saturation(native) == 0, "the poll did not clear the flag"
    assert polled([NAN, 65504.0]) == 0


# ---- weight maximum and scale ----------------------------------------------------------------------------------------------
def _pack_fc(native, w_dev, w, chw_c, transpose, ldim, dt, label):
    """sfod_pack_fc_weight_ld_ws of w [N, K] (w_dev: the same values on the device) against fc_weight; SFOD_F16X3 goes with
    its scale word, as every module packs it.  -> the guarded output."""
    n, k = w.shape
    rows = k if transpose else n
    out = lc.Guarded(rows * ldim * ld.ELEM_BYTES[dt], DEV)
    word = lc.Guarded(4, DEV) if dt == "f16x3" else None
    native.call("sfod_pack_fc_weight_ld_ws", w_dev, out.dst, word.dst if word else None, n, k, chw_c, int(transpose), ldim,
                CODE[dt])
    scale = 1.0
    if word is not None:
        word.check(torch.tensor([ld.weight_scale_bits(w)], dtype=torch.int32).view(torch.uint8), "u32", f"{label}: scale word")
        scale = ld.weight_scale(w)
    out.check(ld.encode(ld.fc_weight(w, chw_c, transpose, ldim), dt, scale), dt, label)
    return out


def _at_offset(w_flat, words):
    """the values on the device, starting 4 * words bytes past a 16-byte boundary (a view into a flat parameter buffer)"""
    buf = torch.empty(w_flat.numel() + 4, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[words:words + w_flat.numel()]
    view.copy_(w_flat.to(DEV))
    return view


def _absmax_cases():
    base = lambda n, s=0: lc.distinct_values((n,), seed=s, amp=2.0 ** -5)          # |w| in [2^-6, 2^-4)
    cases = []
    # the unaligned path: tensors 4, 8, 12 bytes past a 16-byte boundary, the maximum in the last element
    for words in (1, 2, 3):
        w = base(1203)
        w[-1] = 0.3
        cases.append((f"{4 * words} bytes past alignment", w, words))
    # the aligned path: count % 4 = 1, 2, 3 with the maximum in the scalar tail (its first and its last element), and
    # count % 4 = 0 with the maximum in the last element of the last 16-byte load
    for count, at in ((1201, -1), (1202, -2), (1203, -1), (1203, -3), (1200, -1)):
        w = base(count, 1)
        w[at] = -0.3 if count == 1202 else 0.3                                   # one of them negative
        cases.append((f"aligned count={count} max at {at}", w, 0))
    w = base(3)                                                                  # nothing but a tail
    cases.append(("aligned count=3", w, 0))
    # several workgroups and several trips of each lane: the maximum in the tail
    w = base(256 * 64 * 3 + 2, 2)
    w[-1] = -0.25
    cases.append(("count=49154 over 4 workgroups", w, 0))
    # a power of two and the value just below it: one binade apart
    for m, name in ((0.125, "2^-3"), (torch.nextafter(torch.tensor(0.125), torch.tensor(0.0)).item(), "just below 2^-3")):
        w = base(40)
        w[17] = m
        cases.append((f"maximum {name}", w, 0))
    # the clamp: 2^-120 asks for a biased exponent of 260 and gets 246; 2^120 asks for 20 (the lower clamp, 8, is beyond
    # what a finite maximum can ask for)
    w = lc.distinct_values((40,), seed=3) * 2.0 ** -122
    w[5] = 2.0 ** -120
    cases.append(("maximum 2^-120", w, 0))
    w = lc.distinct_values((40,), seed=3) * 2.0 ** 118
    w[5] = -2.0 ** 120
    cases.append(("maximum -2^120", w, 0))
    # unscaled: a subnormal maximum, all zeros (one of them negative), one infinity, one NaN
    cases.append(("subnormal maximum", lc.distinct_values((40,), seed=3) * 2.0 ** -140, 0))
    w = torch.zeros(40)
    w[3] = -0.0
    cases.append(("all zero", w, 0))
    for v in (INF, -INF, NAN):
        w = base(40)
        w[11] = v
        cases.append((f"one {v}", w, 0))
    return cases


def test_weight_maximum_and_scale_of_one_tensor(native):
    """k_weight_absmax through sfod_pack_fc_weight_ld_ws: the published word is the bit pattern of max|w| and the packed half
    pairs are those of w * s, s the power of two of that word."""
    seen = set()
    _clear_saturation(native)
    for name, w, words in _absmax_cases():
        count = w.numel()
        _pack_fc(native, _at_offset(w, words).view(1, count), w.view(1, count), 0, False, _up(count, 8), "f16x3",
                 f"weight scale, {name}")
        seen.add(ld.weight_scale(w))
    assert {2.0 ** 15, 2.0 ** 16, 2.0 ** 119, 2.0 ** -107, 1.0} <= seen, seen      # the cases are the ones they claim to be
    assert _clear_saturation(native) == 1                                         # the infinities, unscaled, were clamped


def _pack_multi(native, entries, dt, label):
    """sfod_pack_conv_weights_multi_ws over entries [(w OIHW CPU, inner_pad, rot180)]: sources at odd 4-byte offsets of one
    flat buffer, destinations 256-byte aligned in one sentinel-filled buffer, so the gaps between them are guard bands."""
    eb = ld.ELEM_BYTES[dt]
    flat = torch.empty(sum(w.numel() + 8 for w, _, _ in entries), dtype=torch.float32, device=DEV)
    assert flat.data_ptr() % 16 == 0
    rows, first, src_off, dst_off, want = [], 0, 0, 0, []
    sizes = []
    for w, pad, rot in entries:
        cout, cin, ks, _ = w.shape
        sizes.append(((cin if rot else cout) * ks * ks * pad * eb, dst_off))
        dst_off += _up(sizes[-1][0] + 64, 256)                       # at least 64 sentinel bytes between two tensors
    out = lc.Guarded(dst_off, DEV)
    amax = lc.Guarded(4 * len(entries), DEV) if dt == "f16x3" else None
    expect = torch.full((dst_off,), lc.SENTINEL, dtype=torch.uint8)
    for i, ((w, pad, rot), (nbytes, off)) in enumerate(zip(entries, sizes)):
        cout, cin, ks, _ = w.shape
        src_off = _up(src_off, 4) + (i + 1) % 4                      # entry i: 4 * ((i + 1) % 4) bytes past a 16-byte boundary
        src = flat[src_off:src_off + w.numel()]
        src.copy_(w.reshape(-1).to(DEV))
        src_off += w.numel()
        rows.append([src.data_ptr(), out.dst.data_ptr() + off, cout, cin, ks, pad, int(rot), first])
        first += native.query("sfod_pack_conv_weights_blocks", cout, cin, ks, pad, int(rot))
        scale = ld.weight_scale(w) if dt == "f16x3" else 1.0
        expect[off:off + nbytes] = ld.encode(ld.conv_weight(w, pad, rot), dt, scale)
        want.append(ld.weight_scale_bits(w))
    rows.append([0, 0, 0, 0, 0, 0, 0, first])
    desc = torch.tensor(rows, dtype=torch.int64).to(DEV)
    native.call("sfod_pack_conv_weights_multi_ws", desc, len(entries), first, CODE[dt], amax.dst if amax else None)
    if amax is not None:
        amax.check(torch.tensor(want, dtype=torch.int32).view(torch.uint8), "u32", f"{label}: scale words")
    out.check(expect, dt, label)
    return out, sizes


def test_weight_maximum_and_scale_per_entry_of_a_table(native):
    """k_weight_absmax over a table (blockIdx.y = entry; sources 4, 8, 12, 0, 4 bytes past a 16-byte boundary): five entries of
    very different magnitudes each get their own word and scale."""
    amps = (2.0 ** -20, 2.0 ** 3, 2.0 ** -5, 2.0 ** 30, 2.0 ** -1)
    shapes = ((5, 3, 3), (8, 8, 1), (33, 7, 3), (3, 5, 1), (40, 9, 3))              # counts 135, 64, 2079, 15, 3240
    entries = [(lc.distinct_values((co, ci, ks, ks), seed=i, amp=a), _up(ci, 8), False)
               for i, ((co, ci, ks), a) in enumerate(zip(shapes, amps))]
    assert len({ld.weight_scale(w) for w, _, _ in entries}) == 5
    _pack_multi(native, entries, "f16x3", "five magnitudes")


# ---- conv weight packers ---------------------------------------------------------------------------------------------------
# (Cout, Cin, inner_pad or None = rounded up to the chunk) against PACK_T = 32, the multi kernel's tile
CONV_SHAPES = [
    (33, 31, None),      # ragged tiles in both directions: one channel past a tile, one short of one
    (64, 3, 8),          # the first layer: 3 channels padded to 8
    (257, 33, None),     # nine row tiles, the last with one row; a second inner tile with one channel
    (40, 8, 72),         # a pad wider than a tile: whole tiles of nothing but pad columns
]


def _conv_pad(cout, cin, pad, rot, dt):
    inner = _up(cout if rot else cin, ld.CHUNK[dt])
    return inner if pad is None else max(pad, inner)


def _pack_conv(native, w, pad, rot, dt, label):
    cout, cin, ks, _ = w.shape
    out = lc.Guarded((cin if rot else cout) * ks * ks * pad * ld.ELEM_BYTES[dt], DEV)
    word = lc.Guarded(4, DEV) if dt == "f16x3" else None
    native.call("sfod_pack_conv_weight_ws", w.to(DEV), out.dst, word.dst if word else None, cout, cin, ks, pad, int(rot),
                CODE[dt])
    scale = 1.0
    if word is not None:
        word.check(torch.tensor([ld.weight_scale_bits(w)], dtype=torch.int32).view(torch.uint8), "u32", f"{label}: scale word")
        scale = ld.weight_scale(w)
    out.check(ld.encode(ld.conv_weight(w, pad, rot), dt, scale), dt, label)
    return out


def _unpack_conv_round_trip(native, packed, w, pad, label):
    """unpack(pack_F32(w)) == w: nothing is lost and nothing moves"""
    cout, cin, ks, _ = w.shape
    back = lc.Guarded(w.numel() * 4, DEV)
    native.call("sfod_unpack_conv_wgrad", packed.dst, back.dst, cout, cin, ks, pad, 0)
    back.check(ld.encode(w, "fp32"), "fp32", f"{label}: round trip")


@pytest.mark.parametrize("dt", ld.DTS)
def test_conv_weight_packer_matches_its_definition(native, dt):
    """k_pack_conv_weight: kernel sizes 1, 3, 7, both orientations, every storage type, the shapes above."""
    for ks in (1, 3, 7):
        for cout, cin, pad0 in CONV_SHAPES:
            w = lc.distinct_values((cout, cin, ks, ks), seed=ks, amp=2.0 ** -4)
            for rot in (False, True):
                pad = _conv_pad(cout, cin, pad0, rot, dt)
                out = _pack_conv(native, w, pad, rot, dt, f"pack_conv {dt} {cout}x{cin}x{ks} pad={pad} rot={int(rot)}")
                if dt == "fp32" and not rot:
                    _unpack_conv_round_trip(native, out, w, pad, f"conv {cout}x{cin}x{ks} pad={pad}")


@pytest.mark.parametrize("rot", [False, True])
def test_conv_weight_packer_beyond_the_grid_cap(native, rot):
    """k_pack_conv_weight with 130 x 49 x 168 = 1 070 160 packed elements (rotated: 168 x 49 x 136): more than 4096 x 256, the
    stride loop's second trip."""
    w = lc.distinct_values((130, 168, 7, 7), seed=5, amp=2.0 ** -4)
    pad = 136 if rot else 168
    assert (168 if rot else 130) * 49 * pad > GRID
    out = _pack_conv(native, w, pad, rot, "fp32", f"pack_conv fp32 130x168x7 rot={int(rot)}")
    if not rot:
        _unpack_conv_round_trip(native, out, w, pad, "conv 130x168x7")             # 1 070 160 elements: the unpacker's too


def _multi_table():
    """44 entries, tensors of one workgroup and of many interleaved (first_block grows unevenly: the binary search takes up
    to six steps and lands on first, middle and last entries), kernel sizes 1 and 3, both orientations, all CONV_SHAPES."""
    small = [(8, 8, 1), (16, 3, 3), (32, 32, 3), (5, 24, 1), (31, 7, 3), (1, 1, 1)]                 # one workgroup each
    big = [(257, 33, 3), (33, 31, 3), (130, 70, 1), (64, 3, 3), (40, 8, 1), (257, 160, 3), (257, 33, 1)]
    shapes = []
    for i in range(22):
        shapes.append(small[i % len(small)] + (None,))
        shapes.append(big[i % len(big)] + (72 if big[i % len(big)][:2] == (40, 8) else None,))
    return shapes


@pytest.mark.parametrize("dt", ld.DTS)
def test_conv_weights_multi_packer_matches_its_definition(native, dt):
    """k_pack_conv_weights_multi against conv_weight (not against the single packer), with the bytes between the packed
    tensors held to the sentinel: a workgroup that picked the wrong entry or tile writes somewhere it should not."""
    entries = []
    for i, (cout, cin, ks, pad0) in enumerate(_multi_table()):
        rot = i % 4 >= 2
        w = lc.distinct_values((cout, cin, ks, ks), seed=i, amp=2.0 ** (-(i % 11) - 1))
        entries.append((w, _conv_pad(cout, cin, pad0, rot, dt), rot))
    assert len(entries) >= 40
    blocks = [native.query("sfod_pack_conv_weights_blocks", w.shape[0], w.shape[1], w.shape[2], p, int(r)) for w, p, r in entries]
    assert min(blocks) == 1 and max(blocks) >= 40
    _pack_multi(native, entries, dt, f"pack_multi {dt}")


# ---- fc weight packers -----------------------------------------------------------------------------------------------------
# the LDS-tiled kernels take N * K >= 2^20 with PP = K / C <= 64 and an unpadded ld; tiles: 64 channels (k_pack_fc_chw,
# k_unpack_fc_chw), 64 rows x 4 channels (k_pack_fc_chw_t)
TILED = [
    (1000, 32, 49),      # C below one 64-channel tile (cw = 32); N % 64 = 40 (nw = 40 in the last row tile)
    (1024, 72, 16),      # C % 64 = 8: a second channel tile of 8
    (1024, 1024, 1),     # PP = 1: the permutation is the identity, every run has one element
    (328, 64, 64),       # PP = 64, N % 64 = 8: the largest tile, 64 * (4 * 64 + 1) * 4 = 65 792 bytes of LDS transposed
    (1024, 22, 49),      # C % 4 = 2 (cw = 2 in the transposed kernel's last tile); K % 8 != 0: fp32 and bf16 only
]
TILED_CASES = [pytest.param(s, dt, id=f"{'x'.join(map(str, s))}-{dt}") for s in TILED for dt in ld.DTS
               if not (ld.is_pairs(dt) and (s[1] * s[2]) % 8)]


def _unpack_fc_round_trip(native, packed, w, chw_c, ldim, label):
    n, k = w.shape
    back = lc.Guarded(w.numel() * 4, DEV)
    native.call("sfod_unpack_fc_wgrad_ld", packed.dst, back.dst, n, k, chw_c, ldim, 0)
    back.check(ld.encode(w, "fp32"), "fp32", f"{label}: round trip")


@pytest.mark.parametrize("shape,dt", TILED_CASES)
def test_tiled_fc_weight_packers_match_their_definition(native, shape, dt):
    """k_pack_fc_chw and k_pack_fc_chw_t at every partial tile extent, every storage type."""
    n, c, pp = shape
    assert n * c * pp >= 1 << 20 and pp <= 64
    w = lc.distinct_values((n, c * pp), seed=7, amp=2.0 ** -6)
    wd = w.to(DEV)
    for transpose in (False, True):
        ldim = n if transpose else c * pp
        out = _pack_fc(native, wd, w, c, transpose, ldim, dt, f"pack_fc tiled {dt} N={n} C={c} PP={pp} transpose={int(transpose)}")
        if dt == "fp32" and not transpose:
            _unpack_fc_round_trip(native, out, w, c, ldim, f"fc tiled N={n} C={c} PP={pp}")


@pytest.mark.parametrize("dt", ld.DTS)
def test_flat_fc_weight_packer_matches_its_definition(native, dt):
    """k_pack_fc_weight: without and with the (c, p) permutation, both orientations, ld equal to the inner size and padded
    (the 41 predictor outputs of a 1024-wide head to 48; K = 392 to 400)."""
    for n, k, c in ((41, 1024, 0), (41, 1024, 64), (24, 392, 8), (1, 8, 8)):
        w = lc.distinct_values((n, k), seed=8, amp=2.0 ** -6)
        wd = w.to(DEV)
        for transpose in (False, True):
            inner = n if transpose else k
            for ldim in (_up(inner, 8), _up(inner, 8) + 8):
                out = _pack_fc(native, wd, w, c, transpose, ldim, dt,
                               f"pack_fc flat {dt} N={n} K={k} chw_c={c} transpose={int(transpose)} ld={ldim}")
                if dt == "fp32" and not transpose:
                    _unpack_fc_round_trip(native, out, w, c, ldim, f"fc flat N={n} K={k} chw_c={c} ld={ldim}")


@pytest.mark.parametrize("dt", ld.DTS)
def test_fc_weight_packers_on_both_sides_of_the_tiling_threshold(native, dt):
    """(C, PP) = (64, 16): N = 1023 gives N * K = 2^20 - 1024 (flat kernel), N = 1024 exactly 2^20 (tiled kernels); a padded ld
    keeps N = 1024 on the flat kernel.  All of them give the defined bits."""
    for n, pad in ((1023, 0), (1024, 0), (1024, 8)):
        w = lc.distinct_values((n, 1024), seed=9, amp=2.0 ** -6)
        wd = w.to(DEV)
        for transpose in (False, True):
            ldim = _up(n if transpose else 1024, 8) + pad
            _pack_fc(native, wd, w, 64, transpose, ldim, dt, f"pack_fc threshold {dt} N={n} transpose={int(transpose)} ld={ldim}")


@pytest.mark.parametrize("chw_c", [0, 8])
def test_flat_fc_weight_packer_beyond_the_grid_cap(native, chw_c):
    """k_pack_fc_weight with 1025 x 1024 packed elements, 1024 past 4096 x 256.  chw_c = 0 never takes the tiled kernels;
    chw_c = 8 gives PP = 128 > 64, the permutation on the flat kernel."""
    w = lc.distinct_values((1025, 1024), seed=10, amp=2.0 ** -6)
    wd = w.to(DEV)
    for transpose in (False, True):
        ldim = 1032 if transpose else 1024
        out = _pack_fc(native, wd, w, chw_c, transpose, ldim, "fp32", f"pack_fc flat fp32 1025x1024 chw_c={chw_c} transpose={int(transpose)}")
        if not transpose:
            _unpack_fc_round_trip(native, out, w, chw_c, ldim, f"fc flat 1025x1024 chw_c={chw_c}")       # the flat unpacker's second trip


# ---- unpackers -------------------------------------------------------------------------------------------------------------
def _check_unpack(native, name, dwp, args, want, label):
    """accumulate = 0 over a sentinel-filled destination and accumulate = 1 onto a non-zero one (one fp32 add)"""
    dwp_dev = dwp.to(DEV)
    out = lc.Guarded(want.numel() * 4, DEV)
    native.call(name, dwp_dev, out.dst, *args, 0)
    out.check(ld.encode(want, "fp32"), "fp32", f"{label} accumulate=0")
    before = lc.distinct_values(tuple(want.shape), seed=11, amp=2.0 ** -3)
    out.write(ld.encode(before, "fp32"))
    native.call(name, dwp_dev, out.dst, *args, 1)
    out.check(ld.encode(before + want, "fp32"), "fp32", f"{label} accumulate=1")


def test_conv_wgrad_unpacker_matches_its_definition(native):
    """k_unpack_conv_wgrad: kernel sizes 1, 3, 7 with CinPad > Cin (the pad columns hold values that must not arrive)."""
    for ks in (1, 3, 7):
        for cout, cin, pad in ((33, 31, 32), (64, 3, 8), (40, 8, 72), (5, 8, 8)):
            dwp = lc.distinct_values((cout, ks * ks, pad), seed=12)
            _check_unpack(native, "sfod_unpack_conv_wgrad", dwp, (cout, cin, ks, pad), ld.conv_wgrad(dwp, cout, cin, ks),
                          f"unpack_conv {cout}x{cin}x{ks} pad={pad}")


def test_conv_wgrad_unpacker_beyond_the_grid_cap(native):
    """130 x 168 x 49 = 1 070 160 gradient elements from a CinPad of 176: the stride loop's second trip, accumulating too."""
    dwp = lc.distinct_values((130, 49, 176), seed=13)
    _check_unpack(native, "sfod_unpack_conv_wgrad", dwp, (130, 168, 7, 176), ld.conv_wgrad(dwp, 130, 168, 7), "unpack_conv 130x168x7")


@pytest.mark.parametrize("shape", TILED, ids=lambda s: "x".join(map(str, s)))
def test_tiled_fc_wgrad_unpacker_matches_its_definition(native, shape):
    """k_unpack_fc_chw at every partial channel tile, with ld = K and ld > K -- a combination the pack side never takes on
    its tiled kernels but this side does."""
    n, c, pp = shape
    k = c * pp
    for ldim in (k, k + 8):
        dwp = lc.distinct_values((n, ldim), seed=14)
        _check_unpack(native, "sfod_unpack_fc_wgrad_ld", dwp, (n, k, c, ldim), ld.fc_wgrad(dwp, n, k, c, ldim),
                      f"unpack_fc tiled N={n} C={c} PP={pp} ld={ldim}")


def test_flat_fc_wgrad_unpacker_matches_its_definition(native):
    """k_unpack_fc_wgrad: without and with the permutation, ld = K and larger; N = 1023 at (C, PP) = (64, 16) is the last size
    below the tiling threshold, N = 1024 (the tiled kernel) the first above."""
    for n, k, c in ((41, 1024, 0), (41, 1024, 64), (24, 392, 8), (1, 8, 8), (1023, 1024, 64), (1024, 1024, 64)):
        for ldim in (k, k + 8):
            dwp = lc.distinct_values((n, ldim), seed=15)
            _check_unpack(native, "sfod_unpack_fc_wgrad_ld", dwp, (n, k, c, ldim), ld.fc_wgrad(dwp, n, k, c, ldim),
                          f"unpack_fc flat N={n} K={k} chw_c={c} ld={ldim}")


@pytest.mark.parametrize("chw_c", [0, 8])
def test_flat_fc_wgrad_unpacker_beyond_the_grid_cap(native, chw_c):
    """1025 x 1024 gradient elements (chw_c = 8: PP = 128, the permutation on the flat kernel), ld = 1032, accumulating too."""
    dwp = lc.distinct_values((1025, 1032), seed=16)
    _check_unpack(native, "sfod_unpack_fc_wgrad_ld", dwp, (1025, 1024, chw_c, 1032), ld.fc_wgrad(dwp, 1025, 1024, chw_c, 1032),
                  f"unpack_fc flat 1025x1024 chw_c={chw_c}")
