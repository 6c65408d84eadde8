"""Index definitions of the layout and conversion kernels of csrc/elementwise.hip, on the CPU and in torch only: the casts
(sfod_cast, sfod_cast_pairs_both), the per-tensor SFOD_F16X3 weight scale, the conv / fc weight packers and the weight-gradient
unpackers.  Written from the layouts documented in include/sfod_hip.h and csrc/common.h; nothing here calls the library.

Every definition returns BIT PATTERNS (or fp32 tensors whose encoding ``encode`` turns into bytes), so the GPU suite
(tests/test_gpu_layout_definition.py) compares byte for byte and there is no tolerance anywhere.  NaN is the one value whose
bits are not defined (its payload is the converter's business): ``canonical`` maps every NaN of a storage type onto one
pattern, on both sides of a comparison.

Storage types (``dt``): "fp32", "bf16", "bf16x3" (bf16 (hi, lo) pairs), "f16x3" (IEEE half (hi, lo) pairs).  A pair tensor
of n logical elements (n % 8 == 0) is n / 8 groups of 32 bytes: 8 hi then 8 lo.
"""
import torch

DTS = ("fp32", "bf16", "bf16x3", "f16x3")
PAIR_FMT = {"bf16x3": "bf16", "f16x3": "f16"}
ELEM_BYTES = {"fp32": 4, "bf16": 2, "bf16x3": 4, "f16x3": 4, "u32": 4}      # "u32": plain words (the scale word), no NaN
CHUNK = {"fp32": 4, "bf16": 8, "bf16x3": 8, "f16x3": 8}       # elements per 16-byte chunk (pairs: per 32-byte group)
_F16 = {"bf16": torch.bfloat16, "f16": torch.float16}


def is_pairs(dt):
    return dt in PAIR_FMT


# ---- pair and bf16 conversion ----------------------------------------------------------------------------------------------
def bf16(v):
    """fp32 -> bf16, round to nearest even; int16 bit patterns of the same shape."""
    return v.float().bfloat16().view(torch.int16)


def pairs(v, fmt):
    """fp32 tensor of n elements (n % 8 == 0, groups along the flat order) -> int16 [2 n] bit patterns: per 8-element group
    8 hi then 8 lo.  hi = rnd16(v), lo = rnd16(v - hi); "f16": |v| beyond 65504 (infinities too) is exactly +-65504 with
    lo = 0, NaN stays NaN in both halves."""
    v = v.float().reshape(-1)
    assert v.numel() % 8 == 0, v.numel()
    t = _F16[fmt]
    c = v.clamp(-65504.0, 65504.0) if fmt == "f16" else v          # clamp keeps NaN
    hi = c.to(t)
    lo = (c - hi.float()).to(t)
    return torch.cat([hi.view(torch.int16).reshape(-1, 8), lo.view(torch.int16).reshape(-1, 8)], dim=1).reshape(-1)


def unpairs(bits, fmt):
    """int16 [2 n] pair bit patterns -> fp32 [n]: fp32(hi) + fp32(lo), one fp32 add."""
    g = bits.reshape(-1, 16).contiguous().view(_F16[fmt]).float()
    return (g[:, :8] + g[:, 8:]).reshape(-1)


# ---- SFOD_F16X3 weight scale -----------------------------------------------------------------------------------------------
def weight_scale_bits(w):
    """the word the `_ws` packers publish: the bit pattern of max|w|, maximised as an unsigned integer -- so a NaN (whose
    pattern without the sign lies above infinity's) wins, and an all-zero tensor gives 0."""
    b = w.float().reshape(-1).contiguous().view(torch.int32) & 0x7FFFFFFF
    return int(b.max()) if b.numel() else 0


def scale_from_bits(word):
    """the power of two the packing kernels derive from the published word: biased exponent 127 + 13 - (e - 127), clamped to
    [8, 246]; 1 for a zero, subnormal (e = 0), infinite or NaN (e = 255) maximum."""
    e = (word >> 23) & 0xFF
    if e == 0 or e == 255:
        return 1.0
    se = 127 + 13 - (e - 127)
    se = min(max(se, 8), 246)
    return 2.0 ** (se - 127)


def weight_scale(w):
    return scale_from_bits(weight_scale_bits(w))


# ---- conv weights ----------------------------------------------------------------------------------------------------------
def _pad_inner(t, inner_pad):
    out = torch.zeros(*t.shape[:-1], inner_pad, dtype=torch.float32)          # pad columns: +0.0
    out[..., :t.shape[-1]] = t
    return out


def conv_weight(w, inner_pad, rot180):
    """OIHW fp32 [Cout, Cin, ks, ks] -> [Cout, taps, inner_pad], out[co][tap][ci] = w[co][ci][tap]; rot180:
    [Cin, taps, inner_pad], out[ci][tap][co] = w[co][ci][taps - 1 - tap]."""
    cout, cin = w.shape[:2]
    t = w.float().reshape(cout, cin, -1)
    if rot180:
        return _pad_inner(t.flip(2).permute(1, 2, 0), inner_pad)
    return _pad_inner(t.permute(0, 2, 1), inner_pad)


def conv_wgrad(dw_packed, cout, cin, ks):
    """packed fp32 gradient [Cout, taps, CinPad] -> OIHW: dw[co][ci][tap] = dw_packed[co][tap][ci]."""
    p = dw_packed.float().reshape(cout, ks * ks, -1)
    return p[:, :, :cin].permute(0, 2, 1).reshape(cout, cin, ks, ks).contiguous()


# ---- fc weights ------------------------------------------------------------------------------------------------------------
def fc_weight(w, chw_c, transpose, ld):
    """nn.Linear weight [N, K] -> [N, ld], out[n][p * C + c] = w[n][c * PP + p] (C = chw_c, PP = K / C; chw_c = 0: the
    identity); transpose: [K, ld], the same matrix transposed."""
    n, k = w.shape
    p = w.float()
    if chw_c > 0:
        assert k % chw_c == 0
        p = p.reshape(n, chw_c, k // chw_c).permute(0, 2, 1).reshape(n, k)
    return _pad_inner(p.t() if transpose else p, ld)


def fc_wgrad(dw_packed, n, k, chw_c, ld):
    """packed fp32 gradient [N, ld] -> [N, K]: dw[n][c * PP + p] = dw_packed[n][p * C + c]."""
    p = dw_packed.float().reshape(n, ld)[:, :k]
    if chw_c > 0:
        assert k % chw_c == 0
        p = p.reshape(n, k // chw_c, chw_c).permute(0, 2, 1).reshape(n, k)
    return p.contiguous()


# ---- output encoding -------------------------------------------------------------------------------------------------------
def encode(layout, dt, scale=1.0):
    """an fp32 tensor in its packed layout -> the bytes (uint8 [nbytes]) of its storage in ``dt``.  The packers multiply by
    the weight scale in fp32 before they round (``scale`` is 1 everywhere but for SFOD_F16X3 weights)."""
    v = layout.float().reshape(-1).contiguous()
    if scale != 1.0:
        v = v * torch.tensor(scale, dtype=torch.float32)
    if dt == "fp32":
        return v.clone().view(torch.uint8)
    if dt == "bf16":
        return bf16(v).view(torch.uint8)
    return pairs(v, PAIR_FMT[dt]).view(torch.uint8)


def decode(raw, dt):
    """the bytes of a ``dt`` tensor -> the fp32 values a kernel reads from it (pairs: fp32(hi) + fp32(lo))."""
    if dt == "fp32":
        return raw.contiguous().view(torch.float32).clone()
    if dt == "bf16":
        return raw.contiguous().view(torch.bfloat16).float()
    return unpairs(raw.contiguous().view(torch.int16), PAIR_FMT[dt])


def canonical(raw, dt):
    """bytes of a ``dt`` tensor with every NaN replaced by one pattern (a NaN's payload and sign are not defined)."""
    if dt == "u32":
        return raw.contiguous()
    if dt == "fp32":
        b = raw.contiguous().view(torch.int32).clone()
        b[(b & 0x7FFFFFFF) > 0x7F800000] = 0x7FC00000
        return b.view(torch.uint8)
    inf = 0x7C00 if dt == "f16x3" else 0x7F80
    b = raw.contiguous().view(torch.int16).clone()
    b[(b & 0x7FFF) > inf] = 0x7FFF
    return b.view(torch.uint8)
