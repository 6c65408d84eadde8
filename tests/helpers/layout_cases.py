"""Inputs, guarded output buffers and the comparison of tests/test_gpu_layout_definition.py (definitions:
tests/helpers/layout_definitions.py).  tests/test_layout_definitions_host.py plants faults into correct packed tensors and
runs them through the same ``assert_bytes``, so what the GPU suite would and would not notice is itself tested without a GPU.

Inputs: every value of a tensor is distinct, so a permuted, flipped or transposed element cannot land on an equal one, and
every value keeps mantissa bits below half's 11 and bfloat16's 8, so the low half of every operand pair is non-zero and a
dropped or swapped half shows.  Magnitudes stay inside [amp / 2, 2 amp): every bf16 / half hi and lo is zero or a normal
number (half's lo may be subnormal, which the converters serve exactly; bf16 subnormals are not a property the layers depend
on and stay out).

Outputs: the destination lies inside a longer buffer filled with a sentinel byte; ``assert_bytes`` holds every byte of the
tensor to the definition, pad columns included, and every byte in front of and behind it to the sentinel.
"""
import functools

import torch

from helpers import layout_definitions as ld

SENTINEL = 0xA5                # as fp32 / bf16 / half: a small negative normal number, never +0.0 (a pad column) and no input
GUARD = 4096                   # bytes behind (and, with ``lead``, in front of) every destination
_MUL = (0x2545F5, 0x19660D, 0x3C6EF3, 0x5D588B)       # odd: multiplication is a bijection of the 23-bit mantissas


@functools.lru_cache(maxsize=8)
def _distinct_bits(n, seed):
    j = torch.arange(n, dtype=torch.int64)
    r = j >> 2
    assert n == 0 or int(r[-1]) < (1 << 22), "more values than distinct (sign, exponent, mantissa) patterns"
    combo = (j + r + seed) & 3                                       # sign and exponent: all four per group of 4 indices
    mant = ((2 * r + 1) * _MUL[seed % len(_MUL)]) & 0x7FFFFF        # odd x odd: the lowest bit is set; injective in r
    bits = ((combo & 1) << 31) | ((126 + (combo >> 1)) << 23) | mant                 # +-[0.5, 2)
    bits = bits.to(torch.int32) if n == 0 else torch.where(bits >= (1 << 31), bits - (1 << 32), bits).to(torch.int32)
    if n:
        s = bits.sort().values
        assert bool((s[1:] != s[:-1]).all()), "values are not distinct"
    return bits


def distinct_values(shape, seed=0, amp=1.0):
    """fp32 tensor of ``shape``: distinct values of magnitude [amp / 2, 2 amp) (amp a power of two), both signs, with the
    lowest mantissa bit set -- the pair formats' low halves are non-zero (asserted, for both formats, before and after the
    SFOD_F16X3 weight scale)."""
    n = 1
    for d in shape:
        n *= d
    return _distinct_flat(n, seed, float(amp)).reshape(shape).clone()


@functools.lru_cache(maxsize=4)
def _distinct_flat(n, seed, amp):
    v = _distinct_bits(n, seed).view(torch.float32) * amp
    if n:
        assert v.abs().min() >= amp / 2 and v.abs().max() < 2 * amp          # amp is a power of two: the scaling is exact
        if n % 8 == 0:
            # half pairs: activations (unscaled, amp >= 1: below, half's subnormal spacing swallows the residue) and weights
            for fmt, s in (("bf16", 1.0), ("f16", 1.0 if amp >= 1 else ld.weight_scale(v)), ("f16", ld.weight_scale(v))):
                lo = ld.pairs(v * s, fmt).reshape(-1, 16)[:, 8:]
                assert bool(((lo & 0x7FFF) != 0).all()), f"a {fmt} low half is zero"
    return v


# ---- guarded buffers -------------------------------------------------------------------------------------------------------
class Guarded:
    """``nbytes`` destination bytes at ``lead`` bytes into a sentinel-filled device buffer with GUARD bytes behind."""

    def __init__(self, nbytes, device, lead=0):
        self.nbytes, self.lead = nbytes, lead
        self.raw = torch.full((lead + nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device=device)
        self.dst = self.raw[lead:lead + nbytes]                      # contiguous: what the entry point gets

    def write(self, bytes_cpu):
        """pre-fill the destination (an accumulate target)"""
        self.dst.copy_(bytes_cpu.to(self.raw.device))

    def check(self, want, dt, label):
        assert_bytes(self.raw.cpu(), want, self.lead, dt, label)


def assert_bytes(raw, want, lead, dt, label):
    """raw: the whole guarded buffer (uint8, CPU); want: the defined bytes of the tensor at ``lead``.  Every byte of the tensor
    equals the definition (NaNs as NaNs), every other byte is still the sentinel."""
    n = want.numel()
    assert raw.numel() >= lead + n + 1, "no guard band behind the tensor"
    got = raw[lead:lead + n]
    front, behind = raw[:lead], raw[lead + n:]
    assert bool((front == SENTINEL).all()), f"{label}: {int((front != SENTINEL).sum())} bytes in front of the tensor were written"
    if not bool((behind == SENTINEL).all()):
        first = int((behind != SENTINEL).nonzero()[0])
        raise AssertionError(f"{label}: {int((behind != SENTINEL).sum())} bytes behind the tensor were written, the first "
                             f"{first} bytes past its end")
    g, w = ld.canonical(got, dt), ld.canonical(want, dt)
    if not torch.equal(g, w):
        eb = ld.ELEM_BYTES[dt] if not ld.is_pairs(dt) else 2
        bad = (g != w).reshape(-1, eb).any(dim=1).nonzero().reshape(-1)
        i = int(bad[0])
        gi, wi = g[i * eb:(i + 1) * eb].tolist(), w[i * eb:(i + 1) * eb].tolist()
        unit = "16-bit halves" if ld.is_pairs(dt) else "elements"
        raise AssertionError(f"{label}: {bad.numel()} of {n // eb} {unit} differ from the definition; the first at {i}: "
                             f"got bytes {gi}, defined {wi}")


# ---- torch storage of a definition's bytes (inputs of the casts and unpackers) ---------------------------------------------
def to_device_bytes(bytes_cpu, device, lead=0):
    """the bytes on the device, ``lead`` bytes into their allocation (an element offset inside a larger buffer)."""
    buf = torch.empty(lead + bytes_cpu.numel(), dtype=torch.uint8, device=device)
    buf[lead:].copy_(bytes_cpu.to(device))
    return buf[lead:]
