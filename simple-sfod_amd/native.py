"""ctypes binding of ``libsfod_hip.so`` (the C-ABI drop-in boundary, ``include/sfod_hip.h``).

The prototypes are parsed from the header itself, so Python argument types can never drift
from the declared C ABI.  There is NO CPU fallback: if the library is missing or fails to
load, importing any compute entry point raises -- the product path fails loudly.

PyTorch is used here only as the owner of device memory and streams (``tensor.data_ptr()``,
``torch.cuda.current_stream()``).
"""
import collections
import ctypes
import math
import os
import re
import warnings

import torch

# SFOD_BF16X3 tensors are tagged with torch.complex32 (see SPLIT_DTYPE below); torch only ever allocates / views them
warnings.filterwarnings("ignore", message="ComplexHalf support is experimental")

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(_HERE), "include", "sfod_hip.h")
SO_PATH = os.environ.get("SFOD_HIP_LIB", os.path.join(_HERE, "lib", "libsfod_hip.so"))   # override: kernel A/B builds

F32, BF16, BF16X3, F16X3 = 0, 1, 2, 3

# Storage tag of SFOD_BF16X3 ("split") tensors (include/sfod_hip.h): 4 bytes per logical element -- a (hi, lo) bf16
# pair, stored per 8 channels as 8 hi then 8 lo.  torch never does arithmetic on them (only empty / zeros / view /
# permute); torch.complex32 is used purely as a 4-byte dtype that cannot be confused with fp32 data, so tensor
# shapes stay the LOGICAL shapes and every wrapper below dispatches on ``dt_of(t)``.  Conversions go through
# ``cast`` (sfod_cast), never through ``Tensor.to``.
SPLIT_DTYPE = torch.complex32
# SFOD_F16X3 tensors -- the same storage with IEEE half pairs -- carry their own 4-byte tag, so that a tensor of one pair
# format can never reach a kernel instantiated for the other (the weight-gradient entry points reject SFOD_F16X3).
SPLITH_DTYPE = torch.uint32
PAIR_DTYPES = (SPLIT_DTYPE, SPLITH_DTYPE)

# cfg.SFOD.COMPUTE_DTYPE -> operand type of the FORWARD products.  "f16x3": forward products on half pairs (22-bit
# operands; activations and weights sit inside half's exponent range), backward products (data and weight gradients:
# tiny values, no loss scaling) on bf16 pairs -- ``grad_dtype_of``.
COMPUTE_MODES = {"fp32": F32, "bf16": BF16, "bf16x3": BF16X3, "f16x3": F16X3}


def mode_dt(name):
    """cfg.SFOD.COMPUTE_DTYPE -> dt code of the MFMA operands."""
    try:
        return COMPUTE_MODES[str(name).lower()]
    except KeyError:
        raise ValueError(f"SFOD.COMPUTE_DTYPE must be one of {sorted(COMPUTE_MODES)}, got {name!r}") from None


def mode_dtype(name):
    """cfg.SFOD.COMPUTE_DTYPE -> torch dtype of the MFMA operand tensors (activations fed to conv / GEMM, weights)."""
    return torch_dtype(mode_dt(name))


def out_dtype_of(dtype):
    """dtype convolutions / GEMMs write (and elementwise gradients flow in) for operands of ``dtype``."""
    return torch.float32 if dtype in PAIR_DTYPES else dtype


def grad_dtype_of(dtype):
    """operand dtype of the BACKWARD products (data gradient, weight gradient) of a model whose forward operands are
    ``dtype``: half pairs hold activations and weights, not gradients (range) -> bf16 pairs."""
    return SPLIT_DTYPE if dtype == SPLITH_DTYPE else dtype


def is_pairs(dtype):
    return dtype in PAIR_DTYPES


class NativeLibraryError(RuntimeError):
    pass


def parse_header(path=HEADER):
    """-> {name: (restype, [argtypes])} for every function declared in the header."""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    protos = {}
    for m in re.finditer(r"(const\s+char\s*\*|int64_t|int)\s+(sfod_\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        ret, name, args = m.group(1), m.group(2), m.group(3)
        restype = ctypes.c_char_p if "char" in ret else (ctypes.c_int64 if ret == "int64_t" else ctypes.c_int)
        argtypes = []
        args = args.strip()
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                if "*" in a:
                    argtypes.append(ctypes.c_void_p)
                elif a.startswith("int64_t"):
                    argtypes.append(ctypes.c_int64)
                elif a.startswith("float"):
                    argtypes.append(ctypes.c_float)
                elif a.startswith("double"):
                    argtypes.append(ctypes.c_double)
                elif a.startswith("int") or a.startswith("int32_t"):
                    argtypes.append(ctypes.c_int)
                else:
                    raise NativeLibraryError(f"cannot map C parameter '{a}' of {name}")
        protos[name] = (restype, argtypes)
    return protos


_lib = None
_protos = None


def load(path=SO_PATH):
    """Load the shared library and bind every symbol the header declares."""
    global _lib, _protos
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise NativeLibraryError(
            f"{path} not found: build it with `python {os.path.join(_HERE, 'csrc', 'build.py')}` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the hot path.")
    lib = ctypes.CDLL(path)
    protos = parse_header()
    for name, (restype, argtypes) in protos.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise NativeLibraryError(f"{path} does not export {name} declared in {HEADER}") from e
        fn.restype = restype
        fn.argtypes = argtypes
    _lib, _protos = lib, protos
    return lib


def exported_symbols():
    load()
    return sorted(_protos)


def _chk(rc, name):
    if rc != 0:
        msg = _lib.sfod_last_error().decode()
        raise NativeLibraryError(f"{name} failed with code {rc}: {msg}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    # torch.cuda.current_stream() costs ~8 us of Python per call; the raw getter is a single C call
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    if t is None:
        return None
    assert t.is_cuda, "native ops need device tensors"
    assert t.is_contiguous(), "native ops need contiguous tensors"
    return t.data_ptr()


def dt_of(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == SPLIT_DTYPE:
        return BF16X3
    if t.dtype == SPLITH_DTYPE:
        return F16X3
    raise TypeError(f"unsupported dtype {t.dtype}")


def dt_of_dtype(dtype):
    return {torch.float32: F32, torch.bfloat16: BF16, SPLIT_DTYPE: BF16X3, SPLITH_DTYPE: F16X3}[dtype]


def torch_dtype(dt):
    return {F32: torch.float32, BF16: torch.bfloat16, BF16X3: SPLIT_DTYPE, F16X3: SPLITH_DTYPE}[dt]


def chunk_elems(dt):
    """channel granularity of a tensor of storage type dt (one 16-byte chunk; bf16x3: one 32-byte (hi | lo) group)"""
    return 4 if dt == F32 else 8


def nhwc_operand(x_nchw, dtype):
    """NCHW-shaped view of NHWC memory (what the backbones return) -> contiguous NHWC MFMA operand of ``dtype``."""
    p = x_nchw.permute(0, 2, 3, 1)
    if p.dtype == dtype:
        return p.contiguous()
    if dtype in PAIR_DTYPES or p.dtype in PAIR_DTYPES:
        return cast(p.contiguous(), dtype)
    return p.to(dtype).contiguous()


def as_operand(t, dtype):
    """t as an MFMA operand of ``dtype``: unchanged if it already is, else converted by sfod_cast (fp32 -> bf16 /
    operand pairs; half pairs -> bf16 pairs for a weight gradient whose producer did not write both).  The trunk's
    producers write operand tensors directly; the heads' small fp32 tensors pass here."""
    return t if t.dtype == dtype else cast(t, dtype)


def conv3x3_channels(c, dt):
    """the channel count the 3x3 convolution kernels take for a ``c``-channel input of storage type dt: whole chunks, a power
    of two of them (gemm_conv.hip: ``Cin / chunk`` is a shift in the k loop)"""
    e = chunk_elems(dt)
    n = max((c + e - 1) // e, 1)
    return e << (n - 1).bit_length()


def pad_channels(x, cp):
    """x [..., C] -> [..., cp] with zero channels behind (a copy; x itself when cp == C).  Pair tensors are moved as their
    4-byte storage: 8-channel groups stay whole because C and cp are multiples of 8."""
    c = x.shape[-1]
    if cp == c:
        return x
    raw = torch.int32 if x.dtype in PAIR_DTYPES else x.dtype
    out = torch.zeros(*x.shape[:-1], cp, dtype=raw, device=x.device)
    out[..., :c] = x.view(raw)
    return out.view(x.dtype)


def operands_for(t, dtype, need_grad):
    """fp32 ``t`` -> (forward operand of ``dtype``, the operand the weight gradient will read or None).  One pass over
    ``t`` also when the two differ ("f16x3": half pairs + bf16 pairs)."""
    gdt = grad_dtype_of(dtype)
    if not need_grad:
        return as_operand(t, dtype), None
    if gdt == dtype:
        op = as_operand(t, dtype)
        return op, op
    if t.dtype == torch.float32 and dtype == SPLITH_DTYPE and gdt == SPLIT_DTYPE:
        t = t.contiguous()
        a = torch.empty(t.shape, dtype=SPLITH_DTYPE, device=t.device)
        b = torch.empty(t.shape, dtype=SPLIT_DTYPE, device=t.device)
        call("sfod_cast_pairs_both", t, a, b, t.numel())
        return a, b
    return as_operand(t, dtype), as_operand(t, gdt)


class _Everything:
    def __contains__(self, item):
        return True


class KernelTimer:
    """Optional per-entry-point timing with HIP events recorded on the launch stream (used by
    bench.py for the roofline figure of the dominant kernels).  ``flops`` is the algorithmic work
    of the launch (2 x MACs of the GEMM the entry point computes)."""

    def __init__(self, watch=("sfod_conv_fwd", "sfod_conv_wgrad", "sfod_conv_wgrad_oihw")):
        # entry points; records are keyed "<entry>[:<kernel tag>]".  watch=None: EVERY entry point (bench.py's
        # `native_kernel_time` figure: how much of a step's wall time the library's own launches cover)
        self.watch = _Everything() if watch is None else set(watch)
        self.records = []      # (name, flops, start_event, end_event)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, flops, a, b in self.records:
            d = out.setdefault(name, {"launches": 0, "ms": 0.0, "flops": 0.0})
            d["launches"] += 1
            d["ms"] += a.elapsed_time(b)
            d["flops"] += flops
        return out


_timer = None


def set_timer(timer):
    global _timer
    _timer = timer


def call(name, *args, timer_name=None, flops=0.0, tag=""):
    """Raw call: tensors are converted to device pointers, the current stream is appended.  ``timer_name``: the entry
    point a KernelTimer files this launch under (sfod_conv_dgrad_bnred runs the sfod_conv_fwd kernel family), as
    "<entry><tag>" with ``flops``, the algorithmic work of THIS launch."""
    lib = load()
    conv = [(_p(a) if isinstance(a, torch.Tensor) else a) for a in args]
    if _timer is not None and (timer_name or name) in _timer.watch:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = getattr(lib, name)(*conv, _stream())
        b.record()
        _timer.records.append(((timer_name or name) + tag, flops, a, b))
    else:
        rc = getattr(lib, name)(*conv, _stream())
    _chk(rc, name)


def query(name, *args):
    return getattr(load(), name)(*args)


def set_conv_algo(algo):
    """0 auto, 1 generic implicit GEMM, 2 halo-patch kernel whenever the shape allows (3x3 bf16); 3 / 4 auto, but the generic
    bf16x3 weight gradient always runs its 64 x 64 kernel / its wide 128 x 256 kernel wherever the operands allow it."""
    load().sfod_set_conv_algo(int(algo))


def set_wgrad3x3_pipe(on):
    """bf16x3 halo-patch weight gradient: 2 = 64 x 64-block kernel on 128-pixel tiles (default), 1 = pipelined 64 x 32-block
    loop, 0 = the round-2 loop (A/B knob, include/sfod_hip.h)."""
    load().sfod_set_wgrad3x3_pipe(int(on))


def set_gemm_tile(tile):
    """Tile shape of the generic implicit-GEMM kernel: 0 the planner's choice, 1..8 see include/sfod_hip.h (A/B runs, tests;
    other values mean 0).  A shape the layer cannot take falls back to the planner's: ``last_conv_kernel`` says what ran."""
    load().sfod_set_gemm_tile(int(tile))


def set_conv3x3_variant(variant):
    """Workgroup shape of the halo-patch kernel: 0 auto, 1..9 see include/sfod_hip.h (A/B runs, tests; other values mean 0).
    7 / 8 / 9 need operand pairs with logical Cin % 32 == 0; elsewhere they run another kernel: ``last_conv_kernel`` says
    which."""
    load().sfod_set_conv3x3_variant(int(variant))


def last_conv_kernel():
    """Name of the kernel instantiation the calling thread's last convolution launch ran (e.g. "k_conv3x3_m16<8,2,1,0,0,1>"),
    "" before the first one: a host-side record set where the launch is issued (include/sfod_hip.h sfod_last_conv_kernel)."""
    buf = ctypes.create_string_buffer(256)
    n = load().sfod_last_conv_kernel(buf, len(buf))
    if n < 0:
        _chk(n, "sfod_last_conv_kernel")
    return buf.value.decode()


def set_deterministic(on):
    """No float atomics in weight / bias gradients (include/sfod_hip.h: sfod_set_deterministic); -> previous setting."""
    lib = load()
    prev = bool(lib.sfod_get_deterministic())
    lib.sfod_set_deterministic(int(bool(on)))
    return prev


def set_bn_finalize_fused(on):
    """One-launch BatchNorm finalize for layers of <= 64 statistics blocks (default on; include/sfod_hip.h)."""
    load().sfod_set_bn_finalize_fused(int(bool(on)))


def set_conv3x3_m16(on):
    """Automatic shape choice: run the 256 x 128 shape on 16x16x32 MFMAs (default on; include/sfod_hip.h)."""
    load().sfod_set_conv3x3_m16(int(on))       # 0 off, 1 the 8-wave form, 2 the 4-wave form


# =================================================================================================
# tensor-level wrappers (allocate outputs with torch, call the C ABI)
# =================================================================================================
_const_cache = {}


def dev_const(values, dtype, device):
    """Small host-side constants (image sizes, pointer tables) as device tensors, cached by value: a
    pageable host-to-device copy is synchronous and would stall the launch queue every time it recurs."""
    key = (values, dtype, str(device))
    t = _const_cache.get(key)
    if t is None:
        if len(_const_cache) > 4096:
            _const_cache.clear()
        t = torch.tensor(values, dtype=dtype).to(device)
        _const_cache[key] = t
    return t


_PIN_SLOTS, _PIN_WIDTH = 32, 64
_pin_ring = {}


def _pinned_upload_i64(values, dev):
    """Small int64 host vector -> device tensor through a ring of pinned staging slots (asynchronous
    host-to-device copy on the current stream).  A slot is reused only after the copy that read it has
    completed (its event), so the host may run any number of steps ahead."""
    n = len(values)
    if n > _PIN_WIDTH:
        return torch.tensor(values, dtype=torch.int64).to(dev)
    st = _pin_ring.get(dev)
    if st is None:
        st = {"buf": torch.empty(_PIN_SLOTS, _PIN_WIDTH, dtype=torch.int64).pin_memory(), "ev": [None] * _PIN_SLOTS,
              "next": 0}
        _pin_ring[dev] = st
    i = st["next"]
    st["next"] = (i + 1) % _PIN_SLOTS
    if st["ev"][i] is not None:
        st["ev"][i].synchronize()
    slot = st["buf"][i, :n]
    slot.copy_(torch.tensor(values, dtype=torch.int64))
    out = slot.to(dev, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    st["ev"][i] = ev
    return out


def preprocess(images_u8, Hp, Wp, cpad, mean, std, dt):
    """images_u8: list of uint8 device tensors [3,h,w] -> (x [B,Hp,Wp,cpad], sizes int32 [B,2])."""
    dev = images_u8[0].device
    B = len(images_u8)
    imgs = [im.contiguous() for im in images_u8]
    # pointer table: written into a pinned staging slot and copied asynchronously (a pageable copy blocks
    # the host until the stream drains, and the image addresses change whenever the allocator hands out
    # another block, so caching them by value still missed every other step)
    ptrs = _pinned_upload_i64([im.data_ptr() for im in imgs], dev)
    sizes = dev_const(tuple((int(im.shape[1]), int(im.shape[2])) for im in imgs), torch.int32, dev)
    out = torch.empty(B, Hp, Wp, cpad, dtype=torch_dtype(dt), device=dev)
    m = (ctypes.c_float * 3)(*mean)
    s = (ctypes.c_float * 3)(*std)
    lib = load()
    rc = lib.sfod_preprocess(ptrs.data_ptr(), sizes.data_ptr(), B, Hp, Wp, cpad,
                             ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p),
                             out.data_ptr(), dt, _stream())
    _chk(rc, "sfod_preprocess")
    out._keepalive = (imgs, ptrs)
    return out, sizes


def pil_bilinear_coeffs(in_size, out_size):
    """Pillow's precompute_coeffs (BILINEAR, box = the whole axis) + normalize_coeffs_8bpc, same float64
    operation order: -> (bounds int32 [out,2] = (first index, count), coeffs int32 [out,ksize], ksize)."""
    import math
    import numpy as np
    scale = float(in_size) / float(out_size)
    filterscale = scale if scale >= 1.0 else 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)          # C double -> int: truncation (operand is > -1 here)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        k = [0.0] * ksize
        ww = 0.0
        for x in range(xmax):
            a = abs((x + xmin - center + 0.5) * ss)
            w = 1.0 - a if a < 1.0 else 0.0
            k[x] = w
            ww += w
        for x in range(xmax):
            if ww != 0.0:
                k[x] /= ww
        bounds[xx] = (xmin, xmax)
        for x in range(ksize):
            v = k[x] * (1 << 22)
            kk[xx, x] = int(v - 0.5) if k[x] < 0 else int(v + 0.5)
    return bounds, kk, ksize


def pil_bilinear_coeffs_np(in_size, out_size):
    """``pil_bilinear_coeffs`` without the Python double loop: numpy float64, the same operations in the same order (the
    weights' sum runs tap by tap like the loop's), so the integers are equal (tests/test_weak_augment_host.py).  With
    INPUT.CROP nearly every frame brings a new (in, out) pair per axis, and the table sits on the loader's critical path."""
    import math
    import numpy as np
    scale = float(in_size) / float(out_size)
    filterscale = scale if scale >= 1.0 else 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)      # C double -> int: truncation (operand > -1)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    a = np.abs(((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss)
    k = np.where((a < 1.0) & (x < xmax[:, None]), 1.0 - a, 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for i in range(ksize):                       # sequential like the loop's ww += w (zeros beyond xmax change nothing)
        ww = ww + k[:, i]
    k = np.where(ww[:, None] != 0.0, k / np.where(ww != 0.0, ww, 1.0)[:, None], k)
    v = k * float(1 << 22)
    kk = np.where(k < 0, np.trunc(v - 0.5), np.trunc(v + 0.5)).astype(np.int32)
    bounds = np.stack([xmin, xmax], axis=1).astype(np.int32)
    return bounds, kk, ksize


# (device, stream, in, out) -> (bounds, coeffs, ksize) of ONE axis on the device: rows and columns share entries, and the
# cache is bounded (least recently used goes first) -- with INPUT.CROP the shapes never stop coming.  Per stream, like the
# workspaces below: an evicted table's memory returns to the allocator in the order of the stream that allocated and read it.
_RESIZE_TABS_MAX = 512
_resize_tabs = collections.OrderedDict()


def _axis_tabs(device, in_size, out_size):
    import numpy as np
    key = (device, _stream(), int(in_size), int(out_size))
    tabs = _resize_tabs.get(key)
    if tabs is not None:
        _resize_tabs.move_to_end(key)
        return tabs
    bounds, kk, ksize = pil_bilinear_coeffs_np(in_size, out_size)
    both = torch.from_numpy(np.concatenate([bounds.ravel(), kk.ravel()])).to(device)       # one upload per axis
    n = bounds.size
    tabs = (both[:n], both[n:], ksize)
    _resize_tabs[key] = tabs
    while len(_resize_tabs) > _RESIZE_TABS_MAX:
        _resize_tabs.popitem(last=False)
    return tabs


def resize_bilinear_u8(img, newh, neww, flip=False):
    """uint8 [C,H,W] device frame -> [C,newh,neww], bit-exact with PIL ``Image.resize((neww, newh), BILINEAR)``
    (optionally followed by a horizontal flip), in one launch."""
    assert img.dtype == torch.uint8 and img.dim() == 3
    img = img.contiguous()
    C, H, W = img.shape
    hb, hk, ksh = _axis_tabs(img.device, W, neww)
    vb, vk, ksv = _axis_tabs(img.device, H, newh)
    out = torch.empty(C, newh, neww, dtype=torch.uint8, device=img.device)
    call("sfod_resize_bilinear_u8", img, out, C, H, W, newh, neww, hb, hk, ksh, vb, vk, ksv, int(flip))
    return out


FLIP_NONE, FLIP_HORIZONTAL, FLIP_VERTICAL = 0, 1, 2


def weak_augment_u8(img, window, out_hw, flip_mode, out=None):
    """The weak augmentation of one uint8 [C,H,W] device frame in one launch (sfod_resize_bilinear_u8_opt):
    ``flip(PIL.resize(img[:, y0:y0+ch, x0:x0+cw], (w, h), BILINEAR))``, bit for bit.  ``window`` = (y0, x0, ch, cw) or None
    (the whole frame), ``out_hw`` = (h, w), ``flip_mode`` 0 none / 1 horizontal / 2 vertical.  Output extents equal to the
    window's: a windowed copy (+ flip), no tables.  Bad windows / modes are refused by the library (NativeLibraryError)."""
    assert img.dtype == torch.uint8 and img.dim() == 3
    img = img.contiguous()
    C, H, W = img.shape
    y0, x0, ch, cw = (0, 0, H, W) if window is None else (int(v) for v in window)
    h, w = int(out_hw[0]), int(out_hw[1])
    if (h, w) == (ch, cw) or min(ch, cw, h, w) < 1:          # (non-positive extents: the library's refusal, not a table error)
        hb = hk = vb = vk = None
        ksh = ksv = 1
    else:
        hb, hk, ksh = _axis_tabs(img.device, cw, w)
        vb, vk, ksv = _axis_tabs(img.device, ch, h)
    if out is None:
        out = torch.empty(C, max(h, 0), max(w, 0), dtype=torch.uint8, device=img.device)
    call("sfod_resize_bilinear_u8_opt", img, out, C, H, W, y0, x0, ch, cw, h, w, hb, hk, ksh, vb, vk, ksv, int(flip_mode))
    return out


def _axis_tab_base(device, in_size, out_size):
    """-> (pointer to one axis' table as sfod_mosaic_u8 takes it: bounds [out][2] immediately followed by coefficients
    [out][ksize], ksize).  That is how ``_axis_tabs`` uploads an axis (one tensor, two views)."""
    b, k, ksize = _axis_tabs(device, in_size, out_size)
    assert k.data_ptr() == b.data_ptr() + 4 * b.numel(), "the coefficient table must follow its bounds"
    return b.data_ptr(), ksize


def mosaic_u8(tiles, up_hw, rects, out_hw, fill=114, out=None):
    """The mosaic of up to four uint8 [3,h0,w0] device tiles in ONE launch (sfod_mosaic_u8): tile k is scaled to ``up_hw[k]``
    = (h, w) like ``PIL.resize(..., BILINEAR)`` bit for bit, its window ``rects[k][1]`` = (sx1, sy1, sx2, sy2) is pasted at
    ``rects[k][0]`` = (lx1, ly1, lx2, ly2) of a [2*H0, 2*W0] canvas filled with ``fill`` (in order: later tiles overwrite
    earlier ones), and the canvas is halved with the rounded 2x2 mean -> uint8 [3,H0,W0] with (H0, W0) = ``out_hw``.  Neither
    the canvas nor an up-scaled tile is materialised.  A tile whose (h, w) equals its own size is copied (no tables).  Bad
    rectangles are refused by the library (NativeLibraryError) and ``out`` stays untouched."""
    n = len(tiles)
    assert n == len(up_hw) == len(rects)
    H0, W0 = int(out_hw[0]), int(out_hw[1])
    dev = tiles[0].device
    ptrs = (ctypes.c_void_p * max(n, 1))()
    tabs = (ctypes.c_void_p * max(2 * n, 1))()
    geom = (ctypes.c_int32 * max(14 * n, 1))()
    tiles = [t.contiguous() for t in tiles]
    for k, t in enumerate(tiles):
        assert t.dtype == torch.uint8 and t.dim() == 3 and t.shape[0] == 3 and t.is_cuda
        h0, w0 = int(t.shape[1]), int(t.shape[2])
        h, w = int(up_hw[k][0]), int(up_hw[k][1])
        ksh = ksv = 1
        if (h, w) != (h0, w0) and min(h, w, h0, w0) >= 1:
            tabs[2 * k], ksh = _axis_tab_base(dev, w0, w)
            tabs[2 * k + 1], ksv = _axis_tab_base(dev, h0, h)
        ptrs[k] = t.data_ptr()
        geom[14 * k:14 * k + 14] = [h0, w0, h, w] + [int(v) for v in rects[k][0]] + [int(v) for v in rects[k][1]] + [ksh, ksv]
    if out is None:
        out = torch.empty(3, max(H0, 0), max(W0, 0), dtype=torch.uint8, device=dev)
    assert out.dtype == torch.uint8 and out.is_contiguous() and tuple(out.shape) == (3, H0, W0)
    lib = load()
    rc = lib.sfod_mosaic_u8(ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(tabs, ctypes.c_void_p),
                            ctypes.cast(geom, ctypes.c_void_p), n, int(fill), out.data_ptr(), H0, W0, _stream())
    _chk(rc, "sfod_mosaic_u8")
    return out


AUG_BRIGHTNESS, AUG_CONTRAST, AUG_SATURATION, AUG_HUE, AUG_GRAYSCALE = 0, 1, 2, 3, 4
_aug_ws = {}


def aug_color(img, ops):
    """Point operations of the strong augmentation on a uint8 [3,H,W] device frame, in order: ``ops`` =
    [(code, factor)] with the factors torchvision draws (brightness / contrast / saturation factor, hue_factor in
    [-0.5, 0.5]; grayscale ignores it).  Bit-exact with the torchvision-on-Pillow path.  -> new tensor."""
    assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[0] == 3
    img = img.contiguous()
    if not ops:
        return img.clone()
    codes = torch.tensor([int(c) for c, _ in ops], dtype=torch.int32)
    # hue: np.uint8(hue_factor * 255) -- double product, truncation toward zero, wrap-around
    factors = torch.tensor([float(int(f * 255) & 255) if c == AUG_HUE else float(f) for c, f in ops],
                           dtype=torch.float32)
    key = (img.device, torch.cuda.current_stream(img.device).cuda_stream)
    ws = _aug_ws.get(key)
    if ws is None:
        ws = _aug_ws[key] = torch.zeros(1, dtype=torch.int64, device=img.device)
    out = torch.empty_like(img)
    # codes / factors are HOST arrays (copied into the launch arguments before the call returns)
    call("sfod_aug_color", img, out, img.shape[1], img.shape[2], len(ops), codes.data_ptr(), factors.data_ptr(), ws)
    return out


def aug_gaussian_blur(img, sigma):
    """Pillow ``ImageFilter.GaussianBlur(radius=sigma)`` on a uint8 [C,H,W] device frame.  -> new tensor."""
    assert img.dtype == torch.uint8 and img.dim() == 3
    img = img.contiguous()
    out, tmp = torch.empty_like(img), torch.empty_like(img)
    call("sfod_aug_gaussian_blur", img, out, tmp, img.shape[0], img.shape[1], img.shape[2], float(sigma))
    return out


def aug_erase_(img, i, j, h, w, noise):
    """In place: RandomErasing(value="random") + ToPILImage -- rectangle <- (uint8)(noise * 255), noise [C,h,w]."""
    assert img.dtype == torch.uint8 and img.dim() == 3 and img.is_contiguous()
    assert noise.dtype == torch.float32 and tuple(noise.shape) == (img.shape[0], h, w) and noise.is_contiguous()
    call("sfod_aug_erase", img, img.shape[0], img.shape[1], img.shape[2], int(i), int(j), int(h), int(w), noise)
    return img


def hflip_u8(img):
    """uint8 [C,H,W] device image -> horizontally flipped copy."""
    assert img.dtype == torch.uint8 and img.dim() == 3
    img = img.contiguous()
    out = torch.empty_like(img)
    call("sfod_hflip_u8", img, out, img.shape[0], img.shape[1], img.shape[2])
    return out


def _wscale_slots(n, dev):
    """device words the `_ws` packers publish max|w| in (SFOD_F16X3 weights carry a per-tensor power-of-two scale,
    include/sfod_hip.h); a packed tensor keeps its word as ``.wscale`` and the forward wrappers hand it to the kernels"""
    return torch.empty(n, dtype=torch.int32, device=dev)


def wscale_of(w_packed):
    ws = getattr(w_packed, "wscale", None)
    if w_packed.dtype == SPLITH_DTYPE and ws is None:
        raise NativeLibraryError("an SFOD_F16X3 weight tensor lost its scale word (.wscale): pass the packer's own tensor, "
                                 "not a view of it")
    return ws


_f16_words = {}


def check_f16x3_range(device):
    """Raise if any producer of half pairs on ``device`` had to clamp a value beyond +-65504 (infinities included) since the last call
    (sfod_f16x3_poll).  One host synchronisation: call it where the step synchronises anyway (the metrics flush)."""
    w = _f16_words.get(device)
    if w is None:
        w = _f16_words[device] = torch.zeros(1, dtype=torch.int32, device=device)
    call("sfod_f16x3_poll", w)
    if w.item() != 0:
        w.zero_()
        raise FloatingPointError(
            "SFOD.COMPUTE_DTYPE f16x3: an activation or scaled weight beyond half's range (|v| > 65504) was clamped "
            "since the last check -- the model leaves the exponent window this mode assumes; use \"fp32\" (or \"bf16x3\").")


def pack_conv_weight(w_oihw, cin_pad, dt, rot180=False):
    cout, cin, ks, _ = w_oihw.shape
    rows = cin if rot180 else cout
    out = torch.empty(rows, ks * ks, cin_pad, dtype=torch_dtype(dt), device=w_oihw.device)
    ws = _wscale_slots(1, w_oihw.device) if dt == F16X3 else None
    call("sfod_pack_conv_weight_ws", w_oihw.contiguous(), out, ws, cout, cin, ks, cin_pad, int(rot180), dt)
    if ws is not None:
        out.wscale = ws
    return out


def grad_sink(param):
    """The tensor a hand-written backward may ACCUMULATE a parameter gradient into directly (the
    parameter's view of the flat gradient buffer, zeroed by zero_grad), or None -> return the gradient to
    autograd instead.  Saves the temporary and autograd's separate accumulate kernel per parameter."""
    g = getattr(param, "grad", None)
    if g is not None and g.is_cuda and g.dtype == torch.float32 and g.is_contiguous() and g.shape == param.shape:
        return g
    return None


class ConvWeightPacker:
    """All conv weights of a module packed by ONE launch per call (the per-layer kernels are launch-bound:
    ~8 us each for <= 9 MB).  ``specs``: list of (weight parameter OIHW, inner_pad, rot180).  The descriptor
    table lives on the device and is rebuilt only when a parameter's storage moved."""

    def __init__(self, specs, dt):
        self.specs, self.dt = list(specs), dt
        self._ptrs = None
        self.views = None

    def _build(self):
        dev = self.specs[0][0].device
        tdt = torch_dtype(self.dt)
        sizes, blocks = [], []
        for w, pad, rot in self.specs:
            cout, cin, ks, _ = w.shape
            rows = cin if rot else cout
            sizes.append((rows, ks * ks, pad))
            blocks.append(query("sfod_pack_conv_weights_blocks", cout, cin, ks, pad, int(rot)))
        offs, tot = [], 0
        for r, t, p_ in sizes:
            offs.append(tot)
            tot += (r * t * p_ + 127) // 128 * 128          # keep every packed tensor 256-byte aligned
        self._buf = torch.empty(tot, dtype=tdt, device=dev)
        self.views = [self._buf[o:o + r * t * p_].view(r, t, p_) for o, (r, t, p_) in zip(offs, sizes)]
        self._amax = _wscale_slots(len(self.specs), dev) if self.dt == F16X3 else None
        if self._amax is not None:
            for i, v in enumerate(self.views):
                v.wscale = self._amax[i:i + 1]
        rows, first = [], 0
        for (w, pad, rot), v, nb in zip(self.specs, self.views, blocks):
            cout, cin, ks, _ = w.shape
            rows.append([w.data_ptr(), v.data_ptr(), cout, cin, ks, pad, int(rot), first])
            first += nb
        rows.append([0, 0, 0, 0, 0, 0, 0, first])
        self._total = first
        self._desc = torch.tensor(rows, dtype=torch.int64).to(dev)
        self._ptrs = tuple(w.data_ptr() for w, _, _ in self.specs)

    def pack(self):
        ptrs = tuple(w.data_ptr() for w, _, _ in self.specs)
        if ptrs != self._ptrs:
            for w, _, _ in self.specs:
                assert w.is_contiguous() and w.dtype == torch.float32
            self._build()
        call("sfod_pack_conv_weights_multi_ws", self._desc, len(self.specs), self._total, self.dt, self._amax)
        return self.views


class PackedConvWeights:
    """A module's forward weights and (for a backward) rotated data-gradient weights: ONE ConvWeightPacker when both are
    packed in the same operand format, two when the gradient format differs ("f16x3": half pairs forward, bf16 pairs
    rotated) -- one launch per operand format and ``pack()``.  ``rot`` may be empty (forward-only pass)."""

    def __init__(self, fwd, rot, dt, gdt):
        self.n = len(fwd)
        if gdt == dt or not rot:
            self.packers = [ConvWeightPacker(list(fwd) + list(rot), dt)]
        else:
            self.packers = [ConvWeightPacker(fwd, dt), ConvWeightPacker(rot, gdt)]

    def pack(self):
        """-> (forward views, rotated views), each in the order of its specs"""
        views = [v for pk in self.packers for v in pk.pack()]
        return views[:self.n], views[self.n:]


def unpack_conv_wgrad(dw_packed, dw_oihw, accumulate=False):
    cout, cin, ks, _ = dw_oihw.shape
    call("sfod_unpack_conv_wgrad", dw_packed, dw_oihw, cout, cin, ks, dw_packed.shape[-1], int(accumulate))


def pack_fc_weight(w, dt, chw_c=0, transpose=False, ld=None):
    n, k = w.shape
    inner = n if transpose else k
    ld = ld or inner
    out = torch.empty(k if transpose else n, ld, dtype=torch_dtype(dt), device=w.device)
    ws = _wscale_slots(1, w.device) if dt == F16X3 else None
    call("sfod_pack_fc_weight_ld_ws", w.contiguous(), out, ws, n, k, chw_c, int(transpose), ld, dt)
    if ws is not None:
        out.wscale = ws
    return out


def unpack_fc_wgrad(dw_packed, dw, chw_c=0, accumulate=False):
    n, k = dw.shape
    call("sfod_unpack_fc_wgrad_ld", dw_packed, dw, n, k, chw_c, dw_packed.shape[-1], int(accumulate))


def _stats_buffer(B, H, W, cin, cout, ksize, dt, dev):
    """BatchNorm partial-statistics buffer of a convolution's epilogue (``.nblk`` rows for bn_finalize)"""
    nb = query("sfod_conv_stats_blocks", B, H, W, cin, cout, ksize, dt)
    stats = torch.empty(nb * (2 * cout + 1), dtype=torch.float32, device=dev)
    stats.nblk = nb
    return stats


def conv_fwd(x, w_packed, bias, cout, ksize, act=0, out_dtype=None, ldy=None, want_stats=False):
    """x [B,H,W,Cin] NHWC (or [R,K] with ksize=1) -> y [B,H,W,ldy]; optional BN partial stats."""
    x = as_operand(x, w_packed.dtype)
    dt = dt_of(x)
    if x.dim() == 2:
        B, H, W, cin = x.shape[0], 1, 1, x.shape[1]
        oshape = lambda ld: (x.shape[0], ld)
    else:
        B, H, W, cin = x.shape
        oshape = lambda ld: (B, H, W, ld)
    out_dtype = out_dtype or out_dtype_of(x.dtype)
    ldy = ldy or cout
    alloc = torch.zeros if ldy != cout else torch.empty
    y = alloc(oshape(ldy), dtype=out_dtype, device=x.device)
    stats = _stats_buffer(B, H, W, cin, cout, ksize, dt, x.device) if want_stats else None
    flops, tag = 2.0 * B * H * W * cout * ksize * ksize * cin, ""
    if _timer is not None:
        tag = ":patch3x3" if query("sfod_conv_fwd_algo", B, H, W, cin, cout, ksize, dt) == 2 else ":gemm"
    odt = dt_of_dtype(out_dtype)
    # linear layers with few rows (one frame per GPU): the library asks for slab scratch and splits along K
    nscratch = load().sfod_conv_fwd_scratch_bytes(B, H, W, cin, cout, ksize, dt, odt, int(want_stats)) if ksize == 1 else 0
    if nscratch > 0:
        scratch = torch.empty(nscratch, dtype=torch.uint8, device=x.device)
        call("sfod_conv_fwd_scratch", x, w_packed, wscale_of(w_packed), bias, y, B, H, W, cin, cout, ksize, ldy, act, stats,
             dt, odt, scratch, nscratch, timer_name="sfod_conv_fwd", flops=flops, tag=tag)
    else:
        call("sfod_conv_fwd_ws", x, w_packed, wscale_of(w_packed), bias, y, B, H, W, cin, cout, ksize, ldy, act, stats, dt,
             odt, timer_name="sfod_conv_fwd", flops=flops, tag=tag)
    return (y, stats) if want_stats else y


def conv_fwd_bnin_supported(y_pre, w_packed, cout):
    """Can the 3x3 convolution that consumes relu(bn(y_pre)) take y_pre itself (BatchNorm + ReLU + pair split in the kernel's
    LDS patch, include/sfod_hip.h: sfod_conv_fwd_bnin)?"""
    if y_pre.dim() != 4 or y_pre.dtype != torch.float32 or w_packed.dtype != SPLIT_DTYPE:
        return False
    B, H, W, cin = y_pre.shape
    return bool(query("sfod_conv_fwd_bnin_supported", B, H, W, cin, cout, BF16X3))


def conv_fwd_bnin(y_pre, mean, invstd, gamma, beta, w_packed, bias, cout, act=0, want_stats=False):
    """conv3x3(relu(bn(y_pre))) without materialising the activated tensor (forward-only passes).  -> y fp32 [B,H,W,cout]
    (+ BatchNorm partial statistics), bit-identical to bn_relu_pool_fwd(pairs) followed by conv_fwd."""
    B, H, W, cin = y_pre.shape
    y = torch.empty((B, H, W, cout), dtype=torch.float32, device=y_pre.device)
    stats = _stats_buffer(B, H, W, cin, cout, 3, BF16X3, y_pre.device) if want_stats else None
    call("sfod_conv_fwd_bnin", y_pre, mean, invstd, gamma, beta, w_packed, bias, y, B, H, W, cin, cout, cout, act, stats,
         BF16X3, timer_name="sfod_conv_fwd", flops=2.0 * B * H * W * cout * 9 * cin, tag=":patch3x3")
    return (y, stats) if want_stats else y


def conv_first_supported(x, cout):
    if x.dim() != 4 or x.dtype not in (torch.bfloat16,) + PAIR_DTYPES:
        return False
    B, H, W, cin = x.shape
    return bool(query("sfod_conv_first_supported", B, H, W, cin, cout, dt_of(x), cout))


def conv_first_stats(x, w_packed, bias):
    """First VGG layer, pass 1 of the recompute-fused form: BatchNorm partial statistics only, nothing stored."""
    B, H, W, cin = x.shape
    stats = _stats_buffer(B, H, W, cin, 64, 3, dt_of(x), x.device)
    call("sfod_conv_first_fused_ws", x, w_packed, wscale_of(w_packed), bias, None, None, None, stats, B, H, W, 64, 0,
         dt_of(x))
    return stats


def conv_first_apply(x, w_packed, bias, scale, shift, relu=True):
    """Pass 2: z = act(scale * (conv + bias) + shift) [B,H,W,64] in x's operand dtype (bf16 / bf16x3 pairs); the
    pre-BatchNorm output is never stored."""
    B, H, W, cin = x.shape
    z = torch.empty(B, H, W, 64, dtype=x.dtype, device=x.device)
    call("sfod_conv_first_fused_ws", x, w_packed, wscale_of(w_packed), bias, scale, shift, z, None, B, H, W, 64,
         1 if relu else 0, dt_of(x))
    return z


def set_conv_first_pipe(on):
    """bf16x3 / f16x3 first-layer kernel: 1 (default) the pipelined tile loop, 0 the plain one.  Same bits (A/B knob,
    include/sfod_hip.h)."""
    load().sfod_set_conv_first_pipe(int(on))


def set_conv_first_grid(n):
    """Cap the first-layer kernel's persistent grid at ``n`` workgroups (0: one per resident slot): several tiles per
    workgroup on small images."""
    load().sfod_set_conv_first_grid(int(n))


def set_first_apply_recompute(on):
    """Student conv1_1's BatchNorm + ReLU pass: 1 (default) by recomputing the convolution (``conv_first_bn_apply``), 0 the
    elementwise pass over y.  Same bits either way (A/B knob, include/sfod_hip.h)."""
    load().sfod_set_first_apply_recompute(int(on))


def conv_first_bn_apply_supported(x, y, cout, pool, relu=True):
    """whether ``conv_first_bn_apply`` reproduces ``bn_relu_pool_fwd(y, ...)`` (bf16 pairs out) for the layer with operand
    ``x`` and pre-BatchNorm output ``y`` of ``conv_fwd`` (first layer, bf16 pairs, ReLU, no pooling)"""
    if x.dim() != 4 or y.dim() != 4 or not x.is_cuda or tuple(y.shape) != (*x.shape[:3], cout):
        return False
    if x.dtype not in PAIR_DTYPES:
        return False
    B, H, W, cin = x.shape
    return bool(query("sfod_conv_first_bn_apply_supported", B, H, W, cin, cout, int(pool) | (0 if relu else 2), dt_of(x),
                      dt_of(y)))


def conv_first_bn_apply(x, w_packed, bias, mean, invstd, gamma, beta):
    """z = relu(bn(conv(x) + bias)) [B,H,W,64] as bf16 pairs, the convolution recomputed: bit-identical to
    ``bn_relu_pool_fwd(conv_fwd(x, ...), mean, invstd, gamma, beta, False, out_dtype=x.dtype)`` where
    ``conv_first_bn_apply_supported`` holds."""
    B, H, W, cin = x.shape
    z = torch.empty(B, H, W, 64, dtype=x.dtype, device=x.device)
    call("sfod_conv_first_bn_apply", x, w_packed, bias, mean, invstd, gamma, beta, z, B, H, W, 64, dt_of(x))
    return z


_ws_cache = {}


def _workspace(dev, nbytes):
    """Grow-only scratch buffer per (device, stream): reuse is stream-ordered, two streams never share one."""
    key = (dev, _stream())
    cur = _ws_cache.get(key)
    if cur is None or cur.numel() < nbytes:
        cur = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        _ws_cache[key] = cur
    return cur


def _wgrad_call(name, args, extents, flops, timer_name=None):
    """The weight-gradient entry point ``name(*args, ws, ws_bytes)`` with the workspace sfod_conv_wgrad_ws_bytes asks for
    ``extents`` = (B, H, W, Cin, Cout, ksize, lddy, dt): the largest need of any of its sub-launches, NULL where it is 0."""
    nbytes = query("sfod_conv_wgrad_ws_bytes", *extents)
    ws = _workspace(args[0].device, nbytes) if nbytes > 0 else None
    call(name, *args, ws, nbytes, timer_name=timer_name, flops=flops)


def conv_wgrad(x, dy, cout, ksize, dw_packed=None, operand=None):
    """-> fp32 packed grad [Cout, taps, Cin] (accumulated into dw_packed if given).  ``operand``: MFMA operand dtype
    (default: x's); fp32 inputs of a bf16x3 model are converted to pairs here."""
    operand = operand or x.dtype
    x, dy = as_operand(x, operand), as_operand(dy, operand)
    dt = dt_of(x)
    if x.dim() == 2:
        B, H, W, cin = x.shape[0], 1, 1, x.shape[1]
    else:
        B, H, W, cin = x.shape
    lddy = dy.shape[-1]
    # bf16x3 rows come in whole 8-channel groups: compute ceil8(cout) rows (dy's padding columns are zero)
    cout_k = (cout + 7) // 8 * 8 if dt in (BF16X3, F16X3) else cout
    assert cout_k <= lddy, "dy narrower than the padded output-channel count"
    if dw_packed is None or cout_k != cout:
        assert dw_packed is None, "accumulating bf16x3 weight gradients needs Cout % 8 == 0"
        dw_packed = torch.zeros(cout_k, ksize * ksize, cin, dtype=torch.float32, device=x.device)
    extents = (B, H, W, cin, cout_k, ksize, lddy, dt)
    _wgrad_call("sfod_conv_wgrad", (x, dy, dw_packed, *extents), extents, 2.0 * B * H * W * cout * ksize * ksize * cin)
    return dw_packed if cout_k == cout else dw_packed[:cout]


def conv_wgrad_oihw_supported(x, dy, cout, ksize):
    if x.dim() != 4:
        return False
    B, H, W, cin = x.shape
    if dt_of(x) == BF16X3 and (cout % 8 or dy.shape[-1] % 8):
        return False
    return bool(query("sfod_conv_wgrad_oihw_supported", B, H, W, cin, cout, ksize, dy.shape[-1], dt_of(x)))


def conv_wgrad_oihw(x, dy, dw_oihw, accumulate=False):
    """3x3 weight gradient written straight into the state-dict layout (e.g. ``grad_sink(conv.weight)``)."""
    cout, cin, ksize, _ = dw_oihw.shape
    B, H, W, cinp = x.shape
    assert cinp == cin and dw_oihw.is_contiguous() and dw_oihw.dtype == torch.float32
    dy = as_operand(dy, x.dtype)
    extents = (B, H, W, cin, cout, ksize, dy.shape[-1], dt_of(x))
    _wgrad_call("sfod_conv_wgrad_oihw", (x, dy, dw_oihw, *extents, int(accumulate)), extents,
                2.0 * B * H * W * cout * ksize * ksize * cin)
    return dw_oihw


def _deliver_wgrad(weight, into_sink, packed):
    """Where a convolution's weight gradient goes: ``into_sink(sink)`` adds it straight into ``grad_sink(weight)`` and says
    whether it could; otherwise ``packed()`` makes it in the packed layout [Cout, taps, Cin], which is unpacked into the
    sink (-> None: nothing for autograd to add) or, for a parameter without one, into a new tensor."""
    sink = grad_sink(weight)
    if sink is not None and into_sink(sink):
        return None
    dwp = packed()
    if sink is not None:
        unpack_conv_wgrad(dwp, sink, accumulate=True)
        return None
    dw = torch.empty_like(weight)
    unpack_conv_wgrad(dwp, dw)
    return dw


def conv_weight_grad(x, dy, weight, operand=None):
    """dL/dweight of a conv whose state-dict weight is ``weight`` (OIHW).  Accumulated straight into
    ``grad_sink(weight)`` when the parameter has one (returns None: nothing for autograd to add), else
    returned as a new tensor."""
    operand = operand or x.dtype
    x, dy = as_operand(x, operand), as_operand(dy, operand)
    cout, cin, k, _ = weight.shape

    def into_sink(sink):
        if k == 3 and x.shape[-1] == cin and conv_wgrad_oihw_supported(x, dy, cout, 3):
            conv_wgrad_oihw(x, dy, sink, accumulate=True)     # the slab reduction writes OIHW directly
            return True
        if k == 1 and x.shape[-1] == cin and (dt_of(x) != BF16X3 or cout % 8 == 0):
            conv_wgrad(x, dy, cout, 1, dw_packed=sink.view(cout, 1, cin))    # packed [Cout,1,Cin] IS the OIHW layout: the
            return True                                                     # kernel's atomics accumulate in place
        return False

    return _deliver_wgrad(weight, into_sink, lambda: conv_wgrad(x, dy, cout, k))


def set_first_wgrad_fused(on):
    """conv1_1's weight gradient: 1 (default) straight from the BatchNorm backward's inputs (``conv_first_wgrad_bn``), 0 the
    apply pass + ``conv_weight_grad``.  Same bits either way (A/B knob, include/sfod_hip.h)."""
    load().sfod_set_first_wgrad_fused(int(on))


def conv_first_wgrad_bn_supported(x, y, cout, pool, relu=True):
    """whether ``conv_first_wgrad_bn`` reproduces ``bn_relu_pool_bwd`` (dy as bf16 pairs) + ``conv_wgrad_oihw`` for the layer
    with weight-gradient operand ``x`` and saved pre-BatchNorm output ``y`` (first layer, bf16 pairs, ReLU, no pooling)"""
    if x is None or x.dim() != 4 or y.dim() != 4 or not x.is_cuda or tuple(y.shape) != (*x.shape[:3], cout):
        return False
    B, H, W, cin = x.shape
    return bool(query("sfod_conv_first_wgrad_bn_supported", B, H, W, cin, cout, int(pool) | (0 if relu else 2),
                      dt_of(x), dt_of(y)))


def conv_first_wgrad_bn(x, dz, y, mean, invstd, gamma, beta, dgamma, dbeta, dw, accumulate=False):
    """The 3x3 weight gradient of the first layer from dz / y and the finalized ``dgamma`` / ``dbeta`` of
    ``bn_relu_pool_bwd(..., apply=False)``, bit-identical to the apply pass followed by ``conv_wgrad`` (``dw`` packed
    [Cout, 9, Cin], always added into) or ``conv_wgrad_oihw`` (``dw`` OIHW, overwritten or added into)."""
    B, H, W, cin = x.shape
    oihw = dw.dim() == 4
    cout = dw.shape[0]
    assert tuple(dw.shape) == ((cout, cin, 3, 3) if oihw else (cout, 9, cin))
    assert dw.is_contiguous() and dw.dtype == torch.float32
    assert dz.dtype == torch.float32 and y.dtype == torch.float32 and dz.shape == y.shape == (B, H, W, cout)
    dt = dt_of(x)
    _wgrad_call("sfod_conv_first_wgrad_bn", (x, dz, y, mean, invstd, gamma, beta, dgamma, dbeta, dw, B, H, W, cin, cout, dt,
                                             int(oihw), int(accumulate)), (B, H, W, cin, cout, 3, cout, dt),
                2.0 * B * H * W * cout * 9 * cin, timer_name="sfod_conv_wgrad_oihw" if oihw else "sfod_conv_wgrad")
    return dw


def conv_first_weight_grad(x, dz, y, mean, invstd, gamma, beta, dgamma, dbeta, weight):
    """``conv_weight_grad(x, dy, weight)`` of the first layer with dy formed inside the kernel (``conv_first_wgrad_bn``): the
    same route into ``grad_sink(weight)`` / a new tensor, so the same bits."""
    cout, cin, _, _ = weight.shape
    args = (x, dz, y, mean, invstd, gamma, beta, dgamma, dbeta)

    def into_sink(sink):
        return x.shape[-1] == cin and conv_first_wgrad_bn(*args, sink, accumulate=True) is sink

    return _deliver_wgrad(weight, into_sink, lambda: conv_first_wgrad_bn(
        *args, torch.zeros(cout, 9, x.shape[-1], dtype=torch.float32, device=x.device)))


def bias_grad(dy, n, db=None, accumulate=False):
    m = dy.numel() // dy.shape[-1]
    if db is None:
        db = torch.empty(n, dtype=torch.float32, device=dy.device)
    call("sfod_bias_grad", dy, db, m, n, dy.shape[-1], int(accumulate), dt_of(dy))
    return db


def bn_finalize(stats, M, C, running_mean, running_var, momentum=0.1, eps=1e-5, update_running=True,
                num_batches_tracked=None, pop=None):
    """``update_running``: False / 0 = no update, True / k = k momentum updates with this batch's statistics;
    ``num_batches_tracked`` (int64 scalar buffer) is incremented by k in the same launch when given.
    ``pop``: the layer's [3, C] fp64 view of a population accumulator (``bn_pop_accumulator``): this batch is merged into it
    by the same launch, the running statistics stay and ``num_batches_tracked`` grows by one (sfod_bn_finalize_pop)."""
    mean = torch.empty(C, dtype=torch.float32, device=stats.device)
    invstd = torch.empty_like(mean)
    ws = torch.empty(query("sfod_bn_finalize_ws_floats", C), dtype=torch.float32, device=stats.device)
    if pop is None:
        call("sfod_bn_finalize", stats, stats.nblk, M, C, mean, invstd, running_mean, running_var,
             float(momentum), float(eps), int(update_running), num_batches_tracked, ws)
        return mean, invstd
    assert pop.is_cuda and pop.dtype == torch.float64 and tuple(pop.shape) == (3, C) and pop.stride(1) == 1
    call("sfod_bn_finalize_pop", stats, stats.nblk, M, C, mean, invstd, running_mean, running_var,
         float(momentum), float(eps), int(update_running), num_batches_tracked, ws, pop.data_ptr(), pop.stride(0))
    return mean, invstd


def bn_pop_accumulator(channels, device):
    """Zeroed population accumulator of a model's BatchNorm layers: one [3, sum C] fp64 tensor (rows n, mean, M2) and each
    layer's [3, C] column view of it, in the order of ``channels``."""
    acc = torch.zeros(3, max(int(sum(channels)), 1), dtype=torch.float64, device=device)
    views, off = [], 0
    for c in channels:
        views.append(acc[:, off:off + c])
        off += c
    return acc, views


def bn_pop_commit(acc, layers):
    """``layers``: (first column, running_mean, running_var) per layer -> every layer's population mean and biased variance
    into its running buffers, ONE launch (a layer that never ran keeps its buffers)."""
    assert acc.is_cuda and acc.dtype == torch.float64 and acc.dim() == 2 and acc.shape[0] == 3 and acc.is_contiguous()
    rows = []
    for off, rm, rv in layers:
        assert rm.dtype == rv.dtype == torch.float32 and rm.is_contiguous() and rv.is_contiguous() and rm.numel() == rv.numel()
        rows.append([int(off), rm.numel(), rm.data_ptr(), rv.data_ptr()])
    if not rows:
        return
    host = torch.tensor(rows, dtype=torch.int64)
    call("sfod_bn_pop_commit", acc, acc.stride(0), host.to(acc.device), host.data_ptr(), len(rows))


def bn_pop_merge(dst, src):
    """dst <- Chan merge of two [3, columns] population accumulators (in place, column by column)."""
    assert dst.shape == src.shape and dst.dtype == src.dtype == torch.float64 and dst.dim() == 2 and dst.shape[0] == 3
    call("sfod_bn_pop_merge", dst, src, dst.shape[1])
    return dst


def bn_relu_pool_fwd(y, mean, invstd, gamma, beta, pool, relu=True, out_dtype=None, with_grad_operand=False):
    """``out_dtype``: y.dtype, or a pair dtype from an fp32 y (the next convolution's operand, written directly).
    ``with_grad_operand`` (out_dtype SPLITH_DTYPE): -> (z, the same values as bf16 pairs: the operand of that
    convolution's weight gradient), both written by the one pass."""
    B, H, W, C = y.shape
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    z = torch.empty(B, Ho, Wo, C, dtype=out_dtype or y.dtype, device=y.device)
    if with_grad_operand and z.dtype == SPLITH_DTYPE:
        z2 = torch.empty(B, Ho, Wo, C, dtype=SPLIT_DTYPE, device=y.device)
        call("sfod_bn_relu_pool_fwd2", y, mean, invstd, gamma, beta, z, z2, B, H, W, C,
             int(pool) | (0 if relu else 2), dt_of(y), dt_of(z))
        return z, z2
    call("sfod_bn_relu_pool_fwd", y, mean, invstd, gamma, beta, z, B, H, W, C, int(pool) | (0 if relu else 2),
         dt_of(y), dt_of(z))
    return (z, z) if with_grad_operand else z


def bn_add_relu_fwd(y, mean, invstd, gamma, beta, residual, with_operand=None, with_grad_operand=False):
    """relu(bn(y) + residual) in one pass (bottleneck tail).  ``with_operand`` (a pair dtype; fp32 data of a bf16x3 /
    f16x3 model): also return the same values as (hi, lo) operand pairs of that type -> (z, z_pairs);
    ``with_grad_operand`` (half pairs only): -> (z, z_pairs, the same as bf16 pairs), all from the one pass."""
    assert residual.shape == y.shape and residual.dtype == y.dtype
    z = torch.empty_like(y)
    C = y.shape[-1]
    with_operand = SPLIT_DTYPE if with_operand is True else with_operand
    zp = torch.empty(y.shape, dtype=with_operand, device=y.device) if with_operand else None
    zg = torch.empty(y.shape, dtype=SPLIT_DTYPE, device=y.device) if (with_grad_operand and with_operand == SPLITH_DTYPE) else None
    call("sfod_bn_add_relu_fwd", y, mean, invstd, gamma, beta, residual.contiguous(), z, zp, zg, y.numel() // C, C, dt_of(y),
         dt_of(zp) if zp is not None else BF16X3)
    if with_grad_operand:
        return z, zp, (zg if zg is not None else zp)
    return (z, zp) if with_operand else z


def bn_relu_pool_bwd(dz, y, mean, invstd, gamma, beta, pool, dgamma=None, dbeta=None, dy=None, relu=True,
                     dgamma_acc=None, dbeta_acc=None, out_dtype=None, reduced=None, apply=True):
    """``dgamma_acc`` / ``dbeta_acc``: gradient accumulators (see ``grad_sink``) updated in the same launch.
    ``out_dtype``: dtype of dy (y.dtype, or SPLIT_DTYPE from fp32 inputs: dy only feeds the wgrad / dgrad MFMAs).
    ``reduced``: the partial-sum workspace ``conv_dgrad_bnred`` returned with dz -- the reduction pass is skipped.
    ``apply`` False: the sums only (same reduction, same finalize), no dy is allocated or written -> (None, dgamma, dbeta);
    for a layer whose dy is formed by its consumer (``conv_first_wgrad_bn``)."""
    B, H, W, C = y.shape
    dy_dt = dt_of_dtype(out_dtype or y.dtype) if dy is None else dt_of(dy)
    if dy is None and apply:
        dy = torch.empty(y.shape, dtype=out_dtype or y.dtype, device=y.device)
    if dgamma is None:
        dgamma = torch.empty(C, dtype=torch.float32, device=y.device)
    if dbeta is None:
        dbeta = torch.empty(C, dtype=torch.float32, device=y.device)
    if reduced is not None:
        ws, nred = reduced, reduced.shape[0] - BN_BWD_SCRATCH_ROWS
        assert reduced.shape[1] == 2 * C and nred > 0 and not pool and relu
    else:
        ws, nred = torch.empty(query("sfod_bn_bwd_ws_floats", B * H * W, C), dtype=torch.float32, device=y.device), 0
    call("sfod_bn_relu_pool_bwd", dz, y, mean, invstd, gamma, beta, dy, dgamma, dbeta, dgamma_acc, dbeta_acc, ws,
         B, H, W, C,
         int(pool) | (0 if relu else 2), dt_of(y), dy_dt, nred)
    return dy, dgamma, dbeta


def group_norm_relu_fwd(y, gamma, beta, groups=32, eps=1e-5, relu=True, out_dtype=None, with_grad_operand=False):
    """GroupNorm + ReLU of a convolution's output ``y`` [R, P, P, C] (or [R, PP, C]) -> (z, z_grad, mean, rstd).
    ``out_dtype``: y.dtype, or a pair dtype from an fp32 y (the next layer's operand, written directly);
    ``with_grad_operand``: ``z_grad`` is what that layer's weight gradient reads -- z itself, or for half pairs the same
    values as bf16 pairs, written by the same pass (None without the flag).  mean / rstd: fp32 [R, groups], for the backward."""
    R, C = y.shape[0], y.shape[-1]
    PP = math.prod(y.shape[1:-1])
    z = torch.empty(y.shape, dtype=out_dtype or y.dtype, device=y.device)
    z2 = torch.empty(y.shape, dtype=SPLIT_DTYPE, device=y.device) if (with_grad_operand and z.dtype == SPLITH_DTYPE) else None
    mean = torch.empty(R, groups, dtype=torch.float32, device=y.device)
    rstd = torch.empty_like(mean)
    call("sfod_group_norm_relu_fwd", y, gamma, beta, z, z2, mean, rstd, R, PP, C, groups, float(eps), int(relu), dt_of(y),
         dt_of(z))
    return z, ((z2 if z2 is not None else z) if with_grad_operand else None), mean, rstd


def group_norm_relu_bwd(dz, y, mean, rstd, gamma, beta, groups=32, relu=True, dgamma=None, dbeta=None, accumulate=False,
                        out_dtype=None):
    """-> (dy, dgamma, dbeta).  ``out_dtype``: dtype of dy (y.dtype, or SPLIT_DTYPE from fp32 inputs: dy only feeds the wgrad /
    dgrad MFMAs).  ``dgamma`` / ``dbeta`` given with ``accumulate``: gradient accumulators (see ``grad_sink``), added into."""
    R, C = y.shape[0], y.shape[-1]
    PP = math.prod(y.shape[1:-1])
    assert dz.dtype == y.dtype and dz.shape == y.shape
    assert not accumulate or (dgamma is not None and dbeta is not None)
    dy = torch.empty(y.shape, dtype=out_dtype or y.dtype, device=y.device)
    if dgamma is None:
        dgamma = torch.empty(C, dtype=torch.float32, device=y.device)
    if dbeta is None:
        dbeta = torch.empty(C, dtype=torch.float32, device=y.device)
    ws = torch.empty(query("sfod_group_norm_bwd_ws_floats", R, C), dtype=torch.float32, device=y.device)
    call("sfod_group_norm_relu_bwd", dz, y, mean, rstd, gamma, beta, dy, dgamma, dbeta, ws, R, PP, C, groups, int(relu),
         int(accumulate), dt_of(y), dt_of(dy))
    return dy, dgamma, dbeta


BN_BWD_SCRATCH_ROWS = 32     # SFOD_BN_BWD_SCRATCH_ROWS of include/sfod_hip.h


def conv_dgrad_bnred(dy, w_rot, cout, y_below, mean, invstd, gamma, beta):
    """3x3 data gradient dz = conv(dy, rotated weights) [B,H,W,cout] fp32, with the BatchNorm-backward reduction of the
    layer below (whose saved pre-BatchNorm output is ``y_below``, same shape as dz) folded into the epilogue.
    -> (dz, partial-sum workspace for ``bn_relu_pool_bwd(reduced=...)``), or None when the shape / dtype is not served
    (caller: plain ``conv_fwd`` + unfused BatchNorm backward)."""
    B, H, W, cin = dy.shape
    if y_below.dtype != torch.float32 or tuple(y_below.shape) != (B, H, W, cout) or not y_below.is_contiguous():
        return None
    nb = query("sfod_conv_dgrad_bnred_blocks", B, H, W, cin, cout, dt_of(dy))
    if nb <= 0:
        return None
    dz = torch.empty(B, H, W, cout, dtype=torch.float32, device=dy.device)
    ws = torch.empty(nb + BN_BWD_SCRATCH_ROWS, 2 * cout, dtype=torch.float32, device=dy.device)   # partial rows + scratch
    # the halo-patch kernel with one more epilogue: same roofline line as sfod_conv_fwd's
    call("sfod_conv_dgrad_bnred", dy, w_rot, dz, B, H, W, cin, cout, dt_of(dy), y_below, mean, invstd, gamma, beta,
         ws, timer_name="sfod_conv_fwd", flops=2.0 * B * H * W * cout * 9 * cin, tag=":patch3x3")
    return dz, ws


def act_bwd_(dy, y, act):
    call("sfod_act_bwd", dy, y, dy.numel(), act, dt_of(dy))
    return dy


def add_(a, b):
    call("sfod_add_inplace", a, b, a.numel(), dt_of(a))
    return a


def add_act_bwd_(a, b, y):
    """a = (a + b) * (y > 0) in place (add_ followed by act_bwd_(.., y, 1))."""
    call("sfod_add_act_bwd", a, b, y, a.numel(), dt_of(a))
    return a


def mul_mask_(a, mask_u8, scale):
    call("sfod_mul_mask", a, mask_u8, a.numel(), float(scale), dt_of(a))
    return a


def add_act(a, b, act=1, with_operand=None, with_grad_operand=False):
    """act(a + b); ``with_operand`` (a pair dtype; fp32 data of a bf16x3 / f16x3 model): also the (hi, lo) operand pairs
    of that type -> (out, out_pairs); ``with_grad_operand``: -> (out, out_pairs, the same as bf16 pairs)."""
    out = torch.empty_like(a)
    with_operand = SPLIT_DTYPE if with_operand is True else with_operand
    op = torch.empty(a.shape, dtype=with_operand, device=a.device) if with_operand else None
    og = torch.empty(a.shape, dtype=SPLIT_DTYPE, device=a.device) if (with_grad_operand and with_operand == SPLITH_DTYPE) else None
    call("sfod_add_act", a, b, out, op, og, a.numel(), int(act), dt_of(a), dt_of(op) if op is not None else BF16X3)
    if with_grad_operand:
        return out, op, (og if og is not None else op)
    return (out, op) if with_operand else out


def subsample2(x):
    B, H, W, C = x.shape
    y = torch.empty(B, (H + 1) // 2, (W + 1) // 2, C, dtype=x.dtype, device=x.device)
    call("sfod_subsample2", x, y, B, H, W, C, 0, dt_of(x))
    return y


def subsample2_bwd(dy, full_shape):
    B, H, W, C = full_shape
    dx = torch.empty(B, H, W, C, dtype=dy.dtype, device=dy.device)
    call("sfod_subsample2", dy, dx, B, H, W, C, 1, dt_of(dy))
    return dx


def im2col_stem(x, kpad=192, out_dtype=None):
    """``out_dtype``: x.dtype, or SPLIT_DTYPE from fp32 (the stem GEMM's operand, no separate conversion pass)."""
    B, H, W, Cp = x.shape
    out = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, kpad, dtype=out_dtype or x.dtype, device=x.device)
    call("sfod_im2col_stem", x, out, B, H, W, Cp, kpad, dt_of(x), dt_of(out))
    return out


def stem7x7_supported(x, dt):
    B, H, W, Cp = x.shape
    return x.dtype == torch.float32 and bool(query("sfod_stem7x7_supported", B, H, W, Cp, dt))


def stem7x7(x, w_packed, bias, act=1):
    """fp32 NHWC input [B,H,W,Cp] -> relu(conv7x7 s2 p3 (+ bias)) fp32 [B,Ho,Wo,64]; w_packed = pack_fc_weight([64,160])."""
    B, H, W, Cp = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty(B, Ho, Wo, 64, dtype=torch.float32, device=x.device)
    call("sfod_stem7x7", x.contiguous(), w_packed, wscale_of(w_packed), bias, y, B, H, W, Cp, int(act), dt_of_dtype(w_packed.dtype),
         timer_name="sfod_conv_fwd", flops=2.0 * B * Ho * Wo * 64 * 147, tag=":stem")
    return y


def maxpool3s2(x):
    B, H, W, C = x.shape
    y = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C, dtype=x.dtype, device=x.device)
    call("sfod_maxpool3s2", x, y, B, H, W, C, dt_of(x))
    return y


def cast(src, dtype):
    if src.dtype == dtype:
        return src
    dst = torch.empty(src.shape, dtype=dtype, device=src.device)
    call("sfod_cast", src.contiguous(), dst, src.numel(), dt_of(src), dt_of_dtype(dtype))
    return dst


# ---- detection ops -----------------------------------------------------------------------------
BOX_REG_LOSS_TYPES = {"smooth_l1": 0, "giou": 1}      # loss_type of the ``*_opt`` entry points (include/sfod_hip.h)


class BoxRegOptions:
    """Box-regression options of one head, as the ``sfod_*_opt`` entry points take them: Box2BoxTransform ``weights``
    (wx, wy, ww, wh), ``loss_type`` ("smooth_l1" / "giou"), smooth-L1 ``beta`` and, for the ROI head, ``cls_agnostic``
    (one delta quadruple per row).  The wrappers below take ``box_reg=None`` for the default entry points and an instance
    for the general forms (which, given the default values, compute the same bits)."""
    __slots__ = ("weights", "loss_type", "beta", "cls_agnostic")

    def __init__(self, weights, loss_type="smooth_l1", beta=0.0, cls_agnostic=False):
        self.weights = tuple(float(w) for w in weights)
        assert len(self.weights) == 4
        self.loss_type, self.beta, self.cls_agnostic = str(loss_type), float(beta), bool(cls_agnostic)

    def is_default(self, weights):
        return (self.weights == tuple(float(w) for w in weights) and self.loss_type == "smooth_l1" and self.beta == 0.0
                and not self.cls_agnostic)

    def pred_cols(self, K):
        """columns of a Fast R-CNN prediction row: K + 1 scores and 4 (class-agnostic) or 4K deltas"""
        return K + 5 if self.cls_agnostic else 5 * K + 1

    def __repr__(self):
        return f"BoxRegOptions({self.weights}, {self.loss_type!r}, beta={self.beta}, cls_agnostic={self.cls_agnostic})"


CLS_LOSS_KINDS = {"CrossEntropy": 0, "FocalLoss": 1}      # cls_mode of the ``*_cls`` entry points; 2 = sigmoid cross-entropy


class ClsLossOptions:
    """Classification options of the Fast R-CNN head, as the ``sfod_*_cls`` entry points take them: ``kind``
    ("CrossEntropy" / "FocalLoss": MODEL.ROI_HEADS.LOSS), the focal ``gamma`` (SFOD.FOCAL_LOSS_GAMMA) and ``sigmoid``
    (MODEL.ROI_BOX_HEAD.USE_SIGMOID_CE: binary cross-entropy over the K foreground columns, probabilities by sigmoid).  The
    wrappers below take ``cls_loss=None`` for today's entry points and an instance for the ``*_cls`` forms (which, given the
    default values, compute the same bits)."""
    __slots__ = ("kind", "gamma", "sigmoid")

    def __init__(self, kind="CrossEntropy", gamma=1.5, sigmoid=False):
        self.kind, self.gamma, self.sigmoid = str(kind), float(gamma), bool(sigmoid)
        if self.kind not in CLS_LOSS_KINDS:
            raise ValueError(f"ClsLossOptions: kind must be one of {sorted(CLS_LOSS_KINDS)}, got {kind!r}")
        if self.sigmoid and self.kind != "CrossEntropy":
            raise ValueError(f"ClsLossOptions: sigmoid excludes kind {self.kind!r} (the focal loss is defined on the softmax)")

    @property
    def mode(self):
        return 2 if self.sigmoid else CLS_LOSS_KINDS[self.kind]

    def is_default(self):
        return self.kind == "CrossEntropy" and not self.sigmoid

    def __repr__(self):
        return f"ClsLossOptions({self.kind!r}, gamma={self.gamma}, sigmoid={self.sigmoid})"


def _box_reg_args(box_reg):
    """(wx, wy, ww, wh, cls_agnostic) of a ROI head's ``box_reg`` (None: Detectron2's defaults, what the plain entry points run)"""
    return (*(box_reg.weights if box_reg is not None else (10.0, 10.0, 5.0, 5.0)),
            int(box_reg.cls_agnostic) if box_reg is not None else 0)


_RPN_UNIT_WEIGHTS = (1.0, 1.0, 1.0, 1.0)


def rpn_decode(rpn_out, cell, B, Hf, Wf, stride, sizes, flags, box_reg=None, shift=0.0):
    """``shift`` (here, in ``anchor_match`` and in ``rpn_loss``): MODEL.ANCHOR_GENERATOR.OFFSET * stride as the product of two python
    doubles; ctypes rounds it to float32 once at the call (include/sfod_hip.h)"""
    A = cell.shape[0]
    NA = Hf * Wf * A
    props = torch.empty(B, NA, 4, dtype=torch.float32, device=rpn_out.device)
    scores = torch.empty(B, NA, dtype=torch.float32, device=rpn_out.device)
    if shift != 0.0:
        call("sfod_rpn_decode_shift", rpn_out, rpn_out.shape[-1], cell, A, B, Hf, Wf, stride, sizes, props, scores, flags,
             *(box_reg.weights if box_reg is not None else _RPN_UNIT_WEIGHTS), float(shift))
    elif box_reg is None:
        call("sfod_rpn_decode", rpn_out, rpn_out.shape[-1], cell, A, B, Hf, Wf, stride, sizes, props, scores, flags)
    else:
        call("sfod_rpn_decode_opt", rpn_out, rpn_out.shape[-1], cell, A, B, Hf, Wf, stride, sizes, props, scores, flags,
             *box_reg.weights)
    return props, scores


_sort_ws = {}


def segmented_sort_desc(keys):
    """keys fp32 [B,n] -> (sorted_keys [B,n], idx int32 [B,n]); stable."""
    B, n = keys.shape
    dev = keys.device
    nbytes = query("sfod_sort_ws_bytes", B, n)
    # per stream: the teacher's side stream and the main stream may both sort.  Grow-only (not one buffer per size): with
    # multi-scale / cropped training frames (data/weak_augment.py) the sizes change from step to step
    k = (dev, _stream())
    ws = _sort_ws.get(k)
    if ws is None or ws.numel() < nbytes:
        ws = _sort_ws[k] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out_keys = torch.empty_like(keys)
    out_idx = torch.empty(B, n, dtype=torch.int32, device=dev)
    call("sfod_segmented_sort_desc", keys, B, n, out_keys, out_idx, ws, nbytes)
    return out_keys, out_idx


def rpn_gather_topk(props, sorted_scores, sorted_idx, k, min_size=0.0):
    """``min_size``: MODEL.PROPOSAL_GENERATOR.MIN_SIZE -- valid = wider AND taller than it, strict"""
    B, NA, _ = props.shape
    dev = props.device
    cb = torch.empty(B, k, 4, dtype=torch.float32, device=dev)
    cs = torch.empty(B, k, dtype=torch.float32, device=dev)
    cv = torch.empty(B, k, dtype=torch.uint8, device=dev)
    if min_size == 0.0:
        call("sfod_rpn_gather_topk", props, sorted_scores, sorted_idx, B, NA, k, cb, cs, cv)
    else:
        call("sfod_rpn_gather_topk_opt", props, sorted_scores, sorted_idx, B, NA, k, float(min_size), cb, cs, cv)
    return cb, cs, cv


_mask_ws = {}


def nms(boxes, thr, max_keep, valid=None, n_per_image=None, alt_boxes=None, classes=None, mode=None):
    """boxes fp32 [B,n,4] sorted by descending score -> (keep_idx int32 [B,max_keep], count [B])."""
    B, n, _ = boxes.shape
    dev = boxes.device
    nbytes = max(8, query("sfod_nms_mask_bytes", B, n))
    k = (dev, _stream())              # per stream: two streams may run NMS at once; grow-only, like the sort's
    mask = _mask_ws.get(k)
    if mask is None or mask.numel() * 8 < nbytes:
        mask = _mask_ws[k] = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    keep_idx = torch.zeros(B, max_keep, dtype=torch.int32, device=dev)
    keep_count = torch.zeros(B, dtype=torch.int32, device=dev)
    call("sfod_nms", boxes, alt_boxes, classes, mode, valid, n_per_image, B, n, float(thr), max_keep, mask,
         keep_idx, keep_count)
    return keep_idx, keep_count


def gather_kept(cand_boxes, cand_scores, keep_idx, keep_count):
    B, n, _ = cand_boxes.shape
    max_keep = keep_idx.shape[1]
    ob = torch.empty(B, max_keep, 4, dtype=torch.float32, device=cand_boxes.device)
    os_ = torch.empty(B, max_keep, dtype=torch.float32, device=cand_boxes.device)
    call("sfod_gather_kept", cand_boxes, cand_scores, keep_idx, keep_count, B, n, max_keep, ob, os_)
    return ob, os_


def anchor_match(cell, B, Hf, Wf, stride, gt_boxes, gt_count, lo, hi, shift=0.0, boundary_thresh=-1.0, sizes=None):
    """``boundary_thresh`` >= 0 (MODEL.RPN.BOUNDARY_THRESH): anchors not inside the image grown by it get label -1; it needs
    ``sizes``, int32 [B, 2] as (h, w) on the device"""
    A = cell.shape[0]
    NA = Hf * Wf * A
    dev = gt_boxes.device
    gcap = gt_boxes.shape[1]
    matched = torch.empty(B, NA, dtype=torch.int32, device=dev)
    labels = torch.empty(B, NA, dtype=torch.int8, device=dev)
    scratch = torch.empty(B * gcap + B * NA, dtype=torch.float32, device=dev)
    if shift == 0.0 and boundary_thresh < 0:
        call("sfod_anchor_match", cell, A, B, Hf, Wf, stride, gt_boxes, gt_count, gcap, float(lo), float(hi),
             matched, labels, scratch)
    else:
        call("sfod_anchor_match_opt", cell, A, B, Hf, Wf, stride, gt_boxes, gt_count, gcap, float(lo), float(hi),
             float(shift), float(boundary_thresh), sizes if boundary_thresh >= 0 else None, matched, labels, scratch)
    return matched, labels


def roi_match(boxes, box_count, gt_boxes, gt_classes, gt_count, thr, num_classes, lo=None):
    """``lo``: lower end of an ignore band [lo, thr) (MODEL.ROI_HEADS.IOU_THRESHOLDS [lo, thr] / IOU_LABELS [0, -1, 1]): ROIs
    whose best IoU falls in it get class -1 and are never sampled.  None: the one-threshold form [thr] / [0, 1]."""
    B, P, _ = boxes.shape
    matched = torch.empty(B, P, dtype=torch.int32, device=boxes.device)
    cls = torch.empty(B, P, dtype=torch.int32, device=boxes.device)
    if lo is None:
        call("sfod_roi_match", boxes, box_count, B, P, gt_boxes, gt_classes, gt_count, gt_boxes.shape[1],
             float(thr), num_classes, matched, cls)
    else:
        call("sfod_roi_match_opt", boxes, box_count, B, P, gt_boxes, gt_classes, gt_count, gt_boxes.shape[1],
             float(lo), float(thr), num_classes, matched, cls)
    return matched, cls


def positive_quota(num, pos_frac):
    """``int(num * positive_fraction)`` in double, as d2's subsample_labels evaluates it from the configured values"""
    q = int(num * float(pos_frac))
    if not 0 <= q <= num:
        raise ValueError(f"POSITIVE_FRACTION {pos_frac} of BATCH_SIZE_PER_IMAGE {num}: the positive quota {q} is outside [0, {num}]")
    return q


def subsample_rpn_(labels, keys, num, pos_frac):
    B, n = labels.shape
    counts = torch.empty(B, 2, dtype=torch.int32, device=labels.device)
    call("sfod_subsample_quota", labels, keys, B, n, num, positive_quota(num, pos_frac), 0, 0, None, counts)
    return labels, counts


def subsample_roi(cls, keys, num, pos_frac, bg_label):
    B, n = cls.shape
    idx = torch.zeros(B, num, dtype=torch.int32, device=cls.device)
    cnt = torch.empty(B, dtype=torch.int32, device=cls.device)
    call("sfod_subsample_quota", cls, keys, B, n, num, positive_quota(num, pos_frac), bg_label, 1, idx, cnt)
    return idx, cnt


def rpn_loss(rpn_out, cell, B, Hf, Wf, stride, labels, matched, gt_boxes, gt_count, batch_per_image,
             grad_scale=None, box_reg=None, shift=0.0):
    A = cell.shape[0]
    NA = Hf * Wf * A
    dev = rpn_out.device
    loss = torch.empty(2, dtype=torch.float32, device=dev)
    nblk = (NA + 255) // 256 * B
    ws = torch.empty(nblk * 2, dtype=torch.float32, device=dev)
    d_out = torch.empty_like(rpn_out) if grad_scale is not None else None
    if shift != 0.0:
        br = box_reg if box_reg is not None else BoxRegOptions(_RPN_UNIT_WEIGHTS)
        call("sfod_rpn_loss_shift", rpn_out, rpn_out.shape[-1], cell, A, B, Hf, Wf, stride, labels, matched, gt_boxes,
             gt_count, gt_boxes.shape[1], batch_per_image, loss, grad_scale, d_out, ws, *br.weights,
             BOX_REG_LOSS_TYPES[br.loss_type], br.beta, float(shift))
    elif box_reg is None:
        call("sfod_rpn_loss", rpn_out, rpn_out.shape[-1], cell, A, B, Hf, Wf, stride, labels, matched, gt_boxes,
             gt_count, gt_boxes.shape[1], batch_per_image, loss, grad_scale, d_out, ws)
    else:
        call("sfod_rpn_loss_opt", rpn_out, rpn_out.shape[-1], cell, A, B, Hf, Wf, stride, labels, matched, gt_boxes,
             gt_count, gt_boxes.shape[1], batch_per_image, loss, grad_scale, d_out, ws, *box_reg.weights,
             BOX_REG_LOSS_TYPES[box_reg.loss_type], box_reg.beta)
    return loss, d_out


def append_gt(props, prop_count, gt_boxes, gt_count):
    B, P, _ = props.shape
    gcap = gt_boxes.shape[1]
    out = torch.empty(B, P + gcap, 4, dtype=torch.float32, device=props.device)
    cnt = torch.empty(B, dtype=torch.int32, device=props.device)
    call("sfod_append_gt", props, prop_count, B, P, gt_boxes, gt_count, gcap, out, cnt)
    return out, cnt


def roi_build_samples(boxes, cls, matched, samp_idx, samp_count, gt_boxes, gt_count):
    B, P, _ = boxes.shape
    S = samp_idx.shape[1]
    dev = boxes.device
    rois = torch.empty(B * S, 5, dtype=torch.float32, device=dev)
    gt_cls = torch.empty(B * S, dtype=torch.int32, device=dev)
    gt_box = torch.empty(B * S, 4, dtype=torch.float32, device=dev)
    n_valid = torch.empty(1, dtype=torch.int32, device=dev)
    call("sfod_roi_build_samples", boxes, cls, matched, samp_idx, samp_count, B, P, S, gt_boxes, gt_count,
         gt_boxes.shape[1], rois, gt_cls, gt_box, n_valid)
    return rois, gt_cls, gt_box, n_valid


def make_rois(props, prop_count):
    B, P, _ = props.shape
    rois = torch.empty(B * P, 5, dtype=torch.float32, device=props.device)
    call("sfod_make_rois", props, prop_count, B, P, rois)
    return rois


def roi_align_fwd(feat, rois, pooled, scale, sampling_ratio=0, aligned=True):
    """``(sampling_ratio, aligned) = (0, True)``: the default entry point; anything else: ``sfod_roi_align_fwd_opt``."""
    B, H, W, C = feat.shape
    R = rois.shape[0]
    out = torch.empty(R, pooled * pooled, C, dtype=feat.dtype, device=feat.device)
    if sampling_ratio == 0 and bool(aligned):
        call("sfod_roi_align_fwd", feat, B, H, W, C, rois, R, pooled, float(scale), out, dt_of(feat))
    else:
        call("sfod_roi_align_fwd_opt", feat, B, H, W, C, rois, R, pooled, float(scale), int(sampling_ratio), int(aligned),
             out, dt_of(feat))
    return out


def roi_align_bwd(dout, rois, feat_shape, pooled, scale, dfeat=None, sampling_ratio=0, aligned=True):
    B, H, W, C = feat_shape
    if dfeat is None:
        dfeat = torch.zeros(B, H, W, C, dtype=torch.float32, device=dout.device)
    if sampling_ratio == 0 and bool(aligned):
        call("sfod_roi_align_bwd", dout, B, H, W, C, rois, rois.shape[0], pooled, float(scale), dfeat, dt_of(dout))
    else:
        call("sfod_roi_align_bwd_opt", dout, B, H, W, C, rois, rois.shape[0], pooled, float(scale), int(sampling_ratio),
             int(aligned), dfeat, dt_of(dout))
    return dfeat


def frcnn_loss(pred, K, rois, gt_cls, gt_box, n_valid, grad_scale=None, box_reg=None, cls_loss=None):
    R, ld = pred.shape
    dev = pred.device
    loss = torch.empty(2, dtype=torch.float32, device=dev)
    # per block two partials; the ``_cls`` form's modes 1 and 2 keep the class partial as a pair of floats: three
    ws = torch.empty(((R + 255) // 256) * (2 if cls_loss is None else 3), dtype=torch.float32, device=dev)
    d_pred = torch.empty_like(pred) if grad_scale is not None else None
    if cls_loss is not None:
        w = _box_reg_args(box_reg)
        call("sfod_frcnn_loss_cls", pred, ld, R, K, rois, gt_cls, gt_box, n_valid, loss, grad_scale, d_pred, ws, *w[:4],
             BOX_REG_LOSS_TYPES[box_reg.loss_type] if box_reg is not None else 0, box_reg.beta if box_reg is not None else 0.0,
             w[4], cls_loss.mode, cls_loss.gamma)
    elif box_reg is None:
        call("sfod_frcnn_loss", pred, ld, R, K, rois, gt_cls, gt_box, n_valid, loss, grad_scale, d_pred, ws)
    else:
        call("sfod_frcnn_loss_opt", pred, ld, R, K, rois, gt_cls, gt_box, n_valid, loss, grad_scale, d_pred, ws,
             *box_reg.weights, BOX_REG_LOSS_TYPES[box_reg.loss_type], box_reg.beta, int(box_reg.cls_agnostic))
    return loss, d_pred


def _logit_column(z):
    """(tensor, rows, ld) of a one-channel fp32 logit matrix [..., ld] (the GEMM's output under ldy)"""
    assert z.dtype == torch.float32 and z.is_contiguous()
    ld = z.shape[-1]
    return z, z.numel() // ld, ld


def da_bce(z, label, rois=None, grad_scale=None):
    """BCE-with-logits of column 0 of ``z`` [..., ld] against the constant ``label``, mean over the live rows (``rois``:
    rows with batch index -1 are padding) -> (loss [2] = (value, live count), dz like ``z`` or None)."""
    z, n, ld = _logit_column(z)
    loss = torch.empty(2, dtype=torch.float32, device=z.device)
    ws = torch.empty(max((n + 255) // 256, 1) * 2, dtype=torch.float32, device=z.device)
    dz = torch.empty_like(z) if grad_scale is not None else None
    call("sfod_da_bce", z, n, ld, rois, float(label), loss, grad_scale, dz, ws)
    return loss, dz


def da_consistency_fwd(z_img, z_ins, rois, pooled, scale, sampling_ratio=0, aligned=True):
    """z_img [B, H, W, ld], z_ins [R, ld'] (column 0 each), rois [R, 5] -> (loss [2] = (value, live count), state for
    ``da_consistency_bwd``).  ``state["p_img"]``: the per-ROI mean of ROIAlign(sigmoid(z_img))."""
    B, H, W, ld = z_img.shape
    R, ld_ins = z_ins.shape
    assert z_img.dtype == torch.float32 and z_ins.dtype == torch.float32 and rois.shape == (R, 5)
    dev = z_img.device
    loss = torch.empty(2, dtype=torch.float32, device=dev)
    per_roi = torch.empty(3, max(R, 1), dtype=torch.float32, device=dev)      # p_img | sgn | term
    wts = torch.empty(max(R, 1), H + W, dtype=torch.float32, device=dev)
    call("sfod_da_consistency_fwd", z_img, B, H, W, ld, z_ins, ld_ins, rois, R, int(pooled), float(scale),
         int(sampling_ratio), int(aligned), loss, per_roi[0], per_roi[1], per_roi[2], wts)
    return loss, {"loss": loss, "p_img": per_roi[0, :R], "sgn": per_roi[1], "wts": wts}


def da_consistency_bwd(z_img, z_ins, rois, state, grad_scale):
    """-> (dz_img like z_img, dz_ins like z_ins): dense, the padding columns zero"""
    B, H, W, ld = z_img.shape
    R, ld_ins = z_ins.shape
    dz_img, dz_ins = torch.empty_like(z_img), torch.empty_like(z_ins)
    call("sfod_da_consistency_bwd", z_img, B, H, W, ld, z_ins, ld_ins, rois, R, state["loss"], state["sgn"], state["wts"],
         grad_scale, dz_img, dz_ins)
    return dz_img, dz_ins


def cda_condition_fwd(f, scores, C, rois, entropy=False, out_dtype=None, with_grad_operand=False):
    """Box features ``f`` [R, D] (any storage type), fp32 ``scores`` [R, ld] (the first ``C`` columns live), ``rois`` [R, 5] ->
    (x [R, C * D] of ``out_dtype`` (default: f's), x_grad, p [R, C], w [R]): x[r, c * D + d] = softmax(scores)[r, c] * f[r, d],
    written as the next GEMM's operand; ``x_grad``: what that GEMM's weight gradient reads -- x itself, or for half pairs the
    same values as bf16 pairs from the same pass (None without ``with_grad_operand``); w = 1 + exp(-entropy(p)) with
    ``entropy``, else 1.  Padding rows (batch index < 0) are zero everywhere."""
    R, D = f.shape
    assert scores.dtype == torch.float32 and scores.dim() == 2 and scores.shape[0] == R and rois.shape == (R, 5)
    dev = f.device
    x = torch.empty(R, C * D, dtype=out_dtype or f.dtype, device=dev)
    x2 = torch.empty(R, C * D, dtype=SPLIT_DTYPE, device=dev) if (with_grad_operand and x.dtype == SPLITH_DTYPE) else None
    p = torch.empty(R, C, dtype=torch.float32, device=dev)
    w = torch.empty(R, dtype=torch.float32, device=dev)
    call("sfod_cda_condition_fwd", f, dt_of(f), scores, scores.shape[1], rois, R, D, C, int(bool(entropy)), x, dt_of(x), x2, p, w)
    return x, ((x2 if x2 is not None else x) if with_grad_operand else None), p, w


def cda_condition_bwd(dx, p, rois):
    """dx [R, C * D] (fp32 or bf16), p [R, C] -> df [R, D] = sum_c p[:, c] * dx[:, c * D:(c + 1) * D], padding rows 0"""
    R, C = p.shape
    D = dx.shape[1] // C
    assert dx.shape == (R, C * D) and rois.shape == (R, 5)
    df = torch.empty(R, D, dtype=dx.dtype, device=dx.device)
    call("sfod_cda_condition_bwd", dx, dt_of(dx), p, rois, R, D, C, df)
    return df


def da_bce_weighted(z, label, weight, rois=None, grad_scale=None):
    """``da_bce`` with a weight per row: the weighted mean ``sum w bce / sum w`` over the live rows and its gradient."""
    z, n, ld = _logit_column(z)
    assert weight.dtype == torch.float32 and weight.numel() == n
    loss = torch.empty(2, dtype=torch.float32, device=z.device)
    ws = torch.empty(query("sfod_da_bce_weighted_ws_floats", n), dtype=torch.float32, device=z.device)
    dz = torch.empty_like(z) if grad_scale is not None else None
    call("sfod_da_bce_weighted", z, n, ld, rois, weight, float(label), loss, grad_scale, dz, ws)
    return loss, dz


def frcnn_inference(pred, K, props, prop_count, sizes, score_thresh, nms_thresh, max_det, pseudo_thr,
                    numel_limit=20000, box_reg=None, cls_loss=None):
    """Teacher post-processing -> dict of fixed-capacity per-image arrays + counts."""
    B, P, _ = props.shape
    dev = pred.device
    n = P * K
    cb = torch.empty(B, n, 4, dtype=torch.float32, device=dev)
    cs = torch.empty(B, n, dtype=torch.float32, device=dev)
    cc = torch.empty(B, dtype=torch.int32, device=dev)
    if cls_loss is not None:
        call("sfod_frcnn_candidates_cls", pred, pred.shape[-1], B, P, K, props, prop_count, sizes, float(score_thresh),
             cb, cs, cc, *_box_reg_args(box_reg), cls_loss.mode, cls_loss.gamma)
    elif box_reg is None:
        call("sfod_frcnn_candidates", pred, pred.shape[-1], B, P, K, props, prop_count, sizes, float(score_thresh),
             cb, cs, cc)
    else:
        call("sfod_frcnn_candidates_opt", pred, pred.shape[-1], B, P, K, props, prop_count, sizes, float(score_thresh),
             cb, cs, cc, *box_reg.weights, int(box_reg.cls_agnostic))
    ss, si = segmented_sort_desc(cs)
    sb = torch.empty(B, n, 4, dtype=torch.float32, device=dev)
    sa = torch.empty(B, n, 4, dtype=torch.float32, device=dev)
    sc = torch.empty(B, n, dtype=torch.int32, device=dev)
    mode = torch.empty(B, dtype=torch.int32, device=dev)
    mx = torch.empty(B, dtype=torch.float32, device=dev)
    call("sfod_frcnn_prepare_nms", cb, ss, si, cc, B, n, K, numel_limit, sb, sa, sc, mode, mx)
    keep_idx, keep_count = nms(sb, nms_thresh, max_det, n_per_image=cc, alt_boxes=sa, classes=sc, mode=mode)
    out = {
        "det_boxes": torch.empty(B, max_det, 4, dtype=torch.float32, device=dev),
        "det_scores": torch.empty(B, max_det, dtype=torch.float32, device=dev),
        "det_classes": torch.empty(B, max_det, dtype=torch.int32, device=dev),
        "det_count": torch.empty(B, dtype=torch.int32, device=dev),
        "gt_boxes": torch.empty(B, max_det, 4, dtype=torch.float32, device=dev),
        "gt_classes": torch.empty(B, max_det, dtype=torch.int32, device=dev),
        "gt_count": torch.empty(B, dtype=torch.int32, device=dev),
        "cand_count": cc, "mode": mode,
    }
    call("sfod_frcnn_finalize", sb, ss, sc, keep_idx, keep_count, B, n, max_det, float(pseudo_thr),
         out["det_boxes"], out["det_scores"], out["det_classes"], out["det_count"], out["gt_boxes"],
         out["gt_classes"], out["gt_count"])
    return out


TTA_ROW = 8               # floats per (image, augmentation) row of sfod_tta_merge's table
TTA_MAX_AUG, TTA_MAX_CAND = 64, 4096      # include/sfod_hip.h: A <= 64, A * cap <= 4096


def tta_merge_candidates(det_boxes, det_scores, det_classes, det_count, aug_table, sizes, K, score_thresh):
    """sfod_tta_merge: containers of B images x A augmentations ([B,A,cap,4] / [B,A,cap] / [B,A,cap] i32 / [B,A] i32), the
    transform table [B,A,8] fp32 and (H0, W0) [B,2] i32 -> compact candidates in the original frame, concatenation order:
    (cand_boxes [B,A*cap,4], cand_scores [B,A*cap] with -1 in filtered slots, cand_classes [B,A*cap] i32, cand_count [B])."""
    B, A, cap = det_scores.shape
    dev = det_boxes.device
    assert det_boxes.dtype == torch.float32 and det_scores.dtype == torch.float32 and aug_table.dtype == torch.float32
    assert det_classes.dtype == torch.int32 and det_count.dtype == torch.int32 and sizes.dtype == torch.int32
    assert det_boxes.shape == (B, A, cap, 4) and det_classes.shape == (B, A, cap) and det_count.shape == (B, A)
    assert aug_table.shape == (B, A, TTA_ROW) and sizes.shape == (B, 2)
    n = A * cap
    cb = torch.empty(B, n, 4, dtype=torch.float32, device=dev)
    cs = torch.empty(B, n, dtype=torch.float32, device=dev)
    ck = torch.empty(B, n, dtype=torch.int32, device=dev)
    cc = torch.empty(B, dtype=torch.int32, device=dev)
    call("sfod_tta_merge", det_boxes, det_scores, det_classes, det_count, aug_table, sizes, B, A, cap, int(K),
         float(score_thresh), cb, cs, ck, cc)
    return cb, cs, ck, cc


def tta_merge(det_boxes, det_scores, det_classes, det_count, aug_table, sizes, K, score_thresh, nms_thresh, max_det,
              numel_limit=20000):
    """The whole merge of test-time augmentation on the device: sfod_tta_merge, then the teacher post-processing's own
    sort -> prepare (compact form) -> class-wise NMS -> top ``max_det``.  -> dict of det_boxes [B,max_det,4], det_scores,
    det_classes, det_count at (H0, W0), plus the candidates (``cand_*``) for whoever checks them."""
    cb, cs, ck, cc = tta_merge_candidates(det_boxes, det_scores, det_classes, det_count, aug_table, sizes, K, score_thresh)
    B, n = cs.shape
    dev = cs.device
    ss, si = segmented_sort_desc(cs)
    sb = torch.empty(B, n, 4, dtype=torch.float32, device=dev)
    sa = torch.empty(B, n, 4, dtype=torch.float32, device=dev)
    sc = torch.empty(B, n, dtype=torch.int32, device=dev)
    mode = torch.empty(B, dtype=torch.int32, device=dev)
    mx = torch.empty(B, dtype=torch.float32, device=dev)
    call("sfod_frcnn_prepare_nms_cls", cb, ck, si, cc, B, n, int(numel_limit), sb, sa, sc, mode, mx)
    keep_idx, keep_count = nms(sb, nms_thresh, max_det, n_per_image=cc, alt_boxes=sa, classes=sc, mode=mode)
    out = {
        "det_boxes": torch.empty(B, max_det, 4, dtype=torch.float32, device=dev),
        "det_scores": torch.empty(B, max_det, dtype=torch.float32, device=dev),
        "det_classes": torch.empty(B, max_det, dtype=torch.int32, device=dev),
        "det_count": torch.empty(B, dtype=torch.int32, device=dev),
        "cand_boxes": cb, "cand_scores": cs, "cand_classes": ck, "cand_count": cc, "mode": mode,
    }
    # (the pseudo-label outputs of the finalize kernel are not wanted here: a threshold nothing passes, scratch arrays)
    gb = torch.empty(B, max_det, 4, dtype=torch.float32, device=dev)
    gc = torch.empty(B, max_det, dtype=torch.int32, device=dev)
    gn = torch.empty(B, dtype=torch.int32, device=dev)
    call("sfod_frcnn_finalize", sb, ss, sc, keep_idx, keep_count, B, n, max_det, float("inf"), out["det_boxes"],
         out["det_scores"], out["det_classes"], out["det_count"], gb, gc, gn)
    return out


def bpc_loss(pred, K, rois, roi_cls, sizes_dev, gt_boxes, gt_classes, gt_count, iou_thresh=0.5, box_reg=None,
             cls_loss=None):
    """BPC calibration scalar of one training pass (fused convert_bbox_scores + bpc_loss) -> 0-dim tensor."""
    B, G = gt_classes.shape
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    ws = torch.empty(max(B, 1) * 4, dtype=torch.float64, device=pred.device)
    if cls_loss is not None:
        call("sfod_bpc_loss_cls", pred, pred.shape[-1], pred.shape[0], K, rois, roi_cls, B, sizes_dev, gt_boxes,
             gt_classes, gt_count, G, float(iou_thresh), loss, ws, *_box_reg_args(box_reg), cls_loss.mode,
             cls_loss.gamma)
    elif box_reg is None:
        call("sfod_bpc_loss", pred, pred.shape[-1], pred.shape[0], K, rois, roi_cls, B, sizes_dev, gt_boxes, gt_classes,
             gt_count, G, float(iou_thresh), loss, ws)
    else:
        call("sfod_bpc_loss_opt", pred, pred.shape[-1], pred.shape[0], K, rois, roi_cls, B, sizes_dev, gt_boxes,
             gt_classes, gt_count, G, float(iou_thresh), loss, ws, *box_reg.weights, int(box_reg.cls_agnostic))
    return loss[0]


def f1_count(det_boxes, det_scores, det_classes, det_count, gt_boxes, gt_classes, gt_count, scale, clip_size, K,
             iou=0.5, top_n=5, score=0.5):
    """F1Evaluator's per-image, per-class (TP, FP, FN) of a batch of fixed-capacity arrays -> [B, K, 3] int32 (no host
    synchronisation; include/sfod_hip.h: sfod_f1_count)."""
    B, D = det_scores.shape
    G = gt_classes.shape[1]
    assert det_boxes.dtype == torch.float32 and det_scores.dtype == torch.float32 and gt_boxes.dtype == torch.float32
    assert det_classes.dtype == torch.int32 and det_count.dtype == torch.int32
    assert gt_classes.dtype == torch.int32 and gt_count.dtype == torch.int32
    assert scale.dtype == torch.float32 and clip_size.dtype == torch.int32
    assert det_boxes.shape == (B, D, 4) and det_classes.shape == (B, D) and gt_boxes.shape == (B, G, 4)
    assert det_count.shape == (B,) and gt_count.shape == (B,) and scale.shape == (B, 2) and clip_size.shape == (B, 2)
    counts = torch.empty(B, K, 3, dtype=torch.int32, device=det_boxes.device)
    call("sfod_f1_count", det_boxes, det_scores, det_classes, det_count, gt_boxes, gt_classes, gt_count, scale, clip_size,
         B, D, G, K, float(iou), int(top_n), float(score), counts)
    return counts


COCO_MAX_DET, COCO_MAX_GT, COCO_MAX_BITS = 100, 256, 64      # include/sfod_hip.h: D <= 100, G <= 256, A * T <= 64


def coco_match(det_boxes, det_scores, det_classes, det_count, gt_boxes, gt_area, gt_classes, gt_iscrowd, gt_count, K,
               iou_thrs, area_rng, out=None):
    """COCOeval's matching of a batch of fixed-capacity arrays (include/sfod_hip.h: sfod_coco_match; no host synchronisation)
    -> (rank [B,D] i32, match [B,D] i64, ignore [B,D] i64, npig [B,K,A] i32); bit ``a * T + t`` of the two 64-bit words
    belongs to area range ``a`` and threshold ``t`` (torch has no arithmetic on uint64: the words are held as int64).
    ``iou_thrs`` [T] and ``area_rng`` [A][2] are host doubles, handed over by value.  ``out``: the four tensors to write."""
    B, D = det_scores.shape
    G = gt_classes.shape[1]
    thrs = [float(t) for t in iou_thrs]
    rng = [float(v) for lo_hi in area_rng for v in lo_hi]
    T, A = len(thrs), len(rng) // 2
    assert len(rng) == 2 * A
    thrs_c, rng_c = (ctypes.c_double * T)(*thrs), (ctypes.c_double * (2 * A))(*rng)      # read by the call itself
    assert det_boxes.dtype == torch.float32 and det_scores.dtype == torch.float32 and det_classes.dtype == torch.int32
    assert gt_boxes.dtype == torch.float64 and gt_area.dtype == torch.float64 and gt_classes.dtype == torch.int32
    assert gt_iscrowd.dtype == torch.int32 and det_count.dtype == torch.int32 and gt_count.dtype == torch.int32
    assert det_boxes.shape == (B, D, 4) and det_classes.shape == (B, D) and det_count.shape == (B,)
    assert gt_boxes.shape == (B, G, 4) and gt_area.shape == (B, G) and gt_iscrowd.shape == (B, G) and gt_count.shape == (B,)
    dev = det_boxes.device
    ins = (det_boxes, det_scores, det_classes, det_count, gt_boxes, gt_area, gt_classes, gt_iscrowd, gt_count)
    # the kernel indexes dense arrays and loads a detection's box as one 16-byte word (call() checks contiguity too)
    assert all(t.is_contiguous() and t.device == dev for t in ins), "coco_match: dense tensors of one device"
    if out is None:
        out = (torch.empty(B, D, dtype=torch.int32, device=dev), torch.empty(B, D, dtype=torch.int64, device=dev),
               torch.empty(B, D, dtype=torch.int64, device=dev), torch.empty(B, int(K), A, dtype=torch.int32, device=dev))
    rank, match, ignore, npig = out
    assert rank.dtype == torch.int32 and match.dtype == torch.int64 and ignore.dtype == torch.int64 and npig.dtype == torch.int32
    assert rank.shape == (B, D) and match.shape == (B, D) and ignore.shape == (B, D) and npig.shape == (B, int(K), A)
    assert all(t.is_contiguous() and t.device == dev for t in out), "coco_match: dense outputs on the inputs' device"
    call("sfod_coco_match", det_boxes, det_scores, det_classes, det_count, gt_boxes, gt_area, gt_classes, gt_iscrowd,
         gt_count, B, D, G, int(K), ctypes.addressof(thrs_c), T, ctypes.addressof(rng_c), A, rank, match, ignore, npig)
    return rank, match, ignore, npig


def predict_probs(scores, cls_loss=None):
    """Row softmax of the class scores [R, K+1] (any row stride) in the teacher post-processing kernel's operation order;
    under ``cls_loss.sigmoid`` the sigmoid of every score."""
    assert scores.is_cuda, "native ops need device tensors"
    assert scores.dim() == 2 and scores.dtype == torch.float32 and scores.stride(1) == 1
    R, n = scores.shape
    out = torch.empty(R, n, dtype=torch.float32, device=scores.device)
    # (rows may be a strided view of the prediction matrix: the pointer goes in as is, the row stride as ld)
    if cls_loss is not None:
        call("sfod_predict_probs_cls", scores.data_ptr(), scores.stride(0) if R > 1 else n, R, n - 1, cls_loss.mode,
             cls_loss.gamma, out)
    else:
        call("sfod_predict_probs", scores.data_ptr(), scores.stride(0) if R > 1 else n, R, n - 1, out)
    return out


def adaptive_pseudo_labels_(d, thr, reserve, row, class_acc, select):
    """In place on the detection dict of ``frcnn_inference``: updates ``reserve[row]`` / ``class_acc`` and, with
    ``select``, replaces ``gt_boxes`` / ``gt_classes`` / ``gt_count`` (adds ``gt_scores``) by the class-wise
    adaptive selection."""
    B, max_det = d["det_scores"].shape
    R, K = reserve.shape
    if "gt_scores" not in d:
        d["gt_scores"] = torch.zeros(B, max_det, dtype=torch.float32, device=reserve.device)
    call("sfod_adaptive_pseudo_labels", d["det_boxes"], d["det_scores"], d["det_classes"], d["det_count"], B, max_det,
         K, float(thr), reserve, R, int(row), class_acc, int(bool(select)), d["gt_boxes"], d["gt_classes"],
         d["gt_scores"], d["gt_count"])
    if select:
        d["gt_adaptive"] = True
    return d


def sgd_ema_(param, grad, mom, teacher, lr, momentum, weight_decay, grad_scale, ema_keep, first_step):
    call("sfod_sgd_ema", param, grad, mom, teacher, param.numel(), lr, float(momentum), float(weight_decay),
         float(grad_scale), float(ema_keep), float(1.0 - float(ema_keep)), int(first_step))


CLIP_TYPES = {None: 0, "value": 1, "norm": 2}      # sfod_sgd_ema_seg's clip_type
NORM_TYPES = {2.0: 0, float("inf"): 1}             # sfod_grad_clip_coef's norm_type


def grad_clip_ws(n, nseg, device):
    """Workspace of ``grad_clip_coef_`` for a flat gradient of ``n`` elements in ``nseg`` segments (allocate once)."""
    return torch.empty(query("sfod_grad_clip_ws_floats", int(n), int(nseg)), dtype=torch.float32, device=device)


def grad_clip_coef_(coef, grad, seg_off, seg_len, grad_scale, clip_value, norm_type, ws):
    """coef[s] <- clip_grad_norm_'s coefficient of segment s of ``grad * grad_scale`` (include/sfod_hip.h; two launches)."""
    assert seg_off.dtype == torch.int64 and seg_len.dtype == torch.int64 and coef.dtype == torch.float32
    assert seg_len.numel() == seg_off.numel() == coef.numel()
    call("sfod_grad_clip_coef", grad, grad.numel(), seg_off, seg_len, seg_off.numel(), float(grad_scale),
         float(clip_value), NORM_TYPES[float(norm_type)], coef, ws, ws.numel())


def sgd_ema_seg_(param, grad, mom, teacher, seg_off, seg_hp, clip_coef, lr, momentum, grad_scale, clip_type, clip_value,
                 nesterov, ema_keep, first_step):
    """``sgd_ema_`` in one launch with per-segment {weight decay, lr factor} (``seg_hp`` [nseg, 2]) and clipping:
    ``clip_type`` None / "value" / "norm" (the latter reads ``clip_coef``, see ``grad_clip_coef_``)."""
    assert seg_off.dtype == torch.int64 and seg_hp.dtype == torch.float32 and seg_hp.numel() == 2 * seg_off.numel()
    call("sfod_sgd_ema_seg", param, grad, mom, teacher, param.numel(), seg_off, seg_off.numel(), seg_hp, clip_coef, lr,
         float(momentum), float(grad_scale), CLIP_TYPES[clip_type], float(clip_value), int(bool(nesterov)),
         float(ema_keep), float(1.0 - float(ema_keep)), int(first_step))


def ema_(teacher, student, keep):
    call("sfod_ema", teacher, student, teacher.numel(), float(keep), float(1.0 - float(keep)))


def ema_i64_(teacher, student, keep):
    """int64 buffers: float32 arithmetic, truncated on the way back (the reference's EMA + load_state_dict copy)."""
    assert teacher.dtype == torch.int64 and student.dtype == torch.int64 and teacher.numel() == student.numel()
    call("sfod_ema_i64", teacher, student, teacher.numel(), float(keep), float(1.0 - keep))


def teacher_metrics(det_scores, det_count, rpn_logits, rpn_count, gt_count, thr):
    """-> float32 [3]: mean detection confidence, RPN proposals above ``thr`` per image, mean pseudo-label count."""
    B, D = det_scores.shape
    out = torch.empty(3, dtype=torch.float32, device=det_scores.device)
    call("sfod_teacher_metrics", det_scores, det_count, D, rpn_logits, rpn_count, rpn_logits.shape[1], gt_count, B,
         float(thr), out)
    return out
