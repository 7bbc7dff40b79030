"""ctypes binding of libfactorizer_hip.so, derived from its C ABI in include/factorizer_hip.h.

Argument lists, descriptor layouts and constants are built at import from what _header.py reads in the header: a new entry
point, field or constant is declared there and nowhere else.  What the header cannot say is stated below, one entry at a time
(_ARG_EXCEPTIONS, _FIELD_NAMES).

The native library is the product path for device tensors.  There is no silent fallback: if a
device tensor reaches an op and the library cannot be loaded, `lib()` raises.
"""
from __future__ import annotations

import ctypes
import os
import threading

import torch

from . import _header
from ._header import NativeError  # noqa: F401  (the package's one error type of the native path)

_HERE = os.path.dirname(os.path.abspath(__file__))
# FZ_LIB_PATH: diagnostics only (A/B of two builds of this library on one box, tools/probes/build_alt.py)
LIB_PATH = os.environ.get("FZ_LIB_PATH") or os.path.join(_HERE, "libfactorizer_hip.so")

_H = _header.read()


def constants(*names):
    """the values of the header's `#define FZ_<name>`, in the order asked for"""
    return tuple(_H.defines["FZ_" + n] for n in names)


FZ_OK, FZ_E_UNSUPPORTED = constants("OK", "E_UNSUPPORTED")
ABI_VERSION, = constants("ABI_VERSION")   # lib() loads only a library that was built from this header
SOLVER_ID = dict(zip(("mu", "hals", "cd", "smu"), constants("SOLVER_MU", "SOLVER_HALS", "SOLVER_CD", "SOLVER_SMU")))
STORE_F32, STORE_BF16 = constants("STORE_F32", "STORE_BF16")
# the `products` field of the descriptors
PRODUCTS_DEFAULT, PRODUCTS_SPLIT_BF16, PRODUCTS_FP32_MFMA = constants("PRODUCTS_DEFAULT", "PRODUCTS_SPLIT_BF16", "PRODUCTS_FP32_MFMA")
SEG_F32, SEG_BF16, SEG_U8 = constants("SEG_F32", "SEG_BF16", "SEG_U8")   # element kinds of fz_seg_counts
LABEL_U8, LABEL_I64, LABEL_F32 = constants("LABEL_U8", "LABEL_I64", "LABEL_F32")   # element kinds of a class-index label map
VOL_F32, VOL_BF16, VOL_U8, VOL_I16 = constants("VOL_F32", "VOL_BF16", "VOL_U8", "VOL_I16")
VOL_IMAGE_IN, VOL_IMAGE_OUT, VOL_LABEL_IN, VOL_LOGITS = constants("VOL_ROLE_IMAGE_IN", "VOL_ROLE_IMAGE_OUT", "VOL_ROLE_LABEL_IN",
                                                                  "VOL_ROLE_LOGITS")
RESPACE_BILINEAR, RESPACE_NEAREST = constants("RESPACE_BILINEAR", "RESPACE_NEAREST")
DROP_RES, DROP_GELU, DROP_GELU_BWD = constants("DROP_RES", "DROP_GELU", "DROP_GELU_BWD")
_products = threading.local()   # per thread: two models driven from two threads may use different pipes


def products() -> int:
    """the FZ_PRODUCTS_* value this package's layers put in their descriptors (default: the library's own default)"""
    return getattr(_products, "value", PRODUCTS_DEFAULT)


class use_products:
    """with use_products(PRODUCTS_FP32_MFMA): ...  — fp32 products of every dense layer whose FORWARD runs inside the block on
    the named pipe, through the descriptors' `products` field.  The setting is per thread; every autograd node records it in
    its ctx at forward time and re-establishes it for its backward (`capture_products` / `with_products` below), so a backward
    pass that runs after the block has exited, or on one of autograd's worker threads, multiplies on the same pipe as its
    forward did.  The C ABI has no switch to flip for this: a caller of the library sets the field per call."""

    def __init__(self, value):
        self.value = int(value)

    def __enter__(self):
        self.prev = products()
        _products.value = self.value

    def __exit__(self, *exc):
        _products.value = self.prev


# Walking order of the fused core's window launches (fz_set_tile_order, include/factorizer_hip.h): window w walks the patch
# tiles ascending for even w, descending for odd w — consecutive windows read the SAME tensors, so a window then starts where
# the previous one ended, in the part the 256 MiB Infinity Cache still holds.  FZ_TILE_ORDER=0 (read once): always ascending.
TILE_ORDER = os.environ.get("FZ_TILE_ORDER", "1") != "0"


def set_tile_order(descending: int):
    if TILE_ORDER:
        lib().fz_set_tile_order(int(descending) & 1)


def capture_products(fwd):
    """decorator of an autograd Function's forward(ctx, ...): remember the thread's products setting in the ctx"""
    import functools

    @functools.wraps(fwd)
    def wrapper(ctx, *a, **kw):
        ctx._fz_products = products()
        return fwd(ctx, *a, **kw)
    return wrapper


def with_products(bwd):
    """decorator of the matching backward(ctx, ...): run it under the setting its forward saw"""
    import functools

    @functools.wraps(bwd)
    def wrapper(ctx, *a, **kw):
        with use_products(getattr(ctx, "_fz_products", PRODUCTS_DEFAULT)):
            return bwd(ctx, *a, **kw)
    return wrapper


def act_dtype(t: torch.Tensor) -> int:
    """FZ_STORE_* code of an activation tensor (fp32, or bf16 storage with fp32 arithmetic)."""
    if t.dtype == torch.float32:
        return STORE_F32
    if t.dtype == torch.bfloat16:
        return STORE_BF16
    raise TypeError(f"native kernels take float32 or bfloat16 activations, got {t.dtype} "
                    "(float16 is refused on purpose: the NMF eps 1e-16 underflows in it, SURVEY.md §5)")

_lock = threading.Lock()
_lib = None

_c = ctypes
_i = _c.c_int
_SCALARS = {"int": _i, "int64_t": _c.c_int64, "float": _c.c_float, "double": _c.c_double}


def _ctype(t, where):
    """ctypes type of a header type, by the rules at the top of include/factorizer_hip.h"""
    if t.base in _H.structs:
        return _c.POINTER(_DESC[t.base]) if t.ptr == 1 else _c.POINTER(_c.POINTER(_DESC[t.base]))
    if t.ptr == 0:
        return _SCALARS.get(t.base, _c.c_void_p)           # fz_stream_t
    if t.ptr == 2:
        return _c.POINTER(_c.c_void_p)                     # host array of device pointers
    if t.base == "int":
        return _c.POINTER(_i)                              # host array
    if t.base == "char":                                   # only as the `const char*` a function returns
        raise NativeError(f"{where}: a char* needs an entry in _ARG_EXCEPTIONS (factorizer_amd/_native.py)")
    return _c.c_void_p                                     # device buffer


_FIELD_NAMES = {("fz_mlp_desc", "in"): "inp"}   # `in` is a Python keyword: d.in = ... does not parse


def _descriptor(name):
    """ctypes.Structure of a header struct, named like it: fz_gemm_dw_desc -> GemmDwDesc"""
    fields = [(_FIELD_NAMES.get((name, f), f), _ctype(t, f"{name}.{f}") * n if n else _ctype(t, f"{name}.{f}"))
              for t, f, n in _H.structs[name]]
    return type("".join(p.title() for p in name.split("_")[1:]), (_c.Structure,), {"_fields_": fields})


_DESC = {}
for _name in _H.structs:   # in the header's order: a field may point to a struct declared before its own
    _DESC[_name] = _descriptor(_name)
GemmDesc, MlpDesc, MlpDropout, GemmDwDesc, OutprojFac = (_DESC["fz_" + n] for n in (
    "gemm_desc", "mlp_desc", "mlp_dropout", "gemm_dw_desc", "outproj_fac"))
BlockPrologue, WgradDesc, VolGeom, RespaceGeom = (_DESC["fz_" + n] for n in (
    "block_prologue", "wgrad_desc", "vol_geom", "respace_geom"))

_ARG_EXCEPTIONS = {
    # a HOST array of up to 8 bytes that the launcher reads before the launch; by the rules a uint8_t* is a device buffer
    ("fz_vol_restore", "label_values"): _c.POINTER(_c.c_ubyte),
    # a HOST character buffer of `cap` bytes that the dry run writes the kernel form's name into
    ("fz_gemm_plan", "form"): _c.c_char_p,
}


def _signatures():
    """{entry point: (argtypes, restype)} of every prototype of the header"""
    sigs = {name: ([_ARG_EXCEPTIONS.get((name, a)) or _ctype(t, f"{name}, argument `{a}`") for t, a in args],
                   _c.c_char_p if ret == ("char", 1) else _ctype(ret, f"{name}, return type"))
            for name, (ret, args) in _H.functions.items()}
    stale = set(_ARG_EXCEPTIONS) - {(name, a) for name, (_, args) in _H.functions.items() for _, a in args}
    if stale:   # an argument renamed in the header would otherwise fall back to its rule in silence
        raise NativeError(f"_ARG_EXCEPTIONS names {sorted(stale)}, which include/factorizer_hip.h does not declare")
    return sigs


_SIGS = _signatures()


def declared_symbols():
    return sorted(_SIGS)


def lib():
    """Load (once) and return the native library; raise loudly if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                f"{LIB_PATH} not found: build it with `python -m factorizer_amd.build` "
                "(hipcc --offload-arch=gfx950). Device tensors have no fallback path.")
        h = ctypes.CDLL(LIB_PATH)
        try:
            h.fz_abi_version.restype = ctypes.c_int
            abi = int(h.fz_abi_version())
        except AttributeError:
            abi = None
        if abi != ABI_VERSION:
            raise NativeError(f"{LIB_PATH} has ABI revision {abi} and was not built from this tree's include/factorizer_hip.h "
                              f"(FZ_ABI_VERSION {ABI_VERSION}), which the binding is derived from: rebuild with "
                              "`python -m factorizer_amd.build`")
        for name, (args, res) in _SIGS.items():
            fn = getattr(h, name)  # AttributeError if the .so does not export it
            fn.argtypes = args
            fn.restype = res
        _lib = h
    return _lib


def launch_count() -> int:
    return int(lib().fz_launch_count())


def check(rc: int, what: str):
    if rc != FZ_OK:
        msg = lib().fz_last_error_string().decode()
        raise NativeError(f"{what} failed (code {rc}): {msg}")


def stream_ptr(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def shifts_array(shifts):
    flat = [int(v) for s in shifts for v in s]
    return (_i * len(flat))(*flat)


def outproj_fac(fac, geo):
    """fz_outproj_fac of fac = (vfac0, ufac0, vfac1, ufac1) (functional.core_factors) on geometry `geo`"""
    d = OutprojFac()
    d.v[0], d.u[0], d.v[1], d.u[1] = (t.data_ptr() for t in fac)
    d.dims[:] = list(geo.spatial)
    d.heads = geo.h
    d.shift[:] = [int(v) for s in geo.shifts3 for v in s]
    return d
