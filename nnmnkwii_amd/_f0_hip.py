"""ctypes binding of include/nnmnkwii_f0.h: the unvoiced gaps of F0 tracks filled and the V/UV flag, over padded batches
(csrc/f0_interp.hip).  The three entry points live in libmlpg_hip.so beside the ``mlpg_hip_*`` ones, with their
own prefix and version: they are bound here, on the handle ``_hip.lib()`` returns, and are no part of ``_hip.EXPORTS`` /
``_hip.ABI_VERSION``."""
import ctypes
import threading

from . import _hip
from ._hip import HipExtensionError

ABI_VERSION = 1
F32, F64 = 0, 1
KINDS = ("slinear", "linear", "previous", "zero", "next", "nearest", "nearest-up")
SLINEAR, LINEAR, PREVIOUS, ZERO, NEXT, NEAREST, NEAREST_UP = range(7)
TILE = 256                          # NNMK_F0_TILE: frames per step of a workgroup's walk
NAMES = ("nnmk_f0_abi_version", "nnmk_f0_interp", "nnmk_f0_launch_count")

_bound = None
_lock = threading.Lock()


def lib():
    """The library handle with the nnmk_f0_* symbols bound (once).  HipExtensionError: not built, or another version."""
    global _bound
    if _bound is not None:
        return _bound
    L = _hip.lib()
    with _lock:
        if _bound is None:
            ci, vp, i64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
            try:
                L.nnmk_f0_abi_version.restype = ci
                L.nnmk_f0_abi_version.argtypes = []
                L.nnmk_f0_interp.restype = ci
                L.nnmk_f0_interp.argtypes = [ci, vp, ci, vp, i64, vp, ci, ci, ci, ci, ci, vp, i64, ci, vp, i64]
                L.nnmk_f0_launch_count.restype = ctypes.c_longlong
                L.nnmk_f0_launch_count.argtypes = []
            except AttributeError as e:
                raise HipExtensionError("nnmnkwii_amd: %s has no nnmk_f0_* entry points (%s) -- rebuild it with "
                                        "`python nnmnkwii_amd/csrc/build.py`" % (_hip.SO_PATH, e))
            if L.nnmk_f0_abi_version() != ABI_VERSION:
                raise HipExtensionError("nnmnkwii_amd: %s has f0 ABI version %d, this binding needs %d"
                                        % (_hip.SO_PATH, L.nnmk_f0_abi_version(), ABI_VERSION))
            _bound = L
    return _bound


def kind_of(kind):
    """The kind's number; ValueError for anything else ("quadratic", "cubic" and integer orders are global spline solves)."""
    if not isinstance(kind, str) or kind not in KINDS:
        raise ValueError("interp1d: kind must be one of %s, got %r" % (", ".join(KINDS), kind))
    return KINDS.index(kind)


def _check3(name, t, shape, dev):
    torch = _hip.torch_mod()
    if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 3 and t.dtype in (torch.float32, torch.float64)
            and (shape is None or tuple(t.shape) == tuple(shape)) and (dev is None or t.device == dev)):
        raise ValueError("f0: %s must be a float32 / float64 CUDA tensor of shape %s%s"
                         % (name, "(B, Tmax, C)" if shape is None else tuple(shape), "" if dev is None else " on x's device"))


def interp(x, lengths, kind, y, vuv):
    """nnmk_f0_interp on CUDA tensors.  x: (B, Tmax, C) float32 / float64 whose last dimension is contiguous and whose first two
    are those of a dense (B, Tmax, ld) array (a column slice of one is fine); lengths: int32 (B) on x's device or None; kind:
    0 .. 6; y, vuv: like x (shape, not dtype), either may be None, y may be x itself.  One launch on the current stream, no
    synchronisation."""
    torch = _hip.torch_mod()
    _check3("x", x, None, None)
    B, Tmax, C = x.shape
    dev = x.device
    if not 0 <= int(kind) < len(KINDS):
        raise ValueError("f0: unknown kind %r" % (kind,))
    if y is None and vuv is None:
        raise ValueError("f0: y and vuv are both None: nothing to compute")
    for name, t in (("y", y), ("vuv", vuv)):
        if t is not None:
            _check3(name, t, x.shape, dev)
    if lengths is not None and not (torch.is_tensor(lengths) and lengths.dtype == torch.int32 and tuple(lengths.shape) == (B,)
                                    and lengths.device == dev and lengths.is_contiguous()):
        raise ValueError("f0: lengths must be an int32 (B) tensor on x's device")
    try:
        ld = [_hip._pf_row_stride(t, B, Tmax, C, "f0") if t is not None and C else 0 for t in (x, y, vuv)]
    except HipExtensionError as e:
        raise ValueError(str(e))
    L = lib()
    if B * Tmax * C == 0:
        return y, vuv                # (an empty tensor's pointer is NULL: nothing to launch)
    rc = L.nnmk_f0_interp(dev.index, _hip._stream(dev), _hip._dt(x), _hip._p(x), ld[0], _hip._p(lengths), B, Tmax, C, int(kind),
                          _hip._dt(y) if y is not None else F32, _hip._p(y), ld[1], _hip._dt(vuv) if vuv is not None else F32, _hip._p(vuv), ld[2])
    _hip._check(rc, "nnmk_f0_interp")
    return y, vuv
