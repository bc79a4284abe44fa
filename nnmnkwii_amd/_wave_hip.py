"""ctypes binding of include/nnmnkwii_wave.h: pre-emphasis, mu-law and quantisation ("encode") and expansion and de-emphasis
("decode") of padded batches of waveforms, one launch each (csrc/wave_codec.hip).  The five entry points live in
libmlpg_hip.so beside the ``mlpg_hip_*`` ones, with their own prefix and version: they are bound here, on the handle
``_hip.lib()`` returns, and are no part of ``_hip.EXPORTS`` / ``_hip.ABI_VERSION``."""
import ctypes
import threading

from . import _hip
from ._hip import HipExtensionError

ABI_VERSION = 1
F32, F64, U8, I16, I32, I64 = range(6)
PLAIN, MULAW, QUANTIZE = range(3)
TILE = 1024                         # NNMK_WAVE_TILE: samples per step of a decode workgroup's walk
TABLE_LDS = 4096                    # NNMK_WAVE_TABLE_LDS
NAMES = ("nnmk_wave_abi_version", "nnmk_wave_encode", "nnmk_wave_decode", "nnmk_wave_plan", "nnmk_wave_launch_count")

_bound = None
_lock = threading.Lock()


def lib():
    """The library handle with the nnmk_wave_* symbols bound (once).  HipExtensionError: not built, or another version."""
    global _bound
    if _bound is not None:
        return _bound
    L = _hip.lib()
    with _lock:
        if _bound is None:
            ci, vp, i64, dbl = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
            p64 = ctypes.POINTER(ctypes.c_int64)
            try:
                L.nnmk_wave_abi_version.restype = ci
                L.nnmk_wave_abi_version.argtypes = []
                L.nnmk_wave_encode.restype = ci
                L.nnmk_wave_encode.argtypes = [ci, vp, ci, vp, i64, vp, ci, ci, ci, dbl, ci, ci, ci, vp, i64]
                L.nnmk_wave_decode.restype = ci
                L.nnmk_wave_decode.argtypes = [ci, vp, ci, vp, i64, vp, ci, ci, ci, ci, vp, ci, dbl, i64, ci, vp, i64]
                L.nnmk_wave_plan.restype = ci
                L.nnmk_wave_plan.argtypes = [i64, dbl, i64, p64, p64, p64]
                L.nnmk_wave_launch_count.restype = ctypes.c_longlong
                L.nnmk_wave_launch_count.argtypes = []
            except AttributeError as e:
                raise HipExtensionError("nnmnkwii_amd: %s has no nnmk_wave_* entry points (%s) -- rebuild it with "
                                        "`python nnmnkwii_amd/csrc/build.py`" % (_hip.SO_PATH, e))
            if L.nnmk_wave_abi_version() != ABI_VERSION:
                raise HipExtensionError("nnmnkwii_amd: %s has wave ABI version %d, this binding needs %d"
                                        % (_hip.SO_PATH, L.nnmk_wave_abi_version(), ABI_VERSION))
            _bound = L
    return _bound


def plan(Lmax, coef, segment=0):
    """nnmk_wave_plan: (S, W, nseg) for de-emphasis of utterances of Lmax samples; ValueError where the C entry refuses."""
    L = lib()
    S, W, n = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    if L.nnmk_wave_plan(int(Lmax), float(coef), int(segment), ctypes.byref(S), ctypes.byref(W), ctypes.byref(n)) != 0:
        raise ValueError(L.mlpg_hip_last_error().decode())
    return S.value, W.value, n.value


def _code(t):
    torch = _hip.torch_mod()
    return {torch.float32: F32, torch.float64: F64, torch.uint8: U8, torch.int16: I16, torch.int32: I32, torch.int64: I64}.get(t.dtype)


def _check2(name, t, codes, shape, dev):
    torch = _hip.torch_mod()
    if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 2 and _code(t) in codes and (shape is None or tuple(t.shape) == tuple(shape))
            and (dev is None or t.device == dev)):
        kinds = "float32 / float64" if codes == (F32, F64) else "uint8 / int16 / int32 / int64"
        raise ValueError("wave: %s must be a %s CUDA tensor of shape %s%s"
                         % (name, kinds, "(B, Lmax)" if shape is None else tuple(shape), "" if dev is None else " on x's device"))


def _stride(t, name):
    """The utterance stride of a (B, Lmax) tensor whose samples are contiguous (a row of a wider tensor is fine)."""
    B, Lmax = t.shape
    s0, s1 = t.stride()
    if Lmax > 1 and s1 != 1:
        raise ValueError("wave: the samples of %s must be contiguous, got strides %s" % (name, (s0, s1)))
    ld = s0 if B > 1 else Lmax
    if ld < Lmax:
        raise ValueError("wave: the utterances of %s overlap, got strides %s" % (name, (s0, s1)))
    return ld


def _lengths(lengths, B, dev):
    torch = _hip.torch_mod()
    if lengths is not None and not (torch.is_tensor(lengths) and lengths.dtype == torch.int32 and tuple(lengths.shape) == (B,)
                                    and lengths.device == dev and lengths.is_contiguous()):
        raise ValueError("wave: lengths must be an int32 (B) tensor on x's device")
    return lengths


def encode(x, lengths, coef, stage, mu, y):
    """nnmk_wave_encode on CUDA tensors.  x: (B, Lmax) float32 / float64 with contiguous samples; lengths: int32 (B) on x's device
    or None; coef: None (no pre-emphasis) or a number; stage: PLAIN, MULAW or QUANTIZE; y: (B, Lmax), float for PLAIN / MULAW,
    a class dtype for QUANTIZE.  One launch on the current stream, no synchronisation."""
    _check2("x", x, (F32, F64), None, None)
    B, Lmax = x.shape
    dev = x.device
    if stage not in (PLAIN, MULAW, QUANTIZE):
        raise ValueError("wave: unknown stage %r" % (stage,))
    _check2("y", y, (U8, I16, I32, I64) if stage == QUANTIZE else (F32, F64), x.shape, dev)
    _lengths(lengths, B, dev)
    ld_x, ld_y = _stride(x, "x"), _stride(y, "y")
    L = lib()
    if B * Lmax == 0:
        return y                     # (an empty tensor's pointer is NULL: nothing to launch)
    rc = L.nnmk_wave_encode(dev.index, _hip._stream(dev), _code(x), _hip._p(x), ld_x, _hip._p(lengths), B, Lmax, coef is not None,
                            0.0 if coef is None else float(coef), stage, int(mu), _code(y), _hip._p(y), ld_y)
    _hip._check(rc, "nnmk_wave_encode")
    return y


def decode(x, lengths, stage, mu, table, coef, segment, y):
    """nnmk_wave_decode on CUDA tensors.  x: (B, Lmax), a class dtype for QUANTIZE (table: float32 (mu + 1) on x's device), float
    for MULAW / PLAIN; coef: None (no de-emphasis) or a number, used as given; segment: 0 automatic, >= Lmax none; y: (B, Lmax)
    float32 / float64.  One launch on the current stream, no synchronisation."""
    torch = _hip.torch_mod()
    if stage not in (PLAIN, MULAW, QUANTIZE):
        raise ValueError("wave: unknown stage %r" % (stage,))
    _check2("x", x, (U8, I16, I32, I64) if stage == QUANTIZE else (F32, F64), None, None)
    B, Lmax = x.shape
    dev = x.device
    _check2("y", y, (F32, F64), x.shape, dev)
    _lengths(lengths, B, dev)
    if stage == QUANTIZE and not (torch.is_tensor(table) and table.dtype == torch.float32 and tuple(table.shape) == (int(mu) + 1,)
                                  and table.device == dev and table.is_contiguous()):
        raise ValueError("wave: table must be a float32 (mu + 1) tensor on x's device")
    ld_x, ld_y = _stride(x, "x"), _stride(y, "y")
    L = lib()
    if B * Lmax == 0:
        return y
    rc = L.nnmk_wave_decode(dev.index, _hip._stream(dev), _code(x), _hip._p(x), ld_x, _hip._p(lengths), B, Lmax, stage, int(mu),
                            _hip._p(table) if stage == QUANTIZE else None, coef is not None, 0.0 if coef is None else float(coef),
                            int(segment), _code(y), _hip._p(y), ld_y)
    _hip._check(rc, "nnmk_wave_decode")
    return y
