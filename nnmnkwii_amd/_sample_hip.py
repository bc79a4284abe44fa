"""ctypes binding of include/nnmnkwii_sample.h: draws from MLPG's trajectory distribution N(cbar, R^-1) and the whitening map
over padded batches (csrc/mlpg_trajsample.hip).  The entry points live in libmlpg_hip.so beside the ``mlpg_hip_*``
ones, with their own prefix and version: they are bound here, on the handle ``_hip.lib()`` returns, and are no part of
``_hip.EXPORTS`` / ``_hip.ABI_VERSION``.  The wrappers that hand the current torch stream on are in ``_sample_calls``."""
import ctypes
import threading

from . import _hip
from ._hip import HipExtensionError

ABI_VERSION = 1
NAMES = ("nnmk_draw_abi_version", "nnmk_draw_factor", "nnmk_draw_sample", "nnmk_draw_whiten", "nnmk_draw_group", "nnmk_draw_launch_count")

_bound = None
_lock = threading.Lock()


def lib():
    """The library handle with the nnmk_draw_* symbols bound (once).  HipExtensionError: not built, or another version."""
    global _bound
    if _bound is not None:
        return _bound
    L = _hip.lib()
    with _lock:
        if _bound is None:
            ci, vp, i64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
            try:
                L.nnmk_draw_abi_version.restype = ci
                L.nnmk_draw_abi_version.argtypes = []
                L.nnmk_draw_factor.restype = ci
                L.nnmk_draw_factor.argtypes = [ci, vp, ci, vp, ci, i64, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, i64, vp, vp]
                for fn in (L.nnmk_draw_sample, L.nnmk_draw_whiten):
                    fn.restype = ci
                    fn.argtypes = [ci, vp, ci, vp, i64, vp, vp, ci, ci, ci, ci, ci, vp, i64, vp, i64, vp, i64]
                L.nnmk_draw_group.restype = ci
                L.nnmk_draw_group.argtypes = []
                L.nnmk_draw_launch_count.restype = ctypes.c_longlong
                L.nnmk_draw_launch_count.argtypes = []
            except AttributeError as e:
                raise HipExtensionError("nnmnkwii_amd: %s has no nnmk_draw_* entry points (%s) -- rebuild it with "
                                        "`python nnmnkwii_amd/csrc/build.py`" % (_hip.SO_PATH, e))
            if L.nnmk_draw_abi_version() != ABI_VERSION:
                raise HipExtensionError("nnmnkwii_amd: %s has sample ABI version %d, this binding needs %d"
                                        % (_hip.SO_PATH, L.nnmk_draw_abi_version(), ABI_VERSION))
            _bound = L
    return _bound


def draw_group():
    """kDrawGroup: the draws a lane of nnmk_draw_sample carries side by side."""
    return int(lib().nnmk_draw_group())
