"""ctypes binding of include/nnmnkwii_trajectory.h: the band of MLPG's trajectory covariance, log det R and the trajectory
likelihood with its gradients over padded batches (csrc/mlpg_trajcov.hip).  The five entry points live in
libmlpg_hip.so beside the ``mlpg_hip_*`` ones, with their own prefix and version: they are bound here, on the handle
``_hip.lib()`` returns, and are no part of ``_hip.EXPORTS`` / ``_hip.ABI_VERSION``."""
import ctypes
import threading

from . import _hip
from ._hip import HipExtensionError

ABI_VERSION = 1
NAMES = ("nnmk_traj_abi_version", "nnmk_traj_covariance", "nnmk_traj_nll", "nnmk_traj_nll_workspace", "nnmk_traj_launch_count")

_bound = None
_lock = threading.Lock()


def lib():
    """The library handle with the nnmk_traj_* symbols bound (once).  HipExtensionError: not built, or another version."""
    global _bound
    if _bound is not None:
        return _bound
    L = _hip.lib()
    with _lock:
        if _bound is None:
            ci, vp, i64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
            try:
                L.nnmk_traj_abi_version.restype = ci
                L.nnmk_traj_abi_version.argtypes = []
                L.nnmk_traj_covariance.restype = ci
                L.nnmk_traj_covariance.argtypes = [ci, vp, ci, vp, ci, i64, vp, ci, ci, ci, ci, ci, vp, vp, vp, ci, vp, i64, vp, vp]
                L.nnmk_traj_nll.restype = ci
                L.nnmk_traj_nll.argtypes = [ci, vp, ci, vp, vp, ci, i64, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, i64, vp, i64, vp, i64, vp,
                                            vp, vp, vp, vp, i64]
                L.nnmk_traj_nll_workspace.restype = i64
                L.nnmk_traj_nll_workspace.argtypes = [ci, ci, ci, ci]
                L.nnmk_traj_launch_count.restype = ctypes.c_longlong
                L.nnmk_traj_launch_count.argtypes = []
            except AttributeError as e:
                raise HipExtensionError("nnmnkwii_amd: %s has no nnmk_traj_* entry points (%s) -- rebuild it with "
                                        "`python nnmnkwii_amd/csrc/build.py`" % (_hip.SO_PATH, e))
            if L.nnmk_traj_abi_version() != ABI_VERSION:
                raise HipExtensionError("nnmnkwii_amd: %s has trajectory ABI version %d, this binding needs %d"
                                        % (_hip.SO_PATH, L.nnmk_traj_abi_version(), ABI_VERSION))
            _bound = L
    return _bound


def half_bandwidth(windows):
    """Q = max (l + u) of a window list or PackedWindows."""
    wl, wu, _ = _hip.pack_windows(windows)
    return int((wl + wu).max()) if len(wl) else 0


def nll_workspace(var_mode, want_grad_vars, B, D):
    n = int(lib().nnmk_traj_nll_workspace(int(var_mode), int(bool(want_grad_vars)), int(B), int(D)))
    if n < 0:
        raise ValueError("trajectory: bad var_mode or size")
    return n
