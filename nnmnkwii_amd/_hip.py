"""ctypes binding of libmlpg_hip.so (include/mlpg_hip.h) + thin tensor helpers.

PyTorch is used here for device memory, streams and nothing else: every
numerical result comes from the hand-written HIP kernels behind the C ABI.
There is NO CPU fallback: if the shared library or a GPU is missing, the calls
raise.
"""
import ctypes
import os
import sys
import threading

import numpy as np

F32, F64 = 0, 1
ABI_VERSION = 14               # mlpg_hip_abi_version() of the library this binding was written for
VAR_FRAME, VAR_GLOBAL, VAR_UNIT = 0, 1, 2
ALGO_AUTO, ALGO_GENERIC, ALGO_WAVE, ALGO_STRIP, ALGO_PIPE, ALGO_CONST, ALGO_CHUNK, ALGO_FIR = 0, 1, 2, 3, 4, 5, 6, 7

_HERE = os.path.dirname(os.path.abspath(__file__))
# NNMNKWII_AMD_SO selects another build of the same library (kernel experiments); default: the in-tree build
SO_PATH = os.environ.get("NNMNKWII_AMD_SO") or os.path.join(_HERE, "csrc", "libmlpg_hip.so")

EXPORTS = (
    "mlpg_hip_abi_version",
    "mlpg_hip_launch_count",
    "mlpg_hip_last_error",
    "mlpg_hip_device_count",
    "mlpg_hip_shutdown",
    "mlpg_hip_forward",
    "mlpg_hip_forward_host",
    "mlpg_hip_fastdtw_host",
    "mlpg_hip_host_alloc",
    "mlpg_hip_host_free",
    "mlpg_hip_forward_streams",
    "mlpg_hip_backward",
    "mlpg_hip_delta_features",
    "mlpg_hip_modspec",
    "mlpg_hip_inv_modspec",
    "mlpg_hip_modspec_smoothing",
    "mlpg_hip_modspec_backward",
    "mlpg_hip_modspec_set_direct",
    "mlpg_hip_modspec_route",
    "mlpg_hip_modspec_batch",
    "mlpg_hip_modspec_batch_backward",
    "mlpg_hip_modspec_loss_form",
    "mlpg_hip_modspec_loss_workspace_bytes",
    "mlpg_hip_modspec_loss_step",
    "mlpg_hip_trim_lengths",
    "mlpg_hip_fastdtw",
    "mlpg_hip_forward_host_multi",
    "mlpg_hip_fastdtw_host_multi",
    "mlpg_hip_host_chunk_plan",
    "mlpg_hip_dtw_level_windows",
    "mlpg_hip_dtw_level_from_costs",
    "mlpg_hip_fastdtw_l2",
    "mlpg_hip_gather_path",
    "mlpg_hip_gmm_convert",
    "mlpg_hip_stream_copy",
    "mlpg_hip_unit_mse_step",
    "mlpg_hip_unit_mse_workspace_bytes",
    "mlpg_hip_unit_mse_workspace_bytes_t",
    "mlpg_hip_unit_mse_form",
    "mlpg_hip_host_copy",
    "mlpg_hip_backward_host",
    "mlpg_hip_backward_var",
    "mlpg_hip_backward_streams",
    "mlpg_hip_gmm_workspace_bytes",
    "mlpg_hip_gmm_estep",
    "mlpg_hip_gmm_mstep",
    "mlpg_hip_gmm_precisions",
    "mlpg_hip_kmeans_workspace_bytes",
    "mlpg_hip_kmeans_seed_step",
    "mlpg_hip_kmeans_lloyd_step",
    "mlpg_hip_postfilter_table",
    "mlpg_hip_merlin_post_filter",
    "mlpg_hip_modspec_filter_form",
    "mlpg_hip_modspec_filter",
    "mlpg_hip_gmm_trajectory_stats",
    "mlpg_hip_gv_max_frames",
    "mlpg_hip_gv_ascent",
    "mlpg_hip_gv",
    "mlpg_hip_column_stats_workspace",
    "mlpg_hip_column_stats",
    "mlpg_hip_column_affine",
)


class HipExtensionError(RuntimeError):
    """The HIP extension is missing, failed to load, or a call into it failed."""


_lib = None
_lock = threading.Lock()


def _preload_torch_hip_runtime():
    """One HIP runtime per process.  The PyTorch-ROCm wheel ships its own libamdhip64 / libhsa-runtime64 and loads them by path;
    libmlpg_hip.so asks for "libamdhip64.so.7".  Loaded after torch, the library is given torch's copy (same SONAME) and all is
    well; loaded BEFORE torch -- a program that starts with the numpy-only entry points -- it would bring in the system's runtime,
    torch would then add its own, and with two runtimes in the process ``torch.cuda.is_available()`` turns False.  So, when torch is
    installed but not imported yet, its runtime libraries are loaded first (no ``import torch``: that costs seconds and the
    host-pointer entry points do not need it)."""
    if "torch" in sys.modules:
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        libdir = os.path.join(os.path.dirname(spec.origin), "lib")
        for name in ("libhsa-runtime64.so", "libamdhip64.so"):
            path = os.path.join(libdir, name)
            if os.path.exists(path):
                ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    except Exception:  # noqa: BLE001 -- best effort: without it the system's runtime is used, as before
        pass


def lib():
    """Load libmlpg_hip.so (once). Raises HipExtensionError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(SO_PATH):
            raise HipExtensionError(
                "nnmnkwii_amd: %s is missing -- build it with `python nnmnkwii_amd/csrc/build.py` "
                "(or __graft_entry__.build()); there is no CPU fallback" % SO_PATH)
        _preload_torch_hip_runtime()
        try:
            L = ctypes.CDLL(SO_PATH)
        except OSError as e:  # pragma: no cover
            raise HipExtensionError("nnmnkwii_amd: cannot load %s: %s" % (SO_PATH, e))
        vp, ci, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
        L.mlpg_hip_abi_version.restype = ci
        L.mlpg_hip_abi_version.argtypes = []
        L.mlpg_hip_launch_count.restype = ctypes.c_longlong
        L.mlpg_hip_launch_count.argtypes = [ci]
        L.mlpg_hip_last_error.restype = ctypes.c_char_p
        L.mlpg_hip_last_error.argtypes = []
        L.mlpg_hip_device_count.restype = ci
        L.mlpg_hip_device_count.argtypes = []
        L.mlpg_hip_shutdown.restype = None
        L.mlpg_hip_shutdown.argtypes = []
        L.mlpg_hip_forward.restype = ci
        L.mlpg_hip_forward.argtypes = [ci, vp, ci, ci, vp, vp, ci, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp]
        L.mlpg_hip_forward_host.restype = ci
        L.mlpg_hip_forward_host.argtypes = [ci, ci, ci, vp, vp, ci, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp]
        L.mlpg_hip_backward_host.restype = ci
        L.mlpg_hip_backward_host.argtypes = [ci, ci, ci, ci, vp, ci, vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp]
        L.mlpg_hip_fastdtw_host.restype = ci
        L.mlpg_hip_fastdtw_host.argtypes = [ci, ci, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ctypes.c_double, ci, ctypes.c_double,
                                            vp, vp, vp, vp, vp, vp]
        L.mlpg_hip_forward_host_multi.restype = ci
        L.mlpg_hip_forward_host_multi.argtypes = [vp, ci, ci, ci, vp, vp, ci, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp]
        L.mlpg_hip_fastdtw_host_multi.restype = ci
        L.mlpg_hip_fastdtw_host_multi.argtypes = [vp, ci, ci, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ctypes.c_double, ci,
                                                  ctypes.c_double, vp, vp, vp, vp, vp, vp]
        L.mlpg_hip_host_chunk_plan.restype = ctypes.c_longlong
        L.mlpg_hip_host_chunk_plan.argtypes = [ctypes.c_longlong, ctypes.c_longlong, ci, ctypes.c_longlong, vp, vp, vp, vp]
        L.mlpg_hip_host_alloc.restype = vp
        L.mlpg_hip_host_alloc.argtypes = [ctypes.c_size_t]
        L.mlpg_hip_host_copy.restype = ci
        L.mlpg_hip_host_copy.argtypes = [vp, vp, ctypes.c_size_t]
        L.mlpg_hip_host_free.restype = None
        L.mlpg_hip_host_free.argtypes = [vp]
        L.mlpg_hip_forward_streams.restype = ci
        L.mlpg_hip_forward_streams.argtypes = [ci, vp, ci, ci, vp, vp, ci, ctypes.c_int64, vp, ci, ci, ci, vp, ci, vp, vp, vp,
                                               vp, ctypes.c_int64, vp]
        L.mlpg_hip_backward.restype = ci
        L.mlpg_hip_backward.argtypes = [ci, vp, ci, ci, ci, vp, ci, vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp]
        L.mlpg_hip_backward_var.restype = ci
        L.mlpg_hip_backward_var.argtypes = [ci, vp, ci, ci, vp, vp, ci, vp, vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]
        L.mlpg_hip_backward_streams.restype = ci
        L.mlpg_hip_backward_streams.argtypes = [ci, vp, ci, ci, vp, vp, ci, ctypes.c_int64, vp, vp, ctypes.c_int64, vp, ci, ci, ci, vp,
                                                ci, vp, vp, vp, vp, vp, vp]
        L.mlpg_hip_delta_features.restype = ci
        L.mlpg_hip_delta_features.argtypes = [ci, vp, ci, vp, vp, ci, ci, ci, ci, vp, vp, vp, vp]
        L.mlpg_hip_modspec.restype = ci
        L.mlpg_hip_modspec.argtypes = [ci, vp, vp, ci, ci, ci, ci, ci, vp, vp]
        L.mlpg_hip_inv_modspec.restype = ci
        L.mlpg_hip_inv_modspec.argtypes = [ci, vp, vp, vp, ci, ci, ci, ci, vp]
        L.mlpg_hip_modspec_smoothing.restype = ci
        L.mlpg_hip_modspec_smoothing.argtypes = [ci, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp]
        L.mlpg_hip_modspec_backward.restype = ci
        L.mlpg_hip_modspec_backward.argtypes = [ci, vp, vp, vp, ci, ci, ci, ci, ci, vp]
        L.mlpg_hip_modspec_set_direct.restype = None
        L.mlpg_hip_modspec_set_direct.argtypes = [ci]
        L.mlpg_hip_modspec_route.restype = ci
        L.mlpg_hip_modspec_route.argtypes = [ci]
        L.mlpg_hip_modspec_batch.restype = ci
        L.mlpg_hip_modspec_batch.argtypes = [ci, vp, ci, vp, vp, ci, ci, ci, ci, ci, vp]
        L.mlpg_hip_modspec_batch_backward.restype = ci
        L.mlpg_hip_modspec_batch_backward.argtypes = [ci, vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, vp]
        L.mlpg_hip_modspec_loss_form.restype = ci
        L.mlpg_hip_modspec_loss_form.argtypes = [ci]
        L.mlpg_hip_modspec_loss_workspace_bytes.restype = ctypes.c_size_t
        L.mlpg_hip_modspec_loss_workspace_bytes.argtypes = [ci, ci]
        L.mlpg_hip_modspec_loss_step.restype = ci
        L.mlpg_hip_modspec_loss_step.argtypes = [ci, vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, ci, cd, cd, vp, vp, vp, ctypes.c_size_t]
        L.mlpg_hip_trim_lengths.restype = ci
        L.mlpg_hip_trim_lengths.argtypes = [ci, vp, ci, vp, ci, ci, ci, cd, vp]
        L.mlpg_hip_fastdtw_l2.restype = ci
        L.mlpg_hip_fastdtw_l2.argtypes = [ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp]
        L.mlpg_hip_dtw_level_windows.restype = ci
        L.mlpg_hip_dtw_level_windows.argtypes = [ci, vp, ci, ci, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, ci]
        L.mlpg_hip_dtw_level_from_costs.restype = ci
        L.mlpg_hip_dtw_level_from_costs.argtypes = [ci, vp, ci, ci, vp, vp, vp, vp, vp, ci, ci, vp, vp, ctypes.c_longlong, vp, vp, vp,
                                                    ci, vp]
        L.mlpg_hip_fastdtw.restype = ci
        L.mlpg_hip_fastdtw.argtypes = [ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, cd, ci, vp, vp, vp, vp]
        L.mlpg_hip_gmm_convert.restype = ci
        L.mlpg_hip_gmm_convert.argtypes = [ci, vp, vp, vp, vp, vp, vp, vp, ctypes.c_int64, ci, ci, ci, vp]
        L.mlpg_hip_gather_path.restype = ci
        L.mlpg_hip_gather_path.argtypes = [ci, vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, vp]
        L.mlpg_hip_unit_mse_step.restype = ci
        L.mlpg_hip_unit_mse_step.argtypes = [ci, vp, ci, vp, vp, vp, ci, ci, ci, ci, vp, vp, vp, cd, vp, vp, vp, vp, vp,
                                             ctypes.c_size_t]
        L.mlpg_hip_unit_mse_workspace_bytes.restype = ctypes.c_size_t
        L.mlpg_hip_unit_mse_workspace_bytes.argtypes = [ci, ci, ci]
        L.mlpg_hip_unit_mse_workspace_bytes_t.restype = ctypes.c_size_t
        L.mlpg_hip_unit_mse_workspace_bytes_t.argtypes = [ci, ci, ci, ci]
        L.mlpg_hip_unit_mse_form.restype = ci
        L.mlpg_hip_unit_mse_form.argtypes = [ci, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp]
        L.mlpg_hip_stream_copy.restype = ci
        L.mlpg_hip_stream_copy.argtypes = [ci, vp, vp, vp, ctypes.c_size_t]
        L.mlpg_hip_gmm_workspace_bytes.restype = ctypes.c_size_t
        L.mlpg_hip_gmm_workspace_bytes.argtypes = [ctypes.c_int64, ci, ci]
        L.mlpg_hip_gmm_estep.restype = ci
        L.mlpg_hip_gmm_estep.argtypes = [ci, vp, vp, vp, vp, vp, vp, ctypes.c_int64, ci, ci, vp, vp, vp, vp, vp, ctypes.c_size_t]
        L.mlpg_hip_gmm_mstep.restype = ci
        L.mlpg_hip_gmm_mstep.argtypes = [ci, vp, vp, vp, ctypes.c_int64, ci, ci, cd, vp, vp, vp, vp, ctypes.c_size_t]
        L.mlpg_hip_gmm_precisions.restype = ci
        L.mlpg_hip_gmm_precisions.argtypes = [ci, vp, vp, ci, ci, vp, vp, vp]
        L.mlpg_hip_kmeans_workspace_bytes.restype = ctypes.c_size_t
        L.mlpg_hip_kmeans_workspace_bytes.argtypes = [ctypes.c_int64, ci, ci]
        L.mlpg_hip_kmeans_seed_step.restype = ci
        L.mlpg_hip_kmeans_seed_step.argtypes = [ci, vp, vp, vp, ctypes.c_int64, ci, vp, ci, vp, vp, vp, vp, ctypes.c_size_t]
        L.mlpg_hip_kmeans_lloyd_step.restype = ci
        L.mlpg_hip_kmeans_lloyd_step.argtypes = [ci, vp, vp, vp, vp, vp, ctypes.c_int64, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t]
        if L.mlpg_hip_abi_version() != ABI_VERSION:
            raise HipExtensionError("nnmnkwii_amd: %s has ABI version %d, this binding needs %d -- rebuild it with "
                                    "`python nnmnkwii_amd/csrc/build.py`" % (SO_PATH, L.mlpg_hip_abi_version(), ABI_VERSION))
        L.mlpg_hip_postfilter_table.restype = ci
        L.mlpg_hip_postfilter_table.argtypes = [ci, cd, ci, ci, vp]
        L.mlpg_hip_merlin_post_filter.restype = ci
        L.mlpg_hip_merlin_post_filter.argtypes = [ci, vp, ci, vp, ctypes.c_int64, vp, ci, ci, ci, cd, vp, vp, ci, vp, ctypes.c_int64]
        L.mlpg_hip_modspec_filter_form.restype = ci
        L.mlpg_hip_modspec_filter_form.argtypes = [ci]
        L.mlpg_hip_modspec_filter.restype = ci
        L.mlpg_hip_modspec_filter.argtypes = [ci, vp, ci, vp, ctypes.c_int64, vp, ci, ci, ci, ci, ci, vp, vp, ci, ci, vp, ctypes.c_int64]
        L.mlpg_hip_gmm_trajectory_stats.restype = ci
        L.mlpg_hip_gmm_trajectory_stats.argtypes = [ci, vp, vp, ctypes.c_int64, vp, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp, ctypes.c_int64,
                                                    vp, ctypes.c_int64]
        L.mlpg_hip_gv_max_frames.restype = ci
        L.mlpg_hip_gv_max_frames.argtypes = []
        L.mlpg_hip_gv_ascent.restype = ci
        L.mlpg_hip_gv_ascent.argtypes = [ci, vp, ci, vp, vp, ci, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, cd, ci, cd, ci, vp, vp]
        L.mlpg_hip_gv.restype = ci
        L.mlpg_hip_gv.argtypes = [ci, vp, ci, vp, ctypes.c_int64, vp, ci, ci, ci, vp]
        # preprocessing/generic.py:496-636 (meanvar, meanstd, minmax) in one pass
        L.mlpg_hip_column_stats_workspace.restype = ctypes.c_int64
        L.mlpg_hip_column_stats_workspace.argtypes = [ci, ci, ci]
        L.mlpg_hip_column_stats.restype = ci
        L.mlpg_hip_column_stats.argtypes = [ci, vp, ci, vp, ctypes.c_int64, vp, ci, ci, ci, vp, vp, vp, ctypes.c_int64]
        # preprocessing/generic.py:639-684 (scale, inv_scale) and :734-828 (minmax_scale, inv_minmax_scale)
        L.mlpg_hip_column_affine.restype = ci
        L.mlpg_hip_column_affine.argtypes = [ci, vp, ci, ci, ci, vp, ctypes.c_int64, vp, ctypes.c_int64, vp, ci, ci, ci, vp, vp]
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        raise HipExtensionError("%s failed (%d): %s" % (what, rc, lib().mlpg_hip_last_error().decode()))


def torch_mod():
    import torch
    return torch


_gpu_ok = False   # torch.cuda.is_available() has been seen True and the library is loaded (neither changes afterwards)


def require_gpu(device=None):
    """Return a torch.device for the GPU to use, or raise (no CPU fallback)."""
    global _gpu_ok
    if _gpu_ok and device is not None and device.__class__.__name__ == "device" and device.type == "cuda" and device.index is not None:
        return device            # the hot path: a tensor's own device (torch.cuda.is_available() alone costs microseconds)
    torch = torch_mod()
    lib()
    if not torch.cuda.is_available():
        raise HipExtensionError("nnmnkwii_amd needs an AMD GPU (torch.cuda.is_available() is False); "
                                "there is no CPU fallback")
    _gpu_ok = True
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise HipExtensionError("nnmnkwii_amd computes on GPU only, got device %s" % device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


class PackedWindows(tuple):
    """(int32 l[], int32 u[], float64 coeff[], num_windows): what pack_windows returns; pass it instead of the window
    list to skip the packing in a hot loop.  `ptrs()`: the three host addresses as ints (computed once: numpy's
    `.ctypes.data_as` costs microseconds per call, the C ABI takes the address itself)."""

    def ptrs(self):
        pt = self.__dict__.get("_ptrs")
        if pt is None:
            pt = self.__dict__["_ptrs"] = (self[0].ctypes.data, self[1].ctypes.data, self[2].ctypes.data)
        return pt


def _win_args(windows):
    """(num_windows, address of l[], u[], coeff[], keep-alive) for the C ABI."""
    if isinstance(windows, PackedWindows):
        a, b, c = windows.ptrs()
        return windows[3], a, b, c, windows
    wl, wu, wc = pack_windows(windows)
    return len(wl), wl.ctypes.data, wu.ctypes.data, wc.ctypes.data, (wl, wu, wc)


def pack_windows(windows):
    """Reference `(l, u, coeff)` triples -> (int32 l[], int32 u[], float64 coeff[]) host arrays."""
    if isinstance(windows, PackedWindows):
        return windows[0], windows[1], windows[2]
    wl, wu, wc = [], [], []
    for l, u, coeff in windows:
        l, u = int(l), int(u)
        assert l >= 0 and u >= 0                     # paramgen/_mlpg.py:44
        coeff = np.asarray(coeff, dtype=np.float64).ravel()
        assert len(coeff) == l + u + 1               # paramgen/_mlpg.py:45
        wl.append(l)
        wu.append(u)
        wc.append(coeff)
    return (np.ascontiguousarray(wl, dtype=np.int32), np.ascontiguousarray(wu, dtype=np.int32),
            np.ascontiguousarray(np.concatenate(wc)))


def prepack_windows(windows):
    """Pack once, reuse: the result is accepted wherever a window list is."""
    if isinstance(windows, PackedWindows):
        return windows
    wl, wu, wc = pack_windows(windows)
    return PackedWindows((wl, wu, wc, len(wl)))


def _nw(windows):
    return windows[3] if isinstance(windows, PackedWindows) else len(windows)


_WIN_CACHE = {}     # id(window list) -> (the list, its signature, PackedWindows): the literal per-utterance calls pass the same list


def cached_windows(windows):
    """PackedWindows of a window list, remembered per list OBJECT (a loop of paramgen.mlpg calls passes the same list every
    time: packing costs 5 us, a config-1 call 30).  The remembered tables are used only if the list still holds the same
    (l, u, coefficient object) triples with the same coefficient bytes; anything else is packed afresh."""
    if isinstance(windows, PackedWindows):
        return windows
    ent = _WIN_CACHE.get(id(windows))
    try:
        if ent is not None and ent[0] is windows and len(windows) == len(ent[1]):
            for w, g in zip(windows, ent[1]):
                c = w[2]
                if w[0] != g[0] or w[1] != g[1] or c is not g[2] or (c.tobytes() if type(c) is np.ndarray else tuple(c)) != g[3]:
                    break
            else:
                return ent[2]
        packed = prepack_windows(windows)
        sig = tuple((w[0], w[1], w[2], w[2].tobytes() if type(w[2]) is np.ndarray else tuple(w[2])) for w in windows)
    except (TypeError, IndexError):      # not a list of (l, u, coeff) triples this cache understands: no caching
        return prepack_windows(windows)
    if len(_WIN_CACHE) >= 64:
        _WIN_CACHE.clear()
    _WIN_CACHE[id(windows)] = (windows, sig, packed)
    return packed


def _dt(t):
    torch = torch_mod()
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float64:
        return F64
    raise HipExtensionError("unsupported dtype %s (float32/float64 only)" % t.dtype)


def _p(t):
    return None if t is None else t.data_ptr()      # (argtypes are declared: ctypes converts the int itself)


def _np(a):
    return a.ctypes.data_as(ctypes.c_void_p)


_raw_stream = None


def _stream(device):
    """The current torch stream of `device` as the raw hipStream_t (an int).  torch._C._cuda_getCurrentRawStream is the
    cheap way (what torch's own compiled code uses); torch.cuda.current_stream(...) builds a Stream object per call."""
    global _raw_stream
    if _raw_stream is None:
        torch = torch_mod()
        f = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        _raw_stream = f if f is not None else (lambda idx: torch.cuda.current_stream(idx).cuda_stream)
    return _raw_stream(device.index if device.index is not None else torch_mod().cuda.current_device())


def _var_mode(var, ref, shape, D):
    """The variance mode of a tensor argument: None -> unit variances, (D,) -> global, else per frame of `shape`; the dtype and
    device of `ref`, contiguous."""
    if var is None:
        return VAR_UNIT
    assert var.dtype == ref.dtype and var.is_contiguous() and var.device == ref.device
    if var.dim() == 1:
        assert var.shape[0] == D
        return VAR_GLOBAL
    assert var.shape == shape
    return VAR_FRAME


def _check_lengths(lengths, B, device):
    if lengths is not None:
        assert lengths.dtype == torch_mod().int32 and lengths.shape == (B,) and lengths.device == device


def forward(mean, var, windows, lengths=None, algo=ALGO_AUTO, want_status=True):
    """Batched MLPG on device tensors.

    mean (B, T, D) cuda float32/float64 contiguous; var: same shape, (D,) or None
    (unit variances); lengths: cuda int32 (B,) or None.  Returns (out (B,T,sd),
    status int32 (B*sd) or None), both on the device, enqueued on the current
    stream (no synchronisation).
    """
    torch = torch_mod()
    assert mean.is_cuda and mean.dim() == 3 and mean.is_contiguous()
    B, T, D = mean.shape
    nw, pl, pu, pc, _keep = _win_args(windows)
    mode = _var_mode(var, mean, mean.shape, D)
    _check_lengths(lengths, B, mean.device)
    out = torch.empty((B, T, D // nw), dtype=mean.dtype, device=mean.device)
    status = torch.empty((B * (D // nw),), dtype=torch.int32, device=mean.device) if want_status else None
    rc = lib().mlpg_hip_forward(mean.device.index, _stream(mean.device), _dt(mean), algo, _p(mean), _p(var), mode,
                                _p(lengths), B, T, D, nw, pl, pu, pc, _p(out), _p(status))
    _check(rc, "mlpg_hip_forward")
    return out, status


def current_device_index(device=None):
    """GPU index for the host-pointer entry points: an explicit int / "cuda:1" / object with .index, otherwise the
    process's current device (what torch.cuda.set_device(local_rank) selected in a one-process-per-GPU job; 0 when
    torch has not been imported or has not touched the GPU yet -- the entry points themselves need no torch)."""
    if device is not None:
        idx = device if isinstance(device, str) else getattr(device, "index", device)
        if isinstance(idx, str):
            idx = idx.split(":")[-1] if ":" in idx else None
        if idx is not None:
            return int(idx)
    t = sys.modules.get("torch")
    # (another thread may be in the middle of `import torch`: sys.modules then holds a module without its attributes yet)
    cuda = getattr(t, "cuda", None)
    ready = getattr(cuda, "is_initialized", None)
    if ready is not None and ready():
        return int(cuda.current_device())
    return 0


def device_list(device=None):
    """The int32 device list of the *_host_multi entry points: ``"all"`` -> empty (= every visible device), a list /
    tuple of indices as given (an index may repeat: each occurrence gets its own streams and staging buffers), anything
    else -> the one device current_device_index picks."""
    if isinstance(device, str) and device == "all":
        return np.zeros((0,), dtype=np.int32)
    if isinstance(device, (list, tuple, np.ndarray)):
        return np.ascontiguousarray([current_device_index(d) for d in device], dtype=np.int32)
    return np.asarray([current_device_index(device)], dtype=np.int32)


def host_chunk_plan(n_items, target_items, num_devices):
    """mlpg_hip_host_chunk_plan (pure host logic, no GPU needed): how the host-memory calls deal a batch to the devices.
    Returns int arrays (entry, slot, first, count), one element per chunk."""
    L = lib()
    n = int(L.mlpg_hip_host_chunk_plan(int(n_items), int(target_items), int(num_devices), 0, None, None, None, None))
    if n < 0:
        _check(n, "mlpg_hip_host_chunk_plan")
    entry, slot = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    first, count = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    L.mlpg_hip_host_chunk_plan(int(n_items), int(target_items), int(num_devices), n, _np(entry), _np(slot), _np(first), _np(count))
    return entry, slot, first, count


_host_gpu_seen = False     # mlpg_hip_device_count() > 0 has been seen (it does not change afterwards)


def _host_lib():
    """The library, for the host-pointer entry points (no torch involved): raises unless the HIP runtime sees a GPU."""
    global _host_gpu_seen
    L = lib()
    if not _host_gpu_seen:
        if L.mlpg_hip_device_count() <= 0:
            raise HipExtensionError("nnmnkwii_amd needs an AMD GPU (none visible to the HIP runtime); there is no CPU fallback")
        _host_gpu_seen = True
    return L


def _np_var(var, ref, shape, D):
    """(variance mode, address) of a numpy variance argument: None, (D,) or `shape`; the dtype of `ref`, C-contiguous."""
    if var is None:
        return VAR_UNIT, None
    assert var.dtype == ref.dtype and var.flags.c_contiguous
    assert var.shape == ((D,) if var.ndim == 1 else shape)
    return (VAR_GLOBAL if var.ndim == 1 else VAR_FRAME), var.ctypes.data


def _np_lengths(lengths, B):
    """(int32 array to keep alive, its address) of a numpy lengths argument; (None, None) without one."""
    if lengths is None:
        return None, None
    lengths = np.ascontiguousarray(lengths, dtype=np.int32)
    assert lengths.shape == (B,)
    return lengths, lengths.ctypes.data


def forward_host(mean, var, windows, lengths=None, algo=ALGO_AUTO, device=None):
    """Batched MLPG, numpy in -> numpy out through mlpg_hip_forward_host[_multi] (no torch involved): mean (B, T, D)
    float32/float64 C-contiguous, var same shape / (D,) / None, lengths int32 (B,) or None; device: GPU index
    (default: the current device, see current_device_index), a list of indices, or "all" (every visible device; the
    utterance chunks are dealt round-robin, see device_list).  One device: mlpg_hip_forward_host, whose small calls
    (a single utterance: the literal paramgen.mlpg call) take the library's short path.
    Returns (out (B, T, sd) ndarray, status int32 (B, sd))."""
    L = _host_lib()
    assert mean.ndim == 3 and mean.flags.c_contiguous and mean.dtype in (np.float32, np.float64)
    B, T, D = mean.shape
    pw = cached_windows(windows)
    nw = pw[3]
    pl, pu, pc = pw.ptrs()
    dt = F32 if mean.dtype == np.float32 else F64
    mode, pv = _np_var(var, mean, mean.shape, D)
    lengths, plen = _np_lengths(lengths, B)
    out = np.empty((B, T, D // nw), dtype=mean.dtype)
    status = np.zeros((B, D // nw), dtype=np.int32)
    if isinstance(device, (list, tuple, np.ndarray)) or (isinstance(device, str) and device == "all"):
        devs = device_list(device)
        rc = L.mlpg_hip_forward_host_multi(_np(devs) if len(devs) else None, len(devs), dt, algo, mean.ctypes.data, pv, mode, plen,
                                           B, T, D, nw, pl, pu, pc, out.ctypes.data, status.ctypes.data)
        _check(rc, "mlpg_hip_forward_host_multi")
    else:
        rc = L.mlpg_hip_forward_host(current_device_index(device), dt, algo, mean.ctypes.data, pv, mode, plen,
                                     B, T, D, nw, pl, pu, pc, out.ctypes.data, status.ctypes.data)
        if rc != 0:
            _check(rc, "mlpg_hip_forward_host")
    return out, status


def backward_host(var, grad_out, windows, D, out_dtype=np.float32, lengths=None, algo=ALGO_AUTO, device=None):
    """MLPG backward, numpy in -> numpy out through mlpg_hip_backward_host (no torch involved): grad_out (B, T, sd)
    float32/float64 C-contiguous, var (B, T, D) / (D,) of the same dtype / None (unit variances), lengths int32 (B,) or None.
    Returns (grad (B, T, D) of out_dtype, status int32 (B, sd)).  The literal paramgen.mlpg_grad call and the backward of
    autograd.MLPG on CPU tensors: the library's short path (see forward_host), in pieces of whole utterances."""
    L = _host_lib()
    assert grad_out.ndim == 3 and grad_out.flags.c_contiguous and grad_out.dtype in (np.float32, np.float64)
    B, T, sd = grad_out.shape
    pw = cached_windows(windows)
    nw = pw[3]
    assert D == nw * sd
    pl, pu, pc = pw.ptrs()
    dt = F32 if grad_out.dtype == np.float32 else F64
    out_dtype = np.dtype(out_dtype)
    assert out_dtype in (np.float32, np.float64)
    mode, pv = _np_var(var, grad_out, (B, T, D), D)
    lengths, plen = _np_lengths(lengths, B)
    grad = np.empty((B, T, D), dtype=out_dtype)
    status = np.zeros((B, sd), dtype=np.int32)
    rc = L.mlpg_hip_backward_host(current_device_index(device), dt, F32 if out_dtype == np.float32 else F64, algo, pv, mode,
                                  grad_out.ctypes.data, plen, B, T, D, nw, pl, pu, pc, grad.ctypes.data, status.ctypes.data)
    if rc != 0:
        _check(rc, "mlpg_hip_backward_host")
    return grad, status


class _PinnedOwner(object):
    def __init__(self, ptr):
        self.ptr = ptr

    def __del__(self):
        try:
            if self.ptr:
                lib().mlpg_hip_host_free(ctypes.c_void_p(self.ptr))
        except Exception:  # interpreter shutdown
            pass


def pinned_empty(shape, dtype=np.float64):
    """An uninitialised numpy array in pinned (page-locked) host memory: forward_host transfers such arrays in place
    (no staging copy), at the PCIe rate."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    ptr = lib().mlpg_hip_host_alloc(max(n, 1))
    if not ptr:
        raise HipExtensionError("mlpg_hip_host_alloc failed: %s" % lib().mlpg_hip_last_error().decode())
    buf = (ctypes.c_char * max(n, 1)).from_address(ptr)
    buf._owner = _PinnedOwner(ptr)     # freed when the last array viewing this buffer goes away
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


class StreamDesc(ctypes.Structure):
    """mlpg_hip_stream_t (include/mlpg_hip.h)."""
    _fields_ = [("in_col", ctypes.c_int32), ("out_col", ctypes.c_int32), ("static_dim", ctypes.c_int32),
                ("num_windows", ctypes.c_int32), ("win_first", ctypes.c_int32)]


def _stream_table(streams):
    """The C stream table of a ``[(in_col, static_dim, windows)]`` list (forward_streams, backward_streams): (table, packed l[],
    u[], coeff[], number of windows, sum static_dim).  Output columns follow table order; window lists shared between streams
    (the same list object) are packed once."""
    table = (StreamDesc * max(len(streams), 1))()
    wl_all, wu_all, wc_all = [], [], []
    seen = {}                       # window lists shared between streams are packed once
    out_col = 0
    for k, (in_col, sd, windows) in enumerate(streams):
        nw = len(windows) if windows else 0
        first = 0
        if nw:
            key = id(windows)
            if key not in seen:
                wl, wu, wc = pack_windows(windows)
                seen[key] = len(wl_all)
                wl_all.extend(wl.tolist())
                wu_all.extend(wu.tolist())
                wc_all.extend(wc.tolist())
            first = seen[key]
        table[k] = StreamDesc(int(in_col), out_col, int(sd), nw, first)
        out_col += int(sd)
    wl = np.ascontiguousarray(wl_all, dtype=np.int32)
    wu = np.ascontiguousarray(wu_all, dtype=np.int32)
    wc = np.ascontiguousarray(wc_all if wc_all else [0.0], dtype=np.float64)
    return table, wl, wu, wc, len(wl_all), out_col


def forward_streams(mean, var, streams, lengths=None, algo=ALGO_AUTO, want_status=True):
    """Multi-stream MLPG over one (B, T, ld) CUDA batch, streams consumed in place.

    ``streams``: list of ``(in_col, static_dim, windows)``; ``windows`` is a list of (l, u, coeff)
    triples, or None / [] for a pass-through stream (static columns copied).  Trajectories are
    written side by side in table order.  Returns (out (B, T, sum static_dim), status (B, sum
    static_dim) int32 or None).
    """
    torch = torch_mod()
    assert mean.is_cuda and mean.dim() == 3 and mean.is_contiguous()
    B, T, ld = mean.shape
    mode = _var_mode(var, mean, mean.shape, ld)
    _check_lengths(lengths, B, mean.device)
    table, wl, wu, wc, n_win, out_col = _stream_table(streams)
    out = torch.empty((B, T, out_col), dtype=mean.dtype, device=mean.device)
    status = torch.empty((B, out_col), dtype=torch.int32, device=mean.device) if want_status else None
    rc = lib().mlpg_hip_forward_streams(mean.device.index, _stream(mean.device), _dt(mean), algo, _p(mean), _p(var), mode,
                                        ld, _p(lengths), B, T, len(streams), ctypes.addressof(table), n_win,
                                        _np(wl), _np(wu), _np(wc), _p(out), out_col, _p(status))
    _check(rc, "mlpg_hip_forward_streams")
    return out, status


def backward_streams(mean, var, y, grad_out, streams, lengths=None, algo=ALGO_AUTO, want_var=True):
    """Backward pass of forward_streams over one (B, T, ld) CUDA batch, gradients written in place (mlpg_hip_backward_streams).

    ``streams`` as in forward_streams; mean (B, T, ld), var of the same shape, (ld,) or None (unit variances: ``want_var`` must be
    False), y and grad_out (B, T, sum static_dim): the trajectory forward_streams returned and its gradient; one dtype, contiguous,
    on one device.  Returns (grad_mean (B, T, ld), grad_var (B, T, ld) or None, status int32 (B, sum static_dim)), enqueued on the
    current stream.  Columns of the (B, T, ld) gradients that belong to no stream are zero.  With (ld,) variances grad_var holds
    each frame's contribution: the gradient of the vector is its sum over (0, 1).  ``want_var=False``: only the means get a
    gradient (mean and y are not read and may be None).
    """
    torch = torch_mod()
    assert grad_out.is_cuda and grad_out.dim() == 3 and grad_out.is_contiguous()
    B, T, ld_out = grad_out.shape
    table, wl, wu, wc, n_win, out_col = _stream_table(streams)
    assert out_col == ld_out
    dev, dt = grad_out.device, grad_out.dtype
    if var is None:
        assert not want_var, "backward_streams: unit variances have no variances to differentiate"
        ld = mean.shape[2] if mean is not None else max([c + max(len(w) if w else 0, 1) * sd for c, sd, w in streams] + [0])
    else:
        ld = var.shape[-1]
    mode = _var_mode(var, grad_out, (B, T, ld), ld)
    if want_var:
        assert mean.shape == (B, T, ld) and mean.dtype == dt and mean.is_contiguous() and mean.device == dev
        assert y.shape == (B, T, ld_out) and y.dtype == dt and y.is_contiguous() and y.device == dev
    _check_lengths(lengths, B, dev)
    # (a table that covers every column -- the Merlin layout -- needs no fill: the library writes every element of its streams)
    covered = np.zeros(ld, dtype=bool)
    for c, sd, w in streams:
        covered[c:c + max(len(w) if w else 0, 1) * sd] = True
    alloc = torch.empty if covered.all() else torch.zeros
    grad_mean = alloc((B, T, ld), dtype=dt, device=dev)
    grad_var = alloc((B, T, ld), dtype=dt, device=dev) if want_var else None
    status = torch.empty((B, ld_out), dtype=torch.int32, device=dev)
    rc = lib().mlpg_hip_backward_streams(dev.index, _stream(dev), _dt(grad_out), algo, _p(mean) if want_var else None, _p(var), mode,
                                         ld, _p(y) if want_var else None, _p(grad_out), ld_out, _p(lengths), B, T, len(streams),
                                         ctypes.addressof(table), n_win, _np(wl), _np(wu), _np(wc), _p(grad_mean), _p(grad_var),
                                         _p(status))
    _check(rc, "mlpg_hip_backward_streams")
    return grad_mean, grad_var, status


def backward(var, grad_out, windows, D, lengths=None, out_dtype=None, algo=ALGO_AUTO, want_status=True):
    """Batched MLPG gradient w.r.t. means on device tensors.

    grad_out (B, T, sd); var (B, T, D), (D,) or None (unit).  Returns
    (grad_mean (B, T, D) in out_dtype (default float32), status).
    """
    torch = torch_mod()
    assert grad_out.is_cuda and grad_out.dim() == 3 and grad_out.is_contiguous()
    B, T, sd = grad_out.shape
    nw, pl, pu, pc, _keep = _win_args(windows)
    assert sd * nw == D
    mode = _var_mode(var, grad_out, (B, T, D), D)
    if out_dtype is None:
        out_dtype = torch.float32
    grad = torch.empty((B, T, D), dtype=out_dtype, device=grad_out.device)
    status = torch.empty((B * sd,), dtype=torch.int32, device=grad_out.device) if want_status else None
    rc = lib().mlpg_hip_backward(grad_out.device.index, _stream(grad_out.device), _dt(grad_out), _dt(grad), algo,
                                 _p(var), mode, _p(grad_out), _p(lengths), B, T, D, nw, pl, pu, pc,
                                 _p(grad), _p(status))
    _check(rc, "mlpg_hip_backward")
    return grad, status


def backward_var(mean, var, y, grad_out, windows, lengths=None, algo=ALGO_AUTO):
    """Batched MLPG gradient w.r.t. the means AND the variances on device tensors (mlpg_hip_backward_var).

    mean (B, T, D), var (B, T, D) or (D,), y (B, T, sd): the trajectory forward() returned for them, grad_out (B, T, sd); one
    dtype (float32 / float64), contiguous, on one device; lengths: cuda int32 (B,) or None.  Returns (grad_mean (B, T, D),
    grad_var (B, T, D), status int32 (B*sd)) in that dtype, enqueued on the current stream.  grad_mean is bit-identical to
    backward(var, grad_out, windows, D, lengths, out_dtype=dtype, algo=algo); with (D,) variances grad_var holds each frame's
    contribution, the gradient of the vector is its sum over (0, 1).
    """
    torch = torch_mod()
    assert grad_out.is_cuda and grad_out.dim() == 3 and grad_out.is_contiguous()
    B, T, sd = grad_out.shape
    nw, pl, pu, pc, _keep = _win_args(windows)
    D = sd * nw
    assert mean.shape == (B, T, D) and mean.dtype == grad_out.dtype and mean.is_contiguous() and mean.device == grad_out.device
    assert y.shape == (B, T, sd) and y.dtype == grad_out.dtype and y.is_contiguous() and y.device == grad_out.device
    assert var is not None, "backward_var: unit variances have no variances to differentiate"
    mode = _var_mode(var, grad_out, (B, T, D), D)
    _check_lengths(lengths, B, grad_out.device)
    grad_mean = torch.empty((B, T, D), dtype=grad_out.dtype, device=grad_out.device)
    grad_var = torch.empty((B, T, D), dtype=grad_out.dtype, device=grad_out.device)
    status = torch.empty((B * sd,), dtype=torch.int32, device=grad_out.device)
    rc = lib().mlpg_hip_backward_var(grad_out.device.index, _stream(grad_out.device), _dt(grad_out), algo, _p(mean), _p(var), mode,
                                     _p(y), _p(grad_out), _p(lengths), B, T, D, nw, pl, pu, pc, _p(grad_mean), _p(grad_var),
                                     _p(status))
    _check(rc, "mlpg_hip_backward_var")
    return grad_mean, grad_var, status


def delta_features(x, windows, lengths=None):
    """Batched delta features on device tensors: x (B, T, D) -> (B, T, D * len(windows))."""
    torch = torch_mod()
    assert x.is_cuda and x.dim() == 3 and x.is_contiguous()
    B, T, D = x.shape
    nw = len(windows)
    wl, wu, wc = pack_windows(windows)
    out = torch.empty((B, T, D * nw), dtype=x.dtype, device=x.device)
    rc = lib().mlpg_hip_delta_features(x.device.index, _stream(x.device), _dt(x), _p(x), _p(lengths), B, T, D, nw,
                                       _np(wl), _np(wu), _np(wc), _p(out))
    _check(rc, "mlpg_hip_delta_features")
    return out


def _f64_3d(x):
    torch = torch_mod()
    assert x.is_cuda and x.dim() == 3
    return x.to(torch.float64).contiguous()


def modspec(x, n, ortho=False, want_phase=False):
    """Power of the n-point DFT along time of a (B, T, D) CUDA batch: (ms (B, n/2+1, D), phase (B, n/2+1, D, 2) | None)."""
    torch = torch_mod()
    x = _f64_3d(x)
    B, T, D = x.shape
    ms = torch.empty((B, n // 2 + 1, D), dtype=torch.float64, device=x.device)
    ph = torch.empty((B, n // 2 + 1, D, 2), dtype=torch.float64, device=x.device) if want_phase else None
    _check(lib().mlpg_hip_modspec(x.device.index, _stream(x.device), _p(x), B, T, D, int(n), int(bool(ortho)), _p(ms), _p(ph)),
           "mlpg_hip_modspec")
    return ms, ph


def inv_modspec(ms, phase, ortho=False):
    """irfft of sqrt(ms) * phase: ms (B, nb, D), phase (B, nb, D, 2) float64 CUDA -> (B, 2*(nb-1), D)."""
    torch = torch_mod()
    ms = _f64_3d(ms)
    phase = phase.to(torch.float64).contiguous()
    B, nb, D = ms.shape
    assert phase.shape == (B, nb, D, 2)
    n = 2 * (nb - 1)
    out = torch.empty((B, n, D), dtype=torch.float64, device=ms.device)
    _check(lib().mlpg_hip_inv_modspec(ms.device.index, _stream(ms.device), _p(ms), _p(phase), B, n, D, int(bool(ortho)), _p(out)),
           "mlpg_hip_inv_modspec")
    return out


def modspec_smoothing(x, n, limit_bin, log_domain=True, ortho=False):
    """Remove the modulation bins >= limit_bin of every column of a (B, T, D) CUDA batch; returns (B, T, D) float64."""
    torch = torch_mod()
    x = _f64_3d(x)
    B, T, D = x.shape
    out = torch.empty((B, T, D), dtype=torch.float64, device=x.device)
    _check(lib().mlpg_hip_modspec_smoothing(x.device.index, _stream(x.device), _p(x), B, T, D, int(n), int(bool(ortho)),
                                            int(limit_bin), int(bool(log_domain)), _p(out)), "mlpg_hip_modspec_smoothing")
    return out


def modspec_backward(x, grad_ms, n, ortho=False):
    """Gradient of the power spectrum w.r.t. the trajectory: x (B, T, D), grad_ms (B, n/2+1, D) -> (B, T, D)."""
    torch = torch_mod()
    x = _f64_3d(x)
    g = _f64_3d(grad_ms)
    B, T, D = x.shape
    assert g.shape == (B, n // 2 + 1, D)
    out = torch.empty((B, T, D), dtype=torch.float64, device=x.device)
    _check(lib().mlpg_hip_modspec_backward(x.device.index, _stream(x.device), _p(x), _p(g), B, T, D, int(n), int(bool(ortho)),
                                           _p(out)), "mlpg_hip_modspec_backward")
    return out


def modspec_route(n):
    """mlpg_hip_modspec_route: the route modspec / inv_modspec / modspec_smoothing / modspec_backward take at DFT length n -- 0 the
    in-LDS FFT, 1 the direct transform, 2 chirp-z, -1 for n < 2 (the library's own decision, not a copy of it)."""
    return int(lib().mlpg_hip_modspec_route(int(n)))


def _batch_args(x, lengths):
    assert x.is_cuda and x.dim() == 3 and x.is_contiguous()
    _check_lengths(lengths, x.shape[0], x.device)
    return x.shape


def modspec_batch(x, n, ortho=False, lengths=None):
    """Power of the n-point DFT along time of a padded (B, Tmax, D) CUDA batch, float32 or float64, used in place
    (mlpg_hip_modspec_batch): utterance b contributes its first min(lengths[b], n) frames.  Returns ms (B, n/2+1, D) of x's dtype."""
    torch = torch_mod()
    B, T, D = _batch_args(x, lengths)
    ms = torch.empty((B, n // 2 + 1, D), dtype=x.dtype, device=x.device)
    _check(lib().mlpg_hip_modspec_batch(x.device.index, _stream(x.device), _dt(x), _p(x), _p(lengths), B, T, D, int(n),
                                        int(bool(ortho)), _p(ms)), "mlpg_hip_modspec_batch")
    return ms


def modspec_batch_backward(x, grad_ms, n, ortho=False, lengths=None):
    """Gradient of modspec_batch w.r.t. x (mlpg_hip_modspec_batch_backward): x (B, Tmax, D), grad_ms (B, n/2+1, D) of the same
    dtype -> (B, Tmax, D), every row written by the kernel (0 at and past each length)."""
    torch = torch_mod()
    B, T, D = _batch_args(x, lengths)
    assert grad_ms.shape == (B, n // 2 + 1, D) and grad_ms.dtype == x.dtype and grad_ms.device == x.device and grad_ms.is_contiguous()
    out = torch.empty_like(x)
    _check(lib().mlpg_hip_modspec_batch_backward(x.device.index, _stream(x.device), _dt(x), _p(x), _p(grad_ms), _p(lengths), B, T, D,
                                                 int(n), int(bool(ortho)), _p(out)), "mlpg_hip_modspec_batch_backward")
    return out


def modspec_loss_form(n):
    """mlpg_hip_modspec_loss_form: 1 when mlpg_hip_modspec_loss_step takes the DFT length n, 0 when the caller composes the loss."""
    return int(lib().mlpg_hip_modspec_loss_form(int(n)))


_MS_LOSS_WORKSPACE = {}       # (device, stream) -> uint8 tensor (mlpg_hip_modspec_loss_workspace_bytes; the content is irrelevant)


def _ms_loss_workspace(device, B, D):
    """The per-(device, stream) workspace of mlpg_hip_modspec_loss_step, grown geometrically (as _mse_workspace).  An outgrown
    tensor goes back to torch's allocator, which hands it out again behind the work of the stream it was allocated on."""
    torch = torch_mod()
    need = int(lib().mlpg_hip_modspec_loss_workspace_bytes(B, D))
    stream = _stream(device)
    key = (device.index, stream)
    ws = _MS_LOSS_WORKSPACE.get(key)
    if ws is None or ws.numel() < need:
        size = need if ws is None else max(need, ws.numel() * 3 // 2)
        ws = _MS_LOSS_WORKSPACE[key] = torch.empty((size + 4095) // 4096 * 4096, dtype=torch.uint8, device=device)
    return ws, stream


def modspec_loss_step(x, target_ms, n, ortho=False, lengths=None, log_domain=True, eps=1e-10, n_elems=None):
    """Fused modulation-spectrum loss step on device tensors (mlpg_hip_modspec_loss_step): x (B, Tmax, D), target_ms
    (B, n/2+1, D), float32 or float64.  Returns (loss float64 0-dim tensor = sum (f(MS(x)) - f(target_ms))^2 / n_elems,
    grad_x (B, Tmax, D) = d loss / d x); f = log(. + eps) or the identity.  n must be one modspec_loss_form answers 1 for.
    Enqueued on the current stream, no synchronisation.  The per-(device, stream) workspace is allocated on first use and again
    when a batch outgrows it: capturing the step into a graph is not supported."""
    torch = torch_mod()
    B, T, D = _batch_args(x, lengths)
    assert target_ms.shape == (B, n // 2 + 1, D) and target_ms.dtype == x.dtype and target_ms.device == x.device and \
        target_ms.is_contiguous()
    if n_elems is None:
        n_elems = float(B * (n // 2 + 1) * D)
    grad = torch.empty_like(x)
    loss = torch.empty((), dtype=torch.float64, device=x.device)
    ws, stream = _ms_loss_workspace(x.device, B, D)
    rc = lib().mlpg_hip_modspec_loss_step(x.device.index, stream, _dt(x), _p(x), _p(target_ms), _p(lengths), B, T, D, int(n),
                                          int(bool(ortho)), int(bool(log_domain)), float(eps), float(n_elems), _p(grad), _p(loss),
                                          _p(ws), ws.numel())
    _check(rc, "mlpg_hip_modspec_loss_step")
    return loss, grad


def trim_lengths(X, eps=1e-7):
    """int32 (N,) device tensor: frames left after the trailing-zero trim of each utterance."""
    torch = torch_mod()
    assert X.is_cuda and X.dim() == 3 and X.is_contiguous()
    N, T, D = X.shape
    lengths = torch.empty((N,), dtype=torch.int32, device=X.device)
    rc = lib().mlpg_hip_trim_lengths(X.device.index, _stream(X.device), _dt(X), _p(X), N, T, D, float(eps),
                                     _p(lengths))
    _check(rc, "mlpg_hip_trim_lengths")
    return lengths


DIST_L2, DIST_SCALED_L2_NP, DIST_SCALED_L1_NP, DIST_SCALED_SQL2_NP = 0, 1, 2, 3
TIE_FIRST_MIN, TIE_DIAG_LAST = 0, 1   # include/mlpg_hip.h MLPG_HIP_TIE_*


def fastdtw_l2(X, Y, lenx, leny, radius=1, dist_kind=DIST_L2, dist_scale=1.0, tie_rule=TIE_FIRST_MIN):
    """fastdtw paths for N pairs. Returns (path_i, path_j (N, Tx+Ty) int32, path_len (N,), cost (N,)).
    dist_kind / dist_scale: the local distance (include/mlpg_hip.h MLPG_HIP_DIST_*); tie_rule: MLPG_HIP_TIE_*."""
    torch = torch_mod()
    assert X.is_cuda and Y.is_cuda and X.dtype == torch.float64 and Y.dtype == torch.float64
    assert X.is_contiguous() and Y.is_contiguous() and X.dim() == 3 and Y.dim() == 3
    N, Tx, D = X.shape
    assert Y.shape[0] == N and Y.shape[2] == D
    Ty = Y.shape[1]
    dev = X.device
    path_i = torch.empty((N, Tx + Ty), dtype=torch.int32, device=dev)
    path_j = torch.empty((N, Tx + Ty), dtype=torch.int32, device=dev)
    path_len = torch.empty((N,), dtype=torch.int32, device=dev)
    cost = torch.empty((N,), dtype=torch.float64, device=dev)
    rc = lib().mlpg_hip_fastdtw(dev.index, _stream(dev), _p(X), _p(Y), _p(lenx), _p(leny), N, Tx, Ty, D,
                                int(radius), int(dist_kind), float(dist_scale), int(tie_rule), _p(path_i), _p(path_j),
                                _p(path_len), _p(cost))
    _check(rc, "mlpg_hip_fastdtw")
    return path_i, path_j, path_len, cost


def fastdtw_callable(xs, ys, radius, dist, tie_rule=TIE_FIRST_MIN, device=None):
    """fastdtw of N pairs for an ARBITRARY Python ``dist`` (what the reference hands to fastdtw, alignment.py:35-50):
    level by level from the coarsest, the local costs of each level's window cells evaluated HERE by ``dist`` -- one
    call per cell, as upstream fastdtw does -- and the DP recurrence, the back-trace and the window expansion on the GPU
    (mlpg_hip_dtw_level_windows / mlpg_hip_dtw_level_from_costs).  xs, ys: lists of (T, D) arrays (already trimmed).
    Returns numpy (path_i, path_j (N, max(tx+ty)) int32, path_len (N,), cost (N,) float64)."""
    torch = torch_mod()
    dev = require_gpu(device)
    N = len(xs)
    r = int(radius)
    # the halving pyramids, exactly upstream's __reduce_by_half (pairwise means, odd tail dropped), in float64
    px, py, Kn = [], [], []
    for x, y in zip(xs, ys):
        lx, ly = [np.asanyarray(x, dtype="float")], [np.asanyarray(y, dtype="float")]
        while not (len(lx[-1]) < r + 2 or len(ly[-1]) < r + 2):
            for l in (lx, ly):
                a = l[-1]
                h = len(a) // 2
                l.append((a[0:2 * h:2] + a[1:2 * h:2]) / 2)
        px.append(lx)
        py.append(ly)
        Kn.append(len(lx) - 1)
    tx0 = np.asarray([len(l[0]) for l in px], dtype=np.int64)
    ty0 = np.asarray([len(l[0]) for l in py], dtype=np.int64)
    row_stride = int(tx0.max())
    max_ty = int(ty0.max())
    path_stride = int((tx0 + ty0).max())
    i32 = dict(dtype=torch.int32, device=dev)
    path_i = torch.zeros((N, path_stride), **i32)
    path_j = torch.zeros((N, path_stride), **i32)
    path_len = torch.zeros((N,), **i32)
    cost = torch.zeros((N,), dtype=torch.float64, device=dev)
    row_lo = torch.zeros((N, row_stride), **i32)
    row_hi = torch.zeros((N, row_stride), **i32)
    row_off = torch.zeros((N, row_stride + 1), dtype=torch.int64, device=dev)
    st = _stream(dev)
    L = lib()
    for k in range(max(Kn), -1, -1):
        ltx = np.asarray([(int(tx0[n]) >> k) if k <= Kn[n] else 0 for n in range(N)], dtype=np.int32)
        lty = np.asarray([(int(ty0[n]) >> k) if k <= Kn[n] else 0 for n in range(N)], dtype=np.int32)
        full = np.asarray([1 if k == Kn[n] else 0 for n in range(N)], dtype=np.int32)
        d_tx, d_ty, d_full = (torch.from_numpy(a).to(dev) for a in (ltx, lty, full))
        _check(L.mlpg_hip_dtw_level_windows(dev.index, st, N, r, _p(d_tx), _p(d_ty), _p(d_full), _p(path_i), _p(path_j),
                                            _p(path_len), path_stride, _p(row_lo), _p(row_hi), _p(row_off), row_stride),
               "mlpg_hip_dtw_level_windows")
        lo, hi, off = row_lo.cpu().numpy(), row_hi.cpu().numpy(), row_off.cpu().numpy()
        ncell = np.asarray([int(off[n, ltx[n]]) if ltx[n] > 0 else 0 for n in range(N)], dtype=np.int64)
        base = np.concatenate([[0], np.cumsum(ncell)]).astype(np.int64)
        costs = np.empty(max(1, int(base[-1])), dtype=np.float64)
        for n in range(N):
            if ltx[n] <= 0:
                continue
            xk, yk = px[n][k], py[n][k]
            q = int(base[n])
            for i in range(int(ltx[n])):
                xi = xk[i]
                for j in range(int(lo[n, i]), int(hi[n, i]) + 1):
                    costs[q] = dist(xi, yk[j])          # the user's callable, once per window cell
                    q += 1
        d_costs = torch.from_numpy(costs).to(dev)
        d_base = torch.from_numpy(base[:N].copy()).to(dev)
        _check(L.mlpg_hip_dtw_level_from_costs(dev.index, st, N, int(tie_rule), _p(d_tx), _p(d_ty), _p(row_lo), _p(row_hi),
                                               _p(row_off), row_stride, max_ty, _p(d_costs), _p(d_base), int(base[-1]),
                                               _p(path_i), _p(path_j), _p(path_len), path_stride, _p(cost)),
               "mlpg_hip_dtw_level_from_costs")
        torch.cuda.current_stream(dev).synchronize()     # the level's host buffers are released only now
    pl = path_len.cpu().numpy()
    pi, pj = path_i.cpu().numpy(), path_j.cpu().numpy()
    return pi, pj, pl, cost.cpu().numpy()


def fastdtw_host(X, Y, radius=1, dist_kind=DIST_L2, dist_scale=1.0, lenx=None, leny=None, eps=1e-7, device=None,
                 tie_rule=TIE_FIRST_MIN):
    """fastdtw paths for N pairs held in numpy arrays (no framework tensor): mlpg_hip_fastdtw_host, chunked and
    overlapped with the transfers.  X (N, Tx, D), Y (N, Ty, D) float32 / float64.  Without lengths the trailing
    all-zero frames are trimmed on the device (eps as trim_zeros_frames).  Returns numpy
    (path_i, path_j (N, Tx+Ty) int32, path_len (N,), cost (N,), lenx, leny)."""
    L = lib()
    if not X.flags.c_contiguous:
        X = np.ascontiguousarray(X)
    if not Y.flags.c_contiguous:
        Y = np.ascontiguousarray(Y)
    # one dtype for the C entry point; mixed or non-float inputs are WIDENED to float64 (each array from its own
    # dtype, as the device route and the reference's fastdtw do), never narrowed
    if X.dtype != Y.dtype or X.dtype not in (np.float32, np.float64):
        X = X.astype(np.float64, copy=False)
        Y = Y.astype(np.float64, copy=False)
    assert X.ndim == 3 and Y.ndim == 3 and X.shape[0] == Y.shape[0] and X.shape[2] == Y.shape[2]
    N, Tx, D = X.shape
    Ty = Y.shape[1]
    # (the library fills every slot: the path's entries, zeros behind them -- nothing to clear here; addresses as ints: numpy's
    # `.ctypes.data_as` costs microseconds per argument, and DTWAligner.transform on one pair is a 0.3 ms call)
    path_i = np.empty((N, Tx + Ty), dtype=np.int32)
    path_j = np.empty((N, Tx + Ty), dtype=np.int32)
    small = np.zeros((3, N), dtype=np.int32)           # path_len, lenx, leny
    path_len, lx_out, ly_out = small[0], small[1], small[2]
    cost = np.zeros((N,), dtype=np.float64)
    plx = ply = None
    if lenx is not None:
        lenx = np.ascontiguousarray(lenx, dtype=np.int32)
        leny = np.ascontiguousarray(leny, dtype=np.int32)
        plx, ply = lenx.ctypes.data, leny.ctypes.data
    dt = F32 if X.dtype == np.float32 else F64
    tail = (N, Tx, Ty, D, int(radius), int(dist_kind), float(dist_scale), int(tie_rule), float(eps),
            path_i.ctypes.data, path_j.ctypes.data, path_len.ctypes.data, cost.ctypes.data, lx_out.ctypes.data, ly_out.ctypes.data)
    if isinstance(device, (list, tuple, np.ndarray)) or (isinstance(device, str) and device == "all"):
        devs = device_list(device)
        rc = L.mlpg_hip_fastdtw_host_multi(_np(devs) if len(devs) else None, len(devs), dt, X.ctypes.data, Y.ctypes.data, plx, ply, *tail)
    else:
        rc = L.mlpg_hip_fastdtw_host(current_device_index(device), dt, X.ctypes.data, Y.ctypes.data, plx, ply, *tail)
    if rc != 0:
        _check(rc, "mlpg_hip_fastdtw_host")
    return path_i, path_j, path_len, cost, lx_out, ly_out


def gather_path(src, path, path_len, Tout):
    """out[n, k] = src[n, path[n, k]] for k < path_len[n], zeros after. (N, Tout, D)."""
    torch = torch_mod()
    assert src.is_cuda and src.dim() == 3 and src.is_contiguous() and path.is_contiguous()
    N, Tsrc, D = src.shape
    out = torch.empty((N, Tout, D), dtype=src.dtype, device=src.device)
    rc = lib().mlpg_hip_gather_path(src.device.index, _stream(src.device), _dt(src), _p(src), _p(path),
                                    _p(path_len), N, Tsrc, path.shape[1], D, Tout, _p(out))
    _check(rc, "mlpg_hip_gather_path")
    return out


_MSE_WORKSPACE = {}           # (device, stream) -> [tensor, used inside a stream capture]
_MSE_WORKSPACE_RETIRED = []   # outgrown workspaces a captured graph may still replay kernels on (only those: see below)
_MSE_NEED = {}                # (B, T, D, nw, with FIR dy buffer) -> bytes (mlpg_hip_unit_mse_workspace_bytes[_t])
_MSE_FORM = {}                # (device, dtype, lengths given, B, T, D, id(packed windows)) -> (packed windows, form): settled answers only


def unit_mse_form(device, dtype, has_lengths, B, T, D, windows):
    """Which form mlpg_hip_unit_mse_step takes (mlpg_hip_unit_mse_form: the library's own decision, not a copy of it):
    2 the FIR form, 1 the one-launch kernel, 0 neither.  Answers for a PackedWindows object are remembered, except a
    "not 2" given while the stream is being captured (the tap table could not be built then; it may exist later)."""
    torch = torch_mod()
    packed = isinstance(windows, PackedWindows)
    key = (device.index, dtype, bool(has_lengths), B, T, D, id(windows)) if packed else None
    if key is not None:
        hit = _MSE_FORM.get(key)
        if hit is not None and hit[0] is windows:
            return hit[1]
    nw, pl, pu, pc, _keep = _win_args(windows)
    form = lib().mlpg_hip_unit_mse_form(device.index, _stream(device), F32 if dtype == torch.float32 else F64, 1 if has_lengths else 0,
                                        B, T, D, nw, pl, pu, pc)
    if form < 0:
        _check(form, "mlpg_hip_unit_mse_form")
    if key is not None and (form == 2 or not torch.cuda.is_current_stream_capturing()):
        if len(_MSE_FORM) > 1024:
            _MSE_FORM.clear()
        _MSE_FORM[key] = (windows, form)
    return form


def _mse_workspace(device, B, T, D, nw, fir_form):
    """The per-(device, stream) workspace of mlpg_hip_unit_mse_step.  Zeroed once (the kernel leaves its arrival counter
    zero); grown geometrically (length-bucketed or ascending batches would otherwise reallocate at almost every new
    maximum); the FIR form's dy buffer (B * T * sd floats) is only asked for by batches that take that form.  A workspace
    is never created or grown while its stream is being captured -- the allocation would come from the graph's private
    pool and its one-time zero fill would become a node of the graph, replayed behind other launches' backs: warm up one
    step of the largest shape before capturing.  An outgrown buffer is kept alive only if a stream capture has used it (a
    graph may still replay kernels on it)."""
    torch = torch_mod()
    nk = (B, T, D, nw, fir_form)
    need = _MSE_NEED.get(nk)
    if need is None:
        L = lib()
        need = int(L.mlpg_hip_unit_mse_workspace_bytes_t(B, T, D, nw) if fir_form else L.mlpg_hip_unit_mse_workspace_bytes(B, D, nw))
        if len(_MSE_NEED) > 4096:
            _MSE_NEED.clear()
        _MSE_NEED[nk] = need
    stream = _stream(device)
    key = (device.index, stream)
    ent = _MSE_WORKSPACE.get(key)
    capturing = torch.cuda.is_current_stream_capturing()
    if ent is None or ent[0].numel() < need:
        if capturing:
            raise HipExtensionError(
                "unit_mse_step: the workspace of this stream does not exist yet or is too small (%d bytes needed) and cannot be "
                "allocated while the stream is being captured -- run one eager step of this shape on the capturing stream first "
                "(torch.cuda.graph(g, stream=s) with the stream s the warm-up ran on: the default capture stream is torch's own)" % need)
        size = need if ent is None else max(need, ent[0].numel() * 3 // 2)
        if ent is not None and ent[1]:
            _MSE_WORKSPACE_RETIRED.append(ent[0])
        ent = [torch.zeros((size + 4095) // 4096 * 4096, dtype=torch.uint8, device=device), False]
        _MSE_WORKSPACE[key] = ent
    if capturing:
        ent[1] = True
    return ent[0], stream


def unit_mse_step(mean, target, windows, lengths=None, n_elems=None, want_y=False, want_status=False):
    """Fused unit-variance MLPG + MSE training step on device tensors (mlpg_hip_unit_mse_step): mean (B, T, D), target
    (B, T, D / nw), float32 or float64.  Returns (loss float64 0-dim tensor, grad_mean (B, T, D), y or None, status or None).
    One launch (the wave-per-system kernel: window extents <= 1, T <= 1024), or two in the FIR form (float32, no lengths, T >= 96,
    window extents <= 2, any T, a window set whose inverse decays: unit_mse_form says which)."""
    torch = torch_mod()
    assert mean.is_cuda and mean.dim() == 3 and mean.is_contiguous() and target.is_contiguous()
    B, T, D = mean.shape
    nw, pl, pu, pc, _keep = _win_args(windows)
    sd = D // nw
    assert target.shape == (B, T, sd) and target.dtype == mean.dtype and target.device == mean.device
    if lengths is not None:
        assert lengths.dtype == torch.int32 and lengths.shape == (B,) and lengths.device == mean.device
    if n_elems is None:
        n_elems = float(B * T * sd)
    grad = torch.empty_like(mean)
    y = torch.empty_like(target) if want_y else None
    loss = torch.empty((), dtype=torch.float64, device=mean.device)
    status = torch.empty((B * sd,), dtype=torch.int32, device=mean.device) if want_status else None
    # (the FIR form needs room for its dy buffer: the library says whether this call takes it)
    fir_form = mean.dtype == torch.float32 and lengths is None and T >= 96 and \
        unit_mse_form(mean.device, mean.dtype, False, B, T, D, windows) == 2
    ws, stream = _mse_workspace(mean.device, B, T, D, nw, fir_form)
    rc = lib().mlpg_hip_unit_mse_step(mean.device.index, stream, _dt(mean), _p(mean), _p(target), _p(lengths),
                                      B, T, D, nw, pl, pu, pc, float(n_elems), _p(y), _p(grad), _p(loss),
                                      _p(status), _p(ws), ws.numel())
    _check(rc, "mlpg_hip_unit_mse_step")
    return loss, grad, y, status


def stream_copy(src, dst):
    """dst[...] = src[...] by the library's plain streaming-copy kernel (measurement aid: the HBM rate a copy reaches)."""
    assert src.is_cuda and dst.is_cuda and src.is_contiguous() and dst.is_contiguous()
    nbytes = src.numel() * src.element_size()
    assert nbytes == dst.numel() * dst.element_size() and nbytes % 16 == 0
    _check(lib().mlpg_hip_stream_copy(src.device.index, _stream(src.device), _p(src), _p(dst), nbytes), "mlpg_hip_stream_copy")


def gmm_convert(x, posterior, mixture, mu_x, mu_y, A):
    """out[n] = sum_m posterior[n, m] (mu_y[m] + A[m] (x[n] - mu_x[m])) on the GPU; float64 CUDA tensors:
    x (N, D), posterior (N, M) or None, mixture int32 (N) or None, mu_x (M, D), mu_y (M, Dy), A (M, Dy, D)."""
    torch = torch_mod()
    assert x.is_cuda and x.dtype == torch.float64 and x.dim() == 2 and x.is_contiguous()
    N, D = x.shape
    M, Dy = mu_y.shape
    assert mu_x.shape == (M, D) and A.shape == (M, Dy, D) and A.is_contiguous()
    out = torch.empty((N, Dy), dtype=torch.float64, device=x.device)
    rc = lib().mlpg_hip_gmm_convert(x.device.index, _stream(x.device), _p(x), _p(posterior), _p(mixture), _p(mu_x),
                                    _p(mu_y), _p(A), N, D, Dy, M, _p(out))
    _check(rc, "mlpg_hip_gmm_convert")
    return out


GMM_MAX_FEATURES, GMM_MAX_COMPONENTS = 128, 64     # the limits of the mlpg_hip_gmm_* entry points


def _gmm_x(X):
    torch = torch_mod()
    assert X.is_cuda and X.dtype == torch.float64 and X.dim() == 2 and X.is_contiguous()
    return X.shape


def gmm_workspace(device, N, F, K):
    """A uint8 CUDA tensor of mlpg_hip_gmm_workspace_bytes(N, F, K) bytes (its content is irrelevant)."""
    torch = torch_mod()
    need = int(lib().mlpg_hip_gmm_workspace_bytes(int(N), int(F), int(K)))
    return torch.empty(max(need, 256), dtype=torch.uint8, device=device)


def gmm_estep(X, weights, means, prec_chol, log_det, want_resp=True, want_log_prob_norm=False, want_labels=False, want_mean=False,
              workspace=None):
    """mlpg_hip_gmm_estep on float64 CUDA tensors: X (N, F), weights (K), means (K, F), prec_chol (K, F, F), log_det (K).
    Returns (resp (N, K), log_prob_norm (N), labels int32 (N), mean of log_prob_norm as a 0-dim tensor), None where not asked
    for; enqueued on the current stream."""
    torch = torch_mod()
    N, F = _gmm_x(X)
    K = means.shape[0]
    dev = X.device
    for t, shape in ((weights, (K,)), (means, (K, F)), (prec_chol, (K, F, F)), (log_det, (K,))):
        assert t.shape == shape and t.dtype == torch.float64 and t.is_contiguous() and t.device == dev
    resp = torch.empty((N, K), dtype=torch.float64, device=dev) if want_resp else None
    lpn = torch.empty((N,), dtype=torch.float64, device=dev) if want_log_prob_norm else None
    labels = torch.empty((N,), dtype=torch.int32, device=dev) if want_labels else None
    mean = torch.empty((), dtype=torch.float64, device=dev) if want_mean else None
    if want_mean and workspace is None:
        workspace = gmm_workspace(dev, N, F, K)
    rc = lib().mlpg_hip_gmm_estep(dev.index, _stream(dev), _p(X), _p(weights), _p(means), _p(prec_chol), _p(log_det), N, F, K,
                                  _p(resp), _p(lpn), _p(labels), _p(mean), _p(workspace),
                                  workspace.numel() if workspace is not None else 0)
    _check(rc, "mlpg_hip_gmm_estep")
    return resp, lpn, labels, mean


def gmm_mstep(X, resp, reg_covar, workspace=None):
    """mlpg_hip_gmm_mstep on float64 CUDA tensors: X (N, F), resp (N, K) -> (weights (K), means (K, F), covariances (K, F, F))."""
    torch = torch_mod()
    N, F = _gmm_x(X)
    K = resp.shape[1]
    dev = X.device
    assert resp.shape == (N, K) and resp.dtype == torch.float64 and resp.is_contiguous() and resp.device == dev
    weights = torch.empty((K,), dtype=torch.float64, device=dev)
    means = torch.empty((K, F), dtype=torch.float64, device=dev)
    cov = torch.empty((K, F, F), dtype=torch.float64, device=dev)
    if workspace is None:
        workspace = gmm_workspace(dev, N, F, K)
    rc = lib().mlpg_hip_gmm_mstep(dev.index, _stream(dev), _p(X), _p(resp), N, F, K, float(reg_covar), _p(weights), _p(means),
                                  _p(cov), _p(workspace), workspace.numel())
    _check(rc, "mlpg_hip_gmm_mstep")
    return weights, means, cov


def gmm_precisions(cov):
    """mlpg_hip_gmm_precisions: covariances (K, F, F) float64 CUDA -> (prec_chol (K, F, F), log_det (K), status int32 (K))."""
    torch = torch_mod()
    assert cov.is_cuda and cov.dtype == torch.float64 and cov.dim() == 3 and cov.is_contiguous() and cov.shape[1] == cov.shape[2]
    K, F, _ = cov.shape
    dev = cov.device
    U = torch.zeros((K, F, F), dtype=torch.float64, device=dev)
    log_det = torch.zeros((K,), dtype=torch.float64, device=dev)
    status = torch.empty((K,), dtype=torch.int32, device=dev)
    rc = lib().mlpg_hip_gmm_precisions(dev.index, _stream(dev), _p(cov), F, K, _p(U), _p(log_det), _p(status))
    _check(rc, "mlpg_hip_gmm_precisions")
    return U, log_det, status


KMEANS_MAX_CANDIDATES = 8     # candidates of one mlpg_hip_kmeans_seed_step


def kmeans_workspace(device, N, F, K):
    """A uint8 CUDA tensor of mlpg_hip_kmeans_workspace_bytes(N, F, K) bytes (its content is irrelevant)."""
    torch = torch_mod()
    need = int(lib().mlpg_hip_kmeans_workspace_bytes(int(N), int(F), int(K)))
    return torch.empty(max(need, 256), dtype=torch.uint8, device=device)


def kmeans_seed_step(X, shift, candidates, closest=None, workspace=None):
    """mlpg_hip_kmeans_seed_step on CUDA tensors: X (N, F) float64, shift (F) float64 or None, candidates int32 (C), closest (N)
    float64 or None -> (d (C, N), pots (C)); enqueued on the current stream."""
    torch = torch_mod()
    N, F = _gmm_x(X)
    dev = X.device
    C = candidates.shape[0]
    assert candidates.shape == (C,) and candidates.dtype == torch.int32 and candidates.is_contiguous() and candidates.device == dev
    for t, shape in ((shift, (F,)), (closest, (N,))):
        assert t is None or (t.shape == shape and t.dtype == torch.float64 and t.is_contiguous() and t.device == dev)
    d = torch.empty((C, N), dtype=torch.float64, device=dev)
    pots = torch.empty((C,), dtype=torch.float64, device=dev)
    if workspace is None:
        workspace = kmeans_workspace(dev, N, F, 1)
    rc = lib().mlpg_hip_kmeans_seed_step(dev.index, _stream(dev), _p(X), _p(shift), N, F, _p(candidates), C, _p(closest), _p(d),
                                         _p(pots), _p(workspace), workspace.numel())
    _check(rc, "mlpg_hip_kmeans_seed_step")
    return d, pots


def kmeans_lloyd_step(X, shift, centers, labels_prev, update_centers=True, want_min_dist=False, workspace=None):
    """mlpg_hip_kmeans_lloyd_step on CUDA tensors: X (N, F) float64, shift (F) float64 or None, centers (K, F) float64,
    labels_prev int32 (N) -> (labels int32 (N), min_dist (N) or None, sums (K, F), counts (K), centers_out (K, F) or None, stats).
    stats: int64 (4) holding the bits of (double shift, double inertia, int64 changed, int64 empty) -- kmeans_stats reads it."""
    torch = torch_mod()
    N, F = _gmm_x(X)
    dev = X.device
    K = centers.shape[0]
    assert labels_prev.shape == (N,) and labels_prev.dtype == torch.int32 and labels_prev.is_contiguous() and labels_prev.device == dev
    for t, shape in ((shift, (F,)), (centers, (K, F))):
        assert t is None or (t.shape == shape and t.dtype == torch.float64 and t.is_contiguous() and t.device == dev)
    labels = torch.empty((N,), dtype=torch.int32, device=dev)
    min_dist = torch.empty((N,), dtype=torch.float64, device=dev) if want_min_dist else None
    sums = torch.empty((K, F), dtype=torch.float64, device=dev)
    counts = torch.empty((K,), dtype=torch.float64, device=dev)
    centers_out = torch.empty((K, F), dtype=torch.float64, device=dev) if update_centers else None
    stats = torch.empty((4,), dtype=torch.int64, device=dev)
    if workspace is None:
        workspace = kmeans_workspace(dev, N, F, K)
    rc = lib().mlpg_hip_kmeans_lloyd_step(dev.index, _stream(dev), _p(X), _p(shift), _p(centers), _p(labels_prev), N, F, K,
                                          1 if update_centers else 0, _p(labels), _p(min_dist), _p(sums), _p(counts),
                                          _p(centers_out), _p(stats), _p(workspace), workspace.numel())
    _check(rc, "mlpg_hip_kmeans_lloyd_step")
    return labels, min_dist, sums, counts, centers_out, stats


def kmeans_stats(stats):
    """(shift, inertia, changed, empty) of a Lloyd step's statistics record: the step's one read-back."""
    raw = stats.cpu().numpy()
    fl = raw.view(np.float64)
    return float(fl[0]), float(fl[1]), int(raw[2]), int(raw[3])


POSTFILTER_FRAME_TILE = 64      # MLPG_HIP_POSTFILTER_FRAME_TILE: frames per workgroup of mlpg_hip_merlin_post_filter
POSTFILTER_MAX_DIM, POSTFILTER_MIN_FFT, POSTFILTER_MAX_FFT = 64, 4, 4096
_PF_TABLES = {}                 # (device index, D, alpha, order, fftlen) -> G on that device; a few entries, oldest out first
_PF_TABLES_MAX = 8


def postfilter_check(D, alpha, order, fftlen):
    """ValueError for sizes outside the limits of the post-filter entries (the C entries refuse the same)."""
    if not 1 <= D <= POSTFILTER_MAX_DIM:
        raise ValueError("merlin_post_filter: the number of coefficients must be in [1, %d] (got %d)" % (POSTFILTER_MAX_DIM, D))
    if fftlen < POSTFILTER_MIN_FFT or fftlen > POSTFILTER_MAX_FFT or fftlen & (fftlen - 1):
        raise ValueError("merlin_post_filter: fftlen must be a power of two in [%d, %d] (got %d)"
                         % (POSTFILTER_MIN_FFT, POSTFILTER_MAX_FFT, fftlen))
    if not D - 1 <= order < fftlen:
        raise ValueError("merlin_post_filter: minimum_phase_order must be in [D - 1, fftlen) = [%d, %d) (got %d)" % (D - 1, fftlen, order))
    if not abs(alpha) < 1.0:
        raise ValueError("merlin_post_filter: |alpha| must be below 1 (got %r)" % (alpha,))


def postfilter_table_host(D, alpha, order, fftlen):
    """mlpg_hip_postfilter_table: G (fftlen/2 + 1, D) float64 as a numpy array (host code: no GPU needed)."""
    D, alpha, order, fftlen = int(D), float(alpha), int(order), int(fftlen)
    postfilter_check(D, alpha, order, fftlen)
    G = np.empty((fftlen // 2 + 1, D), dtype=np.float64)
    _check(lib().mlpg_hip_postfilter_table(D, alpha, order, fftlen, _np(G)), "mlpg_hip_postfilter_table")
    return G


def postfilter_table(device, D, alpha, order, fftlen):
    """The table on `device`, remembered per (device, D, alpha, order, fftlen): building it costs milliseconds on the host."""
    torch = torch_mod()
    key = (device.index, int(D), float(alpha), int(order), int(fftlen))
    with _lock:
        G = _PF_TABLES.get(key)
    if G is None:
        G = torch.from_numpy(postfilter_table_host(*key[1:])).to(device)
        with _lock:
            while len(_PF_TABLES) >= _PF_TABLES_MAX:
                _PF_TABLES.pop(next(iter(_PF_TABLES)))
            _PF_TABLES[key] = G
    return G


def _pf_row_stride(t, B, T, D, who="merlin_post_filter"):
    """The row stride ld of a (B, T, D) view of a dense (B, T, ld) array (columns contiguous, utterance stride T * ld)."""
    s0, s1, s2 = t.stride()
    ld = s1 if T > 1 else (s0 if B > 1 else D)
    if B * T and ((D > 1 and s2 != 1) or ld < D or (T > 1 and B > 1 and s0 != T * ld)):
        raise HipExtensionError("%s: needs a column slice of a dense (B, Tmax, ld) tensor, got strides %s"
                                % (who, (s0, s1, s2)))
    return ld


def merlin_post_filter(mgc, alpha, weight, G, fftlen, lengths=None, out=None):
    """mlpg_hip_merlin_post_filter on CUDA tensors: mgc (B, Tmax, D) float32 / float64 whose last dimension is contiguous and
    whose first two are those of a dense (B, Tmax, ld) array (a column slice of one is fine), weight (D) float64, G the table
    (fftlen/2 + 1, D), lengths int32 (B) or None, out like mgc (None: a new dense tensor; mgc itself: in place).  Enqueued on the
    current stream."""
    torch = torch_mod()
    assert mgc.is_cuda and mgc.dim() == 3
    B, T, D = mgc.shape
    dev = mgc.device
    if out is None:
        out = torch.empty((B, T, D), dtype=mgc.dtype, device=dev)
    assert out.shape == mgc.shape and out.dtype == mgc.dtype and out.device == dev
    lds = [_pf_row_stride(t, B, T, D) for t in (mgc, out)]
    for t, shape in ((weight, (D,)), (G, (fftlen // 2 + 1, D))):
        assert t.shape == shape and t.dtype == torch.float64 and t.is_contiguous() and t.device == dev
    _check_lengths(lengths, B, dev)
    rc = lib().mlpg_hip_merlin_post_filter(dev.index, _stream(dev), _dt(mgc), _p(mgc), lds[0], _p(lengths), B, T, D, float(alpha),
                                           _p(weight), _p(G), int(fftlen), _p(out), lds[1])
    _check(rc, "mlpg_hip_merlin_post_filter")
    return out


def modspec_filter_form(n):
    """mlpg_hip_modspec_filter_form: 1 when mlpg_hip_modspec_filter takes the DFT length n, 0 when the caller composes the filter."""
    return int(lib().mlpg_hip_modspec_filter_form(int(n)))


def modspec_filter(x, n, A=None, C=None, limit_bin=None, log_domain=True, ortho=False, lengths=None, out=None):
    """mlpg_hip_modspec_filter on CUDA tensors: x (B, Tmax, D) float32 / float64, a column slice of a dense (B, Tmax, ld) tensor
    or dense itself; A, C float64 (n/2 + 1, D) or both None; limit_bin in [0, n/2 + 1] (None: n/2 + 1, nothing removed);
    lengths int32 (B) or None; out like x (None: a new dense tensor; x itself: in place).  Enqueued on the current stream."""
    torch = torch_mod()
    assert x.is_cuda and x.dim() == 3
    B, T, D = x.shape
    dev = x.device
    nb = int(n) // 2 + 1
    if out is None:
        out = torch.empty((B, T, D), dtype=x.dtype, device=dev)
    assert out.shape == x.shape and out.dtype == x.dtype and out.device == dev
    lds = [_pf_row_stride(t, B, T, D, "modspec_filter") for t in (x, out)]
    for t in (A, C):
        assert t is None or (t.shape == (nb, D) and t.dtype == torch.float64 and t.is_contiguous() and t.device == dev)
    _check_lengths(lengths, B, dev)
    rc = lib().mlpg_hip_modspec_filter(dev.index, _stream(dev), _dt(x), _p(x), lds[0], _p(lengths), B, T, D, int(n), int(bool(ortho)),
                                       _p(A), _p(C), nb if limit_bin is None else int(limit_bin), int(bool(log_domain)), _p(out),
                                       lds[1])
    _check(rc, "mlpg_hip_modspec_filter")
    return out


GMM_TRAJ_ROW_TILE = 64          # MLPG_HIP_GMM_TRAJ_ROW_TILE: rows of the (B * Tmax) axis per workgroup of mlpg_hip_gmm_trajectory_stats
GMM_TRAJ_MAX_MIXTURES = 65536


def gmm_trajectory_stats(x, lengths, labels, mu_x, mu_y, A, cvar, mean=None, var=None):
    """mlpg_hip_gmm_trajectory_stats on float64 CUDA tensors: x (B, Tmax, D) whose last dimension is contiguous and whose first
    two are those of a dense (B, Tmax, ld) array (a column slice of one is fine), lengths int32 (B) or None, labels int32
    (B, Tmax) or (B * Tmax), mu_x, mu_y, cvar (M, D), A (M, D, D).  Returns (mean, var), each (B, Tmax, D): mu_y[m] + A[m] (x -
    mu_x[m]) and cvar[m] for the label m of a live row, 0 and 1 on the rows past an utterance's length.  mean / var: where to
    write them (column slices allowed; columns outside are not touched), new dense tensors when None.  Enqueued on the current
    stream."""
    torch = torch_mod()
    for name, t in (("x", x), ("mu_x", mu_x), ("mu_y", mu_y), ("A", A), ("cvar", cvar), ("mean", mean), ("var", var)):
        if t is not None and (not torch.is_tensor(t) or t.dtype != torch.float64 or not t.is_cuda):
            raise ValueError("gmm_trajectory_stats: %s must be a float64 CUDA tensor, got %s"
                             % (name, "%s on %s" % (t.dtype, t.device) if torch.is_tensor(t) else type(t).__name__))
    if not torch.is_tensor(labels) or labels.dtype != torch.int32 or not labels.is_cuda:
        raise ValueError("gmm_trajectory_stats: labels must be an int32 CUDA tensor")
    if x.dim() != 3:
        raise ValueError("gmm_trajectory_stats: x must be (B, Tmax, D), got %d dimensions" % x.dim())
    B, T, D = x.shape
    M = mu_x.shape[0]
    if not 1 <= D <= GMM_MAX_FEATURES or not 1 <= M <= GMM_TRAJ_MAX_MIXTURES:
        raise ValueError("gmm_trajectory_stats: takes 1 to %d features and 1 to %d mixtures, got %d and %d"
                         % (GMM_MAX_FEATURES, GMM_TRAJ_MAX_MIXTURES, D, M))
    dev = x.device
    for t, shape in ((mu_x, (M, D)), (mu_y, (M, D)), (A, (M, D, D)), (cvar, (M, D))):
        if t.shape != shape or not t.is_contiguous() or t.device != dev:
            raise ValueError("gmm_trajectory_stats: the model tensors must be contiguous (M, D), (M, D), (M, D, D), (M, D) on x's device")
    if labels.numel() != B * T or not labels.is_contiguous() or labels.device != dev:
        raise ValueError("gmm_trajectory_stats: labels must hold B * Tmax = %d contiguous entries on x's device" % (B * T))
    _check_lengths(lengths, B, dev)
    if mean is None:
        mean = torch.empty((B, T, D), dtype=torch.float64, device=dev)
    if var is None:
        var = torch.empty((B, T, D), dtype=torch.float64, device=dev)
    if mean.shape != x.shape or var.shape != x.shape or mean.device != dev or var.device != dev:
        raise ValueError("gmm_trajectory_stats: mean and var must have x's shape and device")
    lds = [_pf_row_stride(t, B, T, D, "gmm_trajectory_stats") for t in (x, mean, var)]
    rc = lib().mlpg_hip_gmm_trajectory_stats(dev.index, _stream(dev), _p(x), lds[0], _p(lengths), B, T, D, _p(labels), _p(mu_x),
                                             _p(mu_y), _p(A), _p(cvar), M, _p(mean), lds[1], _p(var), lds[2])
    _check(rc, "mlpg_hip_gmm_trajectory_stats")
    return mean, var


def gv_max_frames():
    """mlpg_hip_gv_max_frames(): the longest padded utterance (Tmax) mlpg_hip_gv_ascent takes."""
    return lib().mlpg_hip_gv_max_frames()


GV_INIT = {"given": 0, "scaled": 1}


def gv_ascent(mean, var, windows, y, gv_mean, gv_prec, lengths=None, n_iter=100, step=None, init="scaled", omega_scale=1.0, out=None):
    """mlpg_hip_gv_ascent on CUDA tensors: mean (B, Tmax, D) float32 / float64 contiguous, var the same shape, (D,) or None, y
    (B, Tmax, D // num_windows) of mean's dtype: the maximum-likelihood trajectory of (mean, var).  gv_mean, gv_prec: float64
    (D // num_windows) on the device.  Runs n_iter steps of steepest ascent on the likelihood with the gv term from the start
    ``init`` ("scaled" or "given"); step None or <= 0: the step the kernel derives per system.  The result goes to ``out``
    (default: ``y`` itself, in place).  Returns (out, report float64 (B, sd, 4): L(start), L(final), v(y), v(final); status int32
    (B, sd): 0 fine, 1 non-finite, 2 no ascent), all on the device, enqueued on the current stream.  One launch."""
    torch = torch_mod()
    assert mean.is_cuda and mean.dim() == 3 and mean.is_contiguous()
    B, T, D = mean.shape
    nw, pl, pu, pc, _keep = _win_args(windows)
    mode = _var_mode(var, mean, mean.shape, D)
    _check_lengths(lengths, B, mean.device)
    sd = D // nw if nw else 0
    if init not in GV_INIT:
        raise ValueError("gv_ascent: init must be 'scaled' or 'given', got %r" % (init,))
    if out is None:
        out = y
    for name, t in (("y", y), ("out", out)):
        if not (t.is_cuda and t.device == mean.device and t.dtype == mean.dtype and tuple(t.shape) == (B, T, sd) and t.is_contiguous()):
            raise ValueError("gv_ascent: %s must be a contiguous (%d, %d, %d) %s tensor on %s" % (name, B, T, sd, mean.dtype, mean.device))
    for name, t in (("gv_mean", gv_mean), ("gv_prec", gv_prec)):
        if not (t.is_cuda and t.device == mean.device and t.dtype == torch.float64 and tuple(t.shape) == (sd,) and t.is_contiguous()):
            raise ValueError("gv_ascent: %s must be a float64 (%d,) tensor on %s" % (name, sd, mean.device))
    report = torch.empty((B, sd, 4), dtype=torch.float64, device=mean.device)
    status = torch.empty((B, sd), dtype=torch.int32, device=mean.device)
    rc = lib().mlpg_hip_gv_ascent(mean.device.index, _stream(mean.device), _dt(mean), _p(mean), _p(var), mode, _p(lengths), B, T, D, nw,
                                  pl, pu, pc, _p(y), _p(out), _p(gv_mean), _p(gv_prec), float(omega_scale), int(n_iter),
                                  -1.0 if step is None else float(step), GV_INIT[init], _p(report), _p(status))
    _check(rc, "mlpg_hip_gv_ascent")
    return out, report, status


def gv(x, lengths=None):
    """mlpg_hip_gv: the gv (variance over the live frames) of every (b, d) of a padded batch.  x: (B, Tmax, D) float32 / float64
    CUDA tensor whose last dimension is contiguous and whose first two are those of a dense (B, Tmax, ld) array (a column slice
    is fine); lengths: int32 (B,) on the device or None.  Returns float64 (B, D) on the device.  One launch."""
    torch = torch_mod()
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 3):
        raise ValueError("gv: x must be a (B, Tmax, D) CUDA tensor")
    B, T, D = x.shape
    _check_lengths(lengths, B, x.device)
    ld = _pf_row_stride(x, B, T, D, "gv")
    out = torch.empty((B, D), dtype=torch.float64, device=x.device)
    rc = lib().mlpg_hip_gv(x.device.index, _stream(x.device), _dt(x), _p(x), ld, _p(lengths), B, T, D, _p(out))
    _check(rc, "mlpg_hip_gv")
    return out


COLSTATS_CHUNK_ROWS = 16        # MLPG_HIP_COLSTATS_CHUNK_ROWS: frames a lane of mlpg_hip_column_stats holds in registers
COLSTATS_BLOCK_ROWS = 512       # MLPG_HIP_COLSTATS_BLOCK_ROWS: frames of one utterance per workgroup


def column_stats_workspace(B, Tmax, D):
    """mlpg_hip_column_stats_workspace: the bytes of workspace a (B, Tmax, D) batch needs (host code)."""
    n = int(lib().mlpg_hip_column_stats_workspace(int(B), int(Tmax), int(D)))
    if n < 0:
        raise ValueError("column_stats: a (%d, %d, %d) batch is too large for one call" % (B, Tmax, D))
    return n


def column_stats(x, lengths=None, state_in=None, state_out=None, workspace=None):
    """mlpg_hip_column_stats on CUDA tensors: x (B, Tmax, D) float32 / float64 whose last dimension is contiguous and whose first
    two are those of a dense (B, Tmax, ld) array (a column slice of one is fine); lengths int32 (B) or None; state_in float64
    (5, D) -- rows count, mean, M2, min, max -- or None (empty); state_out the same (None: a new tensor; state_in itself: in
    place); workspace: a uint8 / float64 tensor of at least column_stats_workspace(B, Tmax, D) bytes (None: allocated).  Returns
    state_out.  Two launches on the current stream, no synchronisation."""
    torch = torch_mod()
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 3):
        raise ValueError("column_stats: x must be a (B, Tmax, D) CUDA tensor")
    B, T, D = x.shape
    dev = x.device
    _check_lengths(lengths, B, dev)
    ld = _pf_row_stride(x, B, T, D, "column_stats")
    for name, t in (("state_in", state_in), ("state_out", state_out)):
        if t is not None and not (torch.is_tensor(t) and t.device == dev and t.dtype == torch.float64 and tuple(t.shape) == (5, D)
                                  and t.is_contiguous()):
            raise ValueError("column_stats: %s must be a contiguous float64 (5, %d) tensor on %s" % (name, D, dev))
    if state_out is None:
        state_out = torch.empty((5, D), dtype=torch.float64, device=dev)
    need = column_stats_workspace(B, T, D)
    if workspace is None:
        workspace = torch.empty((need // 8,), dtype=torch.float64, device=dev)
    have = workspace.numel() * workspace.element_size()
    rc = lib().mlpg_hip_column_stats(dev.index, _stream(dev), _dt(x), _p(x), ld, _p(lengths), B, T, D, _p(state_in), _p(state_out),
                                     _p(workspace), have)
    _check(rc, "mlpg_hip_column_stats")
    return state_out


def column_affine(x, a, c, mode, lengths=None, out=None, out_dtype=None):
    """mlpg_hip_column_affine on CUDA tensors: mode 0  (x - c) / a,  mode 1  a x + c  per column, float64 arithmetic.  x
    (B, Tmax, D) float32 / float64, a column slice of a dense (B, Tmax, ld) tensor or dense itself; a, c float64 (D) on the
    device; out like x in shape, float32 / float64 (None: a new dense tensor of out_dtype, default x's; x itself: in place).
    Rows past an utterance's length come out as zeros.  One launch on the current stream."""
    torch = torch_mod()
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 3):
        raise ValueError("column_affine: x must be a (B, Tmax, D) CUDA tensor")
    B, T, D = x.shape
    dev = x.device
    if out is None:
        out = torch.empty((B, T, D), dtype=out_dtype or x.dtype, device=dev)
    if not (torch.is_tensor(out) and out.device == dev and out.shape == x.shape):
        raise ValueError("column_affine: out must have x's shape and device")
    for name, t in (("a", a), ("c", c)):
        if not (torch.is_tensor(t) and t.device == dev and t.dtype == torch.float64 and tuple(t.shape) == (D,) and t.is_contiguous()):
            raise ValueError("column_affine: %s must be a contiguous float64 (%d,) tensor on %s" % (name, D, dev))
    _check_lengths(lengths, B, dev)
    ld_x, ld_y = _pf_row_stride(x, B, T, D, "column_affine"), _pf_row_stride(out, B, T, D, "column_affine")
    rc = lib().mlpg_hip_column_affine(dev.index, _stream(dev), _dt(x), _dt(out), int(mode), _p(x), ld_x, _p(out), ld_y, _p(lengths),
                                      B, T, D, _p(a), _p(c))
    _check(rc, "mlpg_hip_column_affine")
    return out


def raise_on_status(status, sd):
    """Raise the reference's LinAlgError for the first failing (utterance, dim) system."""
    st = status.cpu().numpy().ravel()
    bad = np.flatnonzero(st)
    if bad.size:
        k = int(st[bad[0]])
        # scipy.linalg.LinAlgError is numpy.linalg.LinAlgError (linalg.pyx:79-82)
        raise np.linalg.LinAlgError("%d-th leading minor not positive definite" % k)
