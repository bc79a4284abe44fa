"""ctypes binding of include/nnmnkwii_metrics.h: the objective metrics over padded batches (csrc/frame_metrics.hip, DESIGN.md
K13).  The four entry points live in libmlpg_hip.so beside the ``mlpg_hip_*`` ones, with their own prefix and version: they are
bound here, on the handle ``_hip.lib()`` returns, and are no part of ``_hip.EXPORTS`` / ``_hip.ABI_VERSION``."""
import ctypes
import threading

from . import _hip
from ._hip import HipExtensionError

ABI_VERSION = 1
BLOCK_ROWS = 256                # NNMK_METRICS_BLOCK_ROWS: frames of one utterance per workgroup
MAX_TERMS = 8                   # NNMK_METRICS_MAX_TERMS
MAX_ROW_BYTES = 16000           # NNMK_METRICS_MAX_ROW_BYTES
FRAME_L2, SQUARED, VOICED_SQUARED, MISMATCH = 0, 1, 2, 3
FLAG_EXP = 1
NAMES = ("nnmk_metrics_abi_version", "nnmk_metrics_workspace", "nnmk_metrics_batch", "nnmk_metrics_launch_count")


class Term(ctypes.Structure):
    """nnmk_metrics_term"""
    _fields_ = [("kind", ctypes.c_int32), ("x_col", ctypes.c_int32), ("y_col", ctypes.c_int32), ("width", ctypes.c_int32),
                ("x_mask_col", ctypes.c_int32), ("y_mask_col", ctypes.c_int32), ("flags", ctypes.c_int32), ("threshold", ctypes.c_double)]


def term(kind, x_col, y_col=None, width=1, x_mask_col=0, y_mask_col=None, flags=0, threshold=None):
    """A Term; y_col and y_mask_col default to the x ones, threshold None is NaN (the reference's rules)."""
    return Term(int(kind), int(x_col), int(x_col if y_col is None else y_col), int(width), int(x_mask_col),
                int(x_mask_col if y_mask_col is None else y_mask_col), int(flags), float("nan") if threshold is None else float(threshold))


_bound = None
_lock = threading.Lock()


def lib():
    """The library handle with the nnmk_metrics_* symbols bound (once).  HipExtensionError: not built, or another version."""
    global _bound
    if _bound is not None:
        return _bound
    L = _hip.lib()
    with _lock:
        if _bound is None:
            ci, vp, i64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
            try:
                L.nnmk_metrics_abi_version.restype = ci
                L.nnmk_metrics_abi_version.argtypes = []
                L.nnmk_metrics_workspace.restype = i64
                L.nnmk_metrics_workspace.argtypes = [ci, ci, ci]
                L.nnmk_metrics_batch.restype = ci
                L.nnmk_metrics_batch.argtypes = [ci, vp, ci, vp, i64, ci, vp, i64, vp, ci, ci, ctypes.POINTER(Term), ci, vp, vp, vp, i64]
                L.nnmk_metrics_launch_count.restype = ctypes.c_longlong
                L.nnmk_metrics_launch_count.argtypes = []
            except AttributeError as e:
                raise HipExtensionError("nnmnkwii_amd: %s has no nnmk_metrics_* entry points (%s) -- rebuild it with "
                                        "`python nnmnkwii_amd/csrc/build.py`" % (_hip.SO_PATH, e))
            if L.nnmk_metrics_abi_version() != ABI_VERSION:
                raise HipExtensionError("nnmnkwii_amd: %s has metrics ABI version %d, this binding needs %d"
                                        % (_hip.SO_PATH, L.nnmk_metrics_abi_version(), ABI_VERSION))
            _bound = L
    return _bound


def metrics_workspace(B, Tmax, nterms):
    """nnmk_metrics_workspace: the bytes of workspace a (B, Tmax) batch with nterms terms needs (host code)."""
    n = int(lib().nnmk_metrics_workspace(int(B), int(Tmax), int(nterms)))
    if n < 0:
        raise ValueError("metrics: a (%d, %d) batch with %d terms is too large for one call" % (B, Tmax, nterms))
    return n


def metrics_batch(x, y, terms, lengths=None, per_utt=False, workspace=None):
    """nnmk_metrics_batch on CUDA tensors.  x, y: (B, Tmax, .) float32 / float64 (the dtypes may differ) whose last dimension is
    contiguous and whose first two are those of a dense (B, Tmax, ld) array (a column slice of one is fine); terms: a sequence of
    1 .. 8 Term whose columns count from the slices' first column; lengths int32 (B) on the device or None; workspace: a tensor
    of at least metrics_workspace(B, Tmax, len(terms)) bytes (None: allocated).  Returns (totals (nterms, 2), per_utt
    (B, nterms, 2) or None), float64 pairs (sum, count) on the device.  Two launches on the current stream, no synchronisation."""
    torch = _hip.torch_mod()
    for name, t in (("x", x), ("y", y)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 3):
            raise ValueError("metrics_batch: %s must be a (B, Tmax, D) CUDA tensor" % name)
    if x.shape[:2] != y.shape[:2] or x.device != y.device:
        raise ValueError("metrics_batch: x and y must agree in (B, Tmax) and device, got %s and %s" % (tuple(x.shape), tuple(y.shape)))
    terms = list(terms)
    if not 1 <= len(terms) <= MAX_TERMS or not all(isinstance(t, Term) for t in terms):
        raise ValueError("metrics_batch: terms must be 1 .. %d Term objects" % MAX_TERMS)
    for i, t in enumerate(terms):
        if t.width < 1 or t.x_col < 0 or t.y_col < 0 or t.x_col + t.width > x.shape[2] or t.y_col + t.width > y.shape[2]:
            raise ValueError("metrics_batch: term %d names columns outside x %s or y %s" % (i, tuple(x.shape), tuple(y.shape)))
        if t.kind == VOICED_SQUARED and not (0 <= t.x_mask_col < x.shape[2] and 0 <= t.y_mask_col < y.shape[2]):
            raise ValueError("metrics_batch: term %d names mask columns outside x %s or y %s" % (i, tuple(x.shape), tuple(y.shape)))
    L = lib()
    B, T = x.shape[:2]
    dev = x.device
    _hip._check_lengths(lengths, B, dev)
    ld_x = _hip._pf_row_stride(x, B, T, x.shape[2], "metrics_batch")
    ld_y = _hip._pf_row_stride(y, B, T, y.shape[2], "metrics_batch")
    n = len(terms)
    totals = torch.empty((n, 2), dtype=torch.float64, device=dev)
    per = torch.empty((B, n, 2), dtype=torch.float64, device=dev) if per_utt else None
    need = metrics_workspace(B, T, n)
    if workspace is None:
        workspace = torch.empty((need // 8,), dtype=torch.float64, device=dev)
    have = workspace.numel() * workspace.element_size()
    arr = (Term * n)(*terms)
    rc = L.nnmk_metrics_batch(dev.index, _hip._stream(dev), _hip._dt(x), _hip._p(x), ld_x, _hip._dt(y), _hip._p(y), ld_y, _hip._p(lengths),
                              B, T, arr, n, _hip._p(per), _hip._p(totals), _hip._p(workspace), have)
    _hip._check(rc, "nnmk_metrics_batch")
    return totals, per
