"""ctypes binding of include/nnmnkwii_joint.h: the joint feature rows of one or two padded batches -- deltas computed on the
way, zero frames and padding removed, the kept rows dense (csrc/joint_rows.hip).  The entry points live in
libmlpg_hip.so beside the ``mlpg_hip_*`` ones, with their own prefix and version: they are bound here, on the handle
``_hip.lib()`` returns, and are no part of ``_hip.EXPORTS`` / ``_hip.ABI_VERSION``."""
import ctypes
import threading

import numpy as np

from . import _hip
from ._hip import HipExtensionError

ABI_VERSION = 1
F32, F64 = 0, 1
NONZERO, LIVE = 0, 1
TILE = 64                           # NNMK_JOINT_TILE: frames of one utterance per workgroup
MAX_WINDOWS, MAX_EXTENT = 8, 8
NAMES = ("nnmk_joint_abi_version", "nnmk_joint_workspace_bytes", "nnmk_joint_count", "nnmk_joint_write", "nnmk_joint_launch_count")

_bound = None
_lock = threading.Lock()


def lib():
    """The library handle with the nnmk_joint_* symbols bound (once).  HipExtensionError: not built, or another version."""
    global _bound
    if _bound is not None:
        return _bound
    L = _hip.lib()
    with _lock:
        if _bound is None:
            ci, vp, i64, dbl = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
            src = [ci, vp, i64, vp, ci, ci, vp, i64, vp, ci, ci, ci, ci, vp, vp, vp]    # dtype_x .. win_coef
            try:
                L.nnmk_joint_abi_version.restype = ci
                L.nnmk_joint_abi_version.argtypes = []
                L.nnmk_joint_workspace_bytes.restype = i64
                L.nnmk_joint_workspace_bytes.argtypes = [ci, ci]
                L.nnmk_joint_count.restype = ci
                L.nnmk_joint_count.argtypes = [ci, vp] + src + [ci, dbl, ci, vp, i64, vp]
                L.nnmk_joint_write.restype = ci
                L.nnmk_joint_write.argtypes = [ci, vp] + src + [vp, i64, ci, vp, i64, i64]
                L.nnmk_joint_launch_count.restype = ctypes.c_longlong
                L.nnmk_joint_launch_count.argtypes = []
            except AttributeError as e:
                raise HipExtensionError("nnmnkwii_amd: %s has no nnmk_joint_* entry points (%s) -- rebuild it with "
                                        "`python nnmnkwii_amd/csrc/build.py`" % (_hip.SO_PATH, e))
            if L.nnmk_joint_abi_version() != ABI_VERSION:
                raise HipExtensionError("nnmnkwii_amd: %s has joint ABI version %d, this binding needs %d"
                                        % (_hip.SO_PATH, L.nnmk_joint_abi_version(), ABI_VERSION))
            _bound = L
    return _bound


def pack_windows(wins):
    """(l, u, coef) triples -> (num_windows, int32 l[], int32 u[], float64 coef[]) host arrays; ValueError past the limits."""
    if len(wins) > MAX_WINDOWS:
        raise ValueError("joint: at most %d windows, got %d" % (MAX_WINDOWS, len(wins)))
    for l, u, c in wins:
        if not (0 <= l <= MAX_EXTENT and 0 <= u <= MAX_EXTENT and len(c) == l + u + 1):
            raise ValueError("joint: a window needs 0 <= l, u <= %d and l + u + 1 coefficients, got l = %d, u = %d, %d coefficients"
                             % (MAX_EXTENT, l, u, len(c)))
    wl = np.array([w[0] for w in wins], dtype=np.int32)
    wu = np.array([w[1] for w in wins], dtype=np.int32)
    wc = np.ascontiguousarray(np.concatenate([np.asarray(w[2], dtype=np.float64).ravel() for w in wins])) if wins else np.zeros(0)
    return len(wins), wl, wu, wc


def workspace(B, Tmax, device):
    """A fresh uint8 tensor of nnmk_joint_workspace_bytes(B, Tmax) bytes on `device`."""
    n = int(lib().nnmk_joint_workspace_bytes(int(B), int(Tmax)))
    if n < 0:
        raise ValueError("joint: negative size (B = %d, Tmax = %d)" % (B, Tmax))
    return _hip.torch_mod().empty((n,), dtype=_hip.torch_mod().uint8, device=device)


def check_source(name, t, B=None, Tmax=None, dev=None):
    """A (B, Tmax, D) float32 / float64 CUDA tensor whose last dimension is contiguous: its row stride.  ValueError otherwise."""
    torch = _hip.torch_mod()
    if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 3 and t.dtype in (torch.float32, torch.float64)
            and (B is None or (t.shape[0], t.shape[1]) == (B, Tmax)) and (dev is None or t.device == dev)):
        raise ValueError("joint: %s must be a float32 / float64 CUDA tensor of shape (B, Tmax, D)%s"
                         % (name, "" if B is None else " with x's B and Tmax, on x's device"))
    try:
        return _hip._pf_row_stride(t, t.shape[0], t.shape[1], t.shape[2], "joint") if t.shape[2] else 0
    except HipExtensionError as e:
        raise ValueError(str(e))


class Plan(object):
    """The arguments both stages share, checked once: sources, lengths, windows, the output's dtype, the workspace."""

    def __init__(self, x, y, len_x, len_y, wins, out_dtype, ws=None):
        torch = _hip.torch_mod()
        self.ld_x = check_source("x", x)
        self.B, self.Tmax, self.Dx = x.shape
        self.dev = x.device
        self.ld_y = check_source("y", y, self.B, self.Tmax, self.dev) if y is not None else 0
        self.Dy = y.shape[2] if y is not None else 0
        for name, n in (("len_x", len_x), ("len_y", len_y)):
            if n is not None and not (torch.is_tensor(n) and n.dtype == torch.int32 and tuple(n.shape) == (self.B,) and n.device == self.dev
                                      and n.is_contiguous()):
                raise ValueError("joint: %s must be an int32 (B) tensor on x's device" % name)
        if out_dtype not in (torch.float32, torch.float64):
            raise ValueError("joint: the output's dtype must be float32 or float64, got %s" % (out_dtype,))
        self.x, self.y, self.len_x, self.len_y, self.out_dtype = x, y, len_x, len_y, out_dtype
        self.nw, self.wl, self.wu, self.wc = pack_windows(wins)
        self.W = (self.Dx + self.Dy) * max(self.nw, 1)
        self.ws = workspace(self.B, self.Tmax, self.dev) if ws is None else ws
        if not (torch.is_tensor(self.ws) and self.ws.dtype == torch.uint8 and self.ws.device == self.dev and self.ws.is_contiguous()):
            raise ValueError("joint: the workspace must be a contiguous uint8 tensor on x's device")

    def _src(self):
        x, y = self.x, self.y
        return (_hip._dt(x), _hip._p(x), self.ld_x, _hip._p(self.len_x), self.Dx, _hip._dt(y) if y is not None else F32, _hip._p(y), self.ld_y,
                _hip._p(self.len_y), self.Dy, self.B, self.Tmax, self.nw, self.wl.ctypes.data, self.wu.ctypes.data, self.wc.ctypes.data)

    def count(self, keep, eps, offsets=None):
        """nnmk_joint_count on the current stream, no synchronisation: the device int64 (B + 1) offsets, offsets[B] = N."""
        torch = _hip.torch_mod()
        if keep not in (NONZERO, LIVE):
            raise ValueError("joint: unknown keep mode %r" % (keep,))
        if not float(eps) >= 0.0:
            raise ValueError("joint: eps must be >= 0, got %r" % (eps,))
        if offsets is None:
            offsets = torch.empty((self.B + 1,), dtype=torch.int64, device=self.dev)
        elif not (torch.is_tensor(offsets) and offsets.dtype == torch.int64 and tuple(offsets.shape) == (self.B + 1,)
                  and offsets.device == self.dev and offsets.is_contiguous()):
            raise ValueError("joint: offsets must be an int64 (B + 1) tensor on x's device")
        rc = lib().nnmk_joint_count(self.dev.index, _hip._stream(self.dev), *self._src(), int(keep), float(eps), F64 if self.out_dtype == torch.float64 else F32,
                                    _hip._p(self.ws), self.ws.numel(), _hip._p(offsets))
        _hip._check(rc, "nnmk_joint_count")
        return offsets

    def write(self, out):
        """nnmk_joint_write on the current stream, no synchronisation: the first min(N, len(out)) kept rows into out (cap, >= W)."""
        torch = _hip.torch_mod()
        if not (torch.is_tensor(out) and out.is_cuda and out.device == self.dev and out.dim() == 2 and out.dtype == self.out_dtype
                and out.shape[1] == self.W and (out.shape[1] <= 1 or out.stride(1) == 1) and (out.shape[0] <= 1 or out.stride(0) >= self.W)):
            raise ValueError("joint: out must be a (cap, %d) %s CUDA tensor on x's device with contiguous rows" % (self.W, self.out_dtype))
        cap = out.shape[0]
        ld = out.stride(0) if cap > 1 else self.W
        rc = lib().nnmk_joint_write(self.dev.index, _hip._stream(self.dev), *self._src(), _hip._p(self.ws), self.ws.numel(),
                                    F64 if self.out_dtype == torch.float64 else F32, _hip._p(out) if cap * self.W else None, ld, cap)
        _hip._check(rc, "nnmk_joint_write")
        return out


def count(x, y, len_x, len_y, wins, keep, eps, out_dtype, ws=None, offsets=None):
    """(plan, offsets): the first two stages (see Plan.count); plan.write(out) is the third."""
    plan = Plan(x, y, len_x, len_y, wins, out_dtype, ws)
    return plan, plan.count(keep, eps, offsets)


def write(plan, out):
    return plan.write(out)
