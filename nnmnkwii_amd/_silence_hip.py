"""ctypes binding of include/nnmnkwii_silence.h: silence frames dropped over padded batches -- the kept-frame expansion and the
row gather (csrc/frame_keep.hip).  The five entry points live in libmlpg_hip.so beside the ``mlpg_hip_*`` ones,
with their own prefix and version: they are bound here, on the handle ``_hip.lib()`` returns, and are no part of
``_hip.EXPORTS`` / ``_hip.ABI_VERSION``.  The dtype and kind codes are those of ``_frontend_hip``."""
import ctypes
import threading

from . import _frontend_hip as FH
from . import _hip
from ._hip import HipExtensionError

ABI_VERSION = 1
BLOCK_ROWS = 64                     # NNMK_SIL_BLOCK_ROWS: output rows of one utterance per workgroup
NAMES = ("nnmk_sil_abi_version", "nnmk_sil_frame_counts", "nnmk_sil_expand", "nnmk_sil_gather", "nnmk_sil_launch_count")

_bound = None
_lock = threading.Lock()


def lib():
    """The library handle with the nnmk_sil_* symbols bound (once).  HipExtensionError: not built, or another version."""
    global _bound
    if _bound is not None:
        return _bound
    L = _hip.lib()
    with _lock:
        if _bound is None:
            ci, vp, i64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
            try:
                L.nnmk_sil_abi_version.restype = ci
                L.nnmk_sil_abi_version.argtypes = []
                L.nnmk_sil_frame_counts.restype = ci
                L.nnmk_sil_frame_counts.argtypes = [ci, vp, ci, vp, vp, vp, ci, ci, ci, ci, vp]
                L.nnmk_sil_expand.restype = ci
                L.nnmk_sil_expand.argtypes = [ci, vp, ci, vp, i64, ci, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, ci, vp, i64, ci, vp]
                L.nnmk_sil_gather.restype = ci
                L.nnmk_sil_gather.argtypes = [ci, vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, vp, i64, vp, ci, ci, ci, vp, i64, ci, vp]
                L.nnmk_sil_launch_count.restype = ctypes.c_longlong
                L.nnmk_sil_launch_count.argtypes = []
            except AttributeError as e:
                raise HipExtensionError("nnmnkwii_amd: %s has no nnmk_sil_* entry points (%s) -- rebuild it with "
                                        "`python nnmnkwii_amd/csrc/build.py`" % (_hip.SO_PATH, e))
            if L.nnmk_sil_abi_version() != ABI_VERSION:
                raise HipExtensionError("nnmnkwii_amd: %s has silence ABI version %d, this binding needs %d"
                                        % (_hip.SO_PATH, L.nnmk_sil_abi_version(), ABI_VERSION))
            _bound = L
    return _bound


def _check_batch(durations, num_phones, silence):
    torch = _hip.torch_mod()
    B, Nmax, S = FH._check_batch(durations, num_phones, "silence")
    if not (torch.is_tensor(silence) and silence.dtype in (torch.bool, torch.uint8) and tuple(silence.shape) == (B, Nmax)
            and silence.device == durations.device and silence.is_contiguous()):
        raise ValueError("silence: the flags must be a contiguous bool / uint8 (B, Nmax) tensor on the durations' device")
    return B, Nmax, S


def frame_counts(durations, num_phones, silence, min_frames=0):
    """nnmk_sil_frame_counts on CUDA tensors: durations (B, Nmax, S) int32 / int64 / float32 / float64, contiguous; num_phones
    int32 (B) or None; silence bool / uint8 (B, Nmax).  Returns int64 (B, 2) on the device: the kept frames K_b and all frames
    T_b of every utterance.  One launch, no synchronisation."""
    B, Nmax, S = _check_batch(durations, num_phones, silence)
    dt = FH._dur_dtype(durations)
    mf = FH._min_frames("silence", min_frames)
    torch = _hip.torch_mod()
    L = lib()
    dev = durations.device
    counts = torch.empty((B, 2), dtype=torch.int64, device=dev)
    rc = L.nnmk_sil_frame_counts(dev.index, _hip._stream(dev), dt, _hip._p(durations), _hip._p(num_phones), _hip._p(silence), B, Nmax, S, mf,
                                 _hip._p(counts))
    _hip._check(rc, "nnmk_sil_frame_counts")
    return counts


def expand(phone, durations, num_phones, silence, kind, min_frames, cc, scale_, min_, out, lengths_out=None):
    """nnmk_sil_expand on CUDA tensors: ``_frontend_hip.expand`` with the flags silence (B, Nmax) bool / uint8; out
    (B, Tcap, Dl + F).  Returns lengths int32 (B) = min(K_b, Tcap).  One launch on the current stream, no synchronisation."""
    torch = _hip.torch_mod()
    B, Nmax, S = _check_batch(durations, num_phones, silence)
    dt = FH._dur_dtype(durations)
    dev = durations.device
    Dl, W, Tcap, mf = FH._check_expand("silence", "Tcap", B, Nmax, dev, phone=phone, kind=kind, min_frames=min_frames, cc=cc, scale_=scale_,
                                       min_=min_, out=out)
    L = lib()
    ld_p = _hip._pf_row_stride(phone, B, Nmax, Dl, "silence") if Dl else 0
    ld_out = _hip._pf_row_stride(out, B, Tcap, W, "silence") if W else 0
    if lengths_out is None:
        lengths_out = torch.empty((B,), dtype=torch.int32, device=dev)
    rc = L.nnmk_sil_expand(dev.index, _hip._stream(dev), _hip._dt(phone), _hip._p(phone), ld_p, dt, _hip._p(durations), _hip._p(num_phones),
                           _hip._p(silence), B, Nmax, S, Dl, mf, int(kind), _hip._p(cc) if kind == FH.COARSE_CODING else None, _hip._p(scale_),
                           _hip._p(min_), _hip._dt(out), _hip._p(out), ld_out, Tcap, _hip._p(lengths_out))
    _hip._check(rc, "nnmk_sil_expand")
    return lengths_out


def gather(src, len_src, durations, num_phones, silence, min_frames, out, lengths_out=None):
    """nnmk_sil_gather on CUDA tensors.  src: (B, Tmax, D) float32 / float64 whose last dimension is contiguous and whose first
    two are those of a dense (B, Tmax, ld) array; len_src int32 (B) or None; out: (B, Tcap, D) float32 / float64, a column slice
    of a dense (B, Tcap, ld) tensor is fine, not src itself.  Returns lengths int32 (B).  One launch on the current stream, no
    synchronisation."""
    torch = _hip.torch_mod()
    B, Nmax, S = _check_batch(durations, num_phones, silence)
    dt = FH._dur_dtype(durations)
    dev = durations.device
    if not (torch.is_tensor(src) and src.dim() == 3 and src.shape[0] == B and src.device == dev and src.dtype in (torch.float32, torch.float64)):
        raise ValueError("silence: the source must be a float32 / float64 (B, Tmax, D) tensor on the durations' device")
    Tmax, D = src.shape[1:]
    if not (torch.is_tensor(out) and out.dim() == 3 and out.shape[0] == B and out.shape[2] == D and out.device == dev
            and out.dtype in (torch.float32, torch.float64)):
        raise ValueError("silence: out must be a float32 / float64 (B, Tcap, %d) tensor on the durations' device" % D)
    Tcap = out.shape[1]
    if len_src is not None and not (torch.is_tensor(len_src) and len_src.dtype == torch.int32 and tuple(len_src.shape) == (B,)
                                    and len_src.device == dev and len_src.is_contiguous()):
        raise ValueError("silence: the source's lengths must be an int32 (B) tensor on the durations' device")
    if B * Tcap * D and out.data_ptr() == src.data_ptr():
        raise ValueError("silence: out must not be the source (rows move across workgroups)")
    mf = FH._min_frames("silence", min_frames)
    L = lib()
    ld_src = _hip._pf_row_stride(src, B, Tmax, D, "silence") if D else 0
    ld_out = _hip._pf_row_stride(out, B, Tcap, D, "silence") if D else 0
    if lengths_out is None:
        lengths_out = torch.empty((B,), dtype=torch.int32, device=dev)
    rc = L.nnmk_sil_gather(dev.index, _hip._stream(dev), dt, _hip._p(durations), _hip._p(num_phones), _hip._p(silence), B, Nmax, S, mf,
                           _hip._dt(src), _hip._p(src), ld_src, _hip._p(len_src), Tmax, D, _hip._dt(out), _hip._p(out), ld_out, Tcap,
                           _hip._p(lengths_out))
    _hip._check(rc, "nnmk_sil_gather")
    return lengths_out
