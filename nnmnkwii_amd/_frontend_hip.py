"""ctypes binding of include/nnmnkwii_frontend.h: phone-level linguistic features expanded to frames over padded batches
(csrc/frame_expand.hip).  The five entry points live in libmlpg_hip.so beside the ``mlpg_hip_*`` ones, with their
own prefix and version: they are bound here, on the handle ``_hip.lib()`` returns, and are no part of ``_hip.EXPORTS`` /
``_hip.ABI_VERSION``."""
import ctypes
import threading

from . import _hip
from ._hip import HipExtensionError

ABI_VERSION = 1
F32, F64, I32, I64 = 0, 1, 2, 3
KINDS = (None, "full", "minimal_frame", "state_only", "frame_only", "uniform_state", "coarse_coding", "minimal_phoneme")
NONE, FULL, MINIMAL_FRAME, STATE_ONLY, FRAME_ONLY, UNIFORM_STATE, COARSE_CODING, MINIMAL_PHONEME = range(8)
SIZES = (0, 9, 2, 1, 1, 2, 4, 3)    # nnmk_frontend_feature_size
MAX_S = 8                           # NNMK_FRONTEND_MAX_S
CC_POINTS = 600                     # NNMK_FRONTEND_CC_POINTS
BLOCK_ROWS = 64                     # NNMK_FRONTEND_BLOCK_ROWS: frames of one utterance per workgroup
MAX_STATES = 8192                   # NNMK_FRONTEND_MAX_STATES: Nmax * S at most
NAMES = ("nnmk_frontend_abi_version", "nnmk_frontend_feature_size", "nnmk_frontend_frame_counts", "nnmk_frontend_expand",
         "nnmk_frontend_launch_count")

_bound = None
_lock = threading.Lock()


def lib():
    """The library handle with the nnmk_frontend_* symbols bound (once).  HipExtensionError: not built, or another version."""
    global _bound
    if _bound is not None:
        return _bound
    L = _hip.lib()
    with _lock:
        if _bound is None:
            ci, vp, i64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
            try:
                L.nnmk_frontend_abi_version.restype = ci
                L.nnmk_frontend_abi_version.argtypes = []
                L.nnmk_frontend_feature_size.restype = ci
                L.nnmk_frontend_feature_size.argtypes = [ci]
                L.nnmk_frontend_frame_counts.restype = ci
                L.nnmk_frontend_frame_counts.argtypes = [ci, vp, ci, vp, vp, ci, ci, ci, ci, vp]
                L.nnmk_frontend_expand.restype = ci
                L.nnmk_frontend_expand.argtypes = [ci, vp, ci, vp, i64, ci, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, ci, vp, i64, ci, vp]
                L.nnmk_frontend_launch_count.restype = ctypes.c_longlong
                L.nnmk_frontend_launch_count.argtypes = []
            except AttributeError as e:
                raise HipExtensionError("nnmnkwii_amd: %s has no nnmk_frontend_* entry points (%s) -- rebuild it with "
                                        "`python nnmnkwii_amd/csrc/build.py`" % (_hip.SO_PATH, e))
            if L.nnmk_frontend_abi_version() != ABI_VERSION:
                raise HipExtensionError("nnmnkwii_amd: %s has frontend ABI version %d, this binding needs %d"
                                        % (_hip.SO_PATH, L.nnmk_frontend_abi_version(), ABI_VERSION))
            _bound = L
    return _bound


def _dur_dtype(t):
    torch = _hip.torch_mod()
    try:
        return {torch.float32: F32, torch.float64: F64, torch.int32: I32, torch.int64: I64}[t.dtype]
    except KeyError:
        raise ValueError("frontend: durations must be int32, int64, float32 or float64, got %s" % t.dtype)


def _check_batch(durations, num_phones, who="frontend"):
    torch = _hip.torch_mod()
    if not (torch.is_tensor(durations) and durations.is_cuda and durations.dim() == 3 and durations.is_contiguous()):
        raise ValueError("%s: durations must be a contiguous (B, Nmax, S) CUDA tensor" % who)
    B, Nmax, S = durations.shape
    if not 1 <= S <= MAX_S:
        raise ValueError("%s: S must be in 1 .. %d, got %d" % (who, MAX_S, S))
    if Nmax * S > MAX_STATES:
        raise ValueError("%s: Nmax * S = %d states, at most %d fit" % (who, Nmax * S, MAX_STATES))
    if num_phones is not None and not (torch.is_tensor(num_phones) and num_phones.dtype == torch.int32 and tuple(num_phones.shape) == (B,)
                                       and num_phones.device == durations.device and num_phones.is_contiguous()):
        raise ValueError("%s: num_phones must be an int32 (B) tensor on the durations' device" % who)
    return B, Nmax, S


def _min_frames(who, min_frames):
    if int(min_frames) < 0:
        raise ValueError("%s: min_frames must be at least 0, got %d" % (who, min_frames))
    return int(min_frames)


def _check_expand(who, cap, B, Nmax, dev, *, phone, kind, min_frames, cc, scale_, min_, out):
    """The tensor checks that both expansions share (who: "frontend" / "silence", cap: what the caller calls out's rows, "Tmax" /
    "Tcap"); the tensors go in by keyword.  Returns Dl, the width Dl + F, out's rows and min_frames as an int."""
    torch = _hip.torch_mod()
    if not 0 <= int(kind) < len(SIZES):
        raise ValueError("%s: unknown kind %r" % (who, kind))
    F = SIZES[kind]
    if not (torch.is_tensor(phone) and phone.dim() == 3 and tuple(phone.shape[:2]) == (B, Nmax) and phone.device == dev
            and phone.dtype in (torch.float32, torch.float64)):
        raise ValueError("%s: phone features must be a float32 / float64 (B, Nmax, Dl) tensor on the durations' device" % who)
    Dl = phone.shape[2]
    W = Dl + F
    if not (torch.is_tensor(out) and out.dim() == 3 and out.shape[0] == B and out.shape[2] == W and out.device == dev
            and out.dtype in (torch.float32, torch.float64)):
        raise ValueError("%s: out must be a float32 / float64 (B, %s, %d) tensor on the durations' device" % (who, cap, W))
    for name, t in (("scale_", scale_), ("min_", min_)):
        if t is not None and not (torch.is_tensor(t) and t.dtype == torch.float64 and tuple(t.shape) == (W,) and t.device == dev and t.is_contiguous()):
            raise ValueError("%s: %s must be a float64 (%d) tensor on the durations' device" % (who, name, W))
    if (scale_ is None) != (min_ is None):
        raise ValueError("%s: scale_ and min_ go together" % who)
    if kind == COARSE_CODING and not (torch.is_tensor(cc) and cc.dtype == torch.float64 and tuple(cc.shape) == (3, CC_POINTS) and cc.device == dev
                                      and cc.is_contiguous()):
        raise ValueError("%s: the coarse-coding kind needs its float64 (3, %d) table on the durations' device" % (who, CC_POINTS))
    return Dl, W, out.shape[1], _min_frames(who, min_frames)


def frame_counts(durations, num_phones=None, min_frames=0):
    """nnmk_frontend_frame_counts on CUDA tensors: durations (B, Nmax, S) int32 / int64 / float32 / float64, contiguous; num_phones
    int32 (B) or None.  Returns the frames of every utterance, int64 (B) on the device.  One launch, no synchronisation."""
    B, Nmax, S = _check_batch(durations, num_phones)
    dt = _dur_dtype(durations)
    mf = _min_frames("frontend", min_frames)
    torch = _hip.torch_mod()
    L = lib()
    dev = durations.device
    counts = torch.empty((B,), dtype=torch.int64, device=dev)
    rc = L.nnmk_frontend_frame_counts(dev.index, _hip._stream(dev), dt, _hip._p(durations), _hip._p(num_phones), B, Nmax, S, mf,
                                      _hip._p(counts))
    _hip._check(rc, "nnmk_frontend_frame_counts")
    return counts


def expand(phone, durations, num_phones, kind, min_frames, cc, scale_, min_, out, lengths_out=None):
    """nnmk_frontend_expand on CUDA tensors.  phone: (B, Nmax, Dl) float32 / float64 whose last dimension is contiguous and
    whose first two are those of a dense (B, Nmax, ld) array; durations (B, Nmax, S) contiguous; kind: 0 .. 7; cc: float64
    (3, 600) for the coarse-coding kind, else None; scale_, min_: float64 (Dl + F) or both None; out: (B, Tmax, Dl + F) float32 /
    float64, a column slice of a dense (B, Tmax, ld) tensor is fine.  Returns lengths int32 (B).  One launch on the current
    stream, no synchronisation."""
    torch = _hip.torch_mod()
    B, Nmax, S = _check_batch(durations, num_phones)
    dt = _dur_dtype(durations)
    dev = durations.device
    Dl, W, Tmax, mf = _check_expand("frontend", "Tmax", B, Nmax, dev, phone=phone, kind=kind, min_frames=min_frames, cc=cc, scale_=scale_,
                                    min_=min_, out=out)
    L = lib()
    ld_p = _hip._pf_row_stride(phone, B, Nmax, Dl, "frontend") if Dl else 0
    ld_out = _hip._pf_row_stride(out, B, Tmax, W, "frontend") if W else 0
    if lengths_out is None:
        lengths_out = torch.empty((B,), dtype=torch.int32, device=dev)
    rc = L.nnmk_frontend_expand(dev.index, _hip._stream(dev), _hip._dt(phone), _hip._p(phone), ld_p, dt, _hip._p(durations), _hip._p(num_phones),
                                B, Nmax, S, Dl, mf, int(kind), _hip._p(cc) if kind == COARSE_CODING else None, _hip._p(scale_),
                                _hip._p(min_), _hip._dt(out), _hip._p(out), ld_out, Tmax, _hip._p(lengths_out))
    _hip._check(rc, "nnmk_frontend_expand")
    return lengths_out
