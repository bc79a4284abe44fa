"""DTW alignment of padded utterance batches on MI355X.

Host-side mirror of /root/reference/nnmnkwii/preprocessing/alignment.py:9-190.
The per-pair Python loop (trim -> fastdtw -> gather -> pad) of the reference
becomes three batched HIP launches over all pairs: trailing-zero trim,
multi-resolution fastdtw with an anti-diagonal DP, and a gather along the
warping paths (C ABI: include/mlpg_hip.h).  ``IterativeDTWAligner`` wraps the
same launches in the reference's align -> fit joint GMM -> convert loop.
"""
import numpy as np
from numpy.linalg import norm

from .. import _hip


def _default_dist(x, y):
    return norm(x - y)


# Widest frames the MLPG_HIP_DIST_SCALED_*_NP kinds take: numpy sums up to 128 contiguous float64 elements as eight partial sums
# and splits longer vectors recursively, which the kernel does not follow (launch_fastdtw refuses them, csrc/dtw_fast.hip)
_NP_MAX_DIMS = 128

_warned = set()


def _warn_once(key, msg):
    """One RuntimeWarning per process and kind: the host-cost route is correct but 1000x slower than the device-side costs,
    and falling onto it silently is how a typo in `dist` turns a millisecond into minutes."""
    if key not in _warned:
        _warned.add(key)
        import warnings
        warnings.warn(msg, RuntimeWarning, stacklevel=3)


def _resolve_dist(dist):
    """Map a ``dist`` callable onto a local cost the HIP kernel evaluates: (dist_kind, dist_scale).

    * the default (``norm(x - y)``) and any callable that IS the Euclidean distance -> MLPG_HIP_DIST_L2;
    * ``metrics.melcd`` (this package's or the reference's) and any callable that is a positive multiple of the
      Euclidean distance -> MLPG_HIP_DIST_SCALED_L2_NP (numpy summation order, the multiple as measured);
    * a positive multiple of the city-block distance ``np.abs(x - y).sum()`` (``norm(x - y, 1)``,
      ``scipy.spatial.distance.cityblock``) or of the squared Euclidean distance ``((x - y) ** 2).sum()``
      (``sqeuclidean``) -> MLPG_HIP_DIST_SCALED_L1_NP / MLPG_HIP_DIST_SCALED_SQL2_NP;
    * anything else: ``None`` -- the caller then evaluates the local costs on the host with the callable itself, one
      call per window cell as upstream fastdtw does, and runs the DP, the back-trace and the window expansion on the GPU
      (``_hip.fastdtw_callable``).
    The three ``_NP`` kinds follow numpy's summation order for frames of at most 128 dims only; on wider features
    ``DTWAligner._paths`` takes the host-evaluated route for them as well (the default Euclidean kind has no width limit).
    A recognised callable is only probed on a few random frame pairs, never called per DP cell.
    """
    from .. import metrics
    if dist is _default_dist:
        return _hip.DIST_L2, 1.0
    if dist is metrics.melcd:
        return _hip.DIST_SCALED_L2_NP, float(metrics._logdb_const)
    if not callable(dist):
        raise TypeError("dist must be callable")
    # candidate forms, each evaluated by the kernel in numpy's summation order: Euclidean, city-block, squared Euclidean
    forms = (
        (_hip.DIST_SCALED_L2_NP, lambda x, y: float(norm(x - y))),
        (_hip.DIST_SCALED_L1_NP, lambda x, y: float(np.abs(x - y).sum())),
        (_hip.DIST_SCALED_SQL2_NP, lambda x, y: float(((x - y) ** 2).sum())),
    )
    rng = np.random.RandomState(12345)
    probes = [(rng.randn(D), rng.randn(D)) for D in (1, 5, 25) for _ in range(3)]
    try:
        vals = np.asarray([float(dist(x, y)) for x, y in probes])
    except Exception as e:   # a callable that does not like the probes: it is simply called per cell
        _warn_once("probe", "DTWAligner: `dist` raised %s on the probe frames; it will be called once per window cell on the "
                            "host (reference speed) instead of being evaluated on the GPU" % type(e).__name__)
        return None
    for kind, form in forms:
        ratios = vals / np.asarray([form(x, y) for x, y in probes])
        c = float(np.median(ratios))
        if c > 0 and np.all(np.abs(ratios - c) <= 1e-9 * c):
            if kind == _hip.DIST_SCALED_L2_NP and abs(c - 1.0) <= 1e-12:
                return _hip.DIST_L2, 1.0
            return kind, c
    return None


class DTWAligner(object):
    """Align feature matrices with fastdtw (radius-limited multi-resolution DTW).

    Same constructor and ``transform`` contract as the reference class: inputs
    are zero-padded ``(N, Tx, D)`` / ``(N, Ty, D)`` arrays; outputs are two
    ``(N, max(T_longer, longest path), D)`` arrays with the dtype of the longer
    input.  ``dist``: where the callable is one the HIP kernel can evaluate
    itself (:func:`_resolve_dist`: the default Euclidean ``norm(x - y)``,
    ``metrics.melcd`` -- the reference's own test passes it --, positive
    multiples of the Euclidean, city-block or squared Euclidean distance) the
    whole alignment runs on the GPU; ANY other callable is evaluated on the
    host, once per window cell as upstream fastdtw does, and only the DP,
    back-trace and window expansion run on the GPU (reference speed: the
    interpreter call per cell is the cost, as it is in the reference).  A
    recognised non-default ``dist`` on features wider than 128 dims takes that
    host-evaluated route too, with one ``RuntimeWarning``: the kernel follows
    numpy's summation order of those distances up to 128 elements only.  The
    default distance runs on the GPU at any width.

    ``tie_rule`` (an extension, keyword only): which of equal DP candidates
    wins -- ``"first"`` (upstream's pure-Python recurrence: first minimum of
    up, left, diagonal; the rule all parity tests are pinned on) or
    ``"diag_last"`` (the strict-less chain recalled for upstream's compiled
    extension; UNVERIFIED, see include/mlpg_hip.h).  Continuous data never tie.
    ``devices`` (extension, keyword only): a list of GPU indices or ``"all"``
    -- the pairs are dealt in chunks over those devices from this one process
    (mlpg_hip_fastdtw_host_multi); default: the process's current GPU.

    ``transform`` on two CUDA tensors (float32 / float64, one device) stays on
    the device: it returns two CUDA tensors of the longer input's dtype with the
    shape the numpy route gives, after one read-back of two integers (the
    shortest and the longest path).  A ``dist`` that would have to be evaluated
    on the host, and ``devices=``, raise ``ValueError`` there.
    ``path_lengths_`` holds the aligned lengths after every call: a device int32
    ``(N)`` tensor for tensors, a numpy array for numpy inputs.

    Attributes:
        dist (function): Distance function (default L2).
        radius (int): fastdtw radius.
        verbose (int): Verbose flag.
    """

    def __init__(self, dist=_default_dist, radius=1, verbose=0, *, tie_rule="first", devices=None):
        self.verbose = verbose
        self.dist = dist
        self.radius = radius
        assert tie_rule in ("first", "diag_last")
        self.tie_rule = tie_rule
        self.devices = devices     # None: the current GPU; a list of GPU indices or "all": pairs dealt over them

    # Batches below this many input bytes go through device tensors (upload once, trim + fastdtw + gather on the GPU,
    # download the aligned arrays: 4-6 ms for 128 config-4 pairs); larger ones through the host-pointer entry point
    # (chunked, transfers overlapped with the kernels) with the aligned arrays assembled on the host.
    _HOST_ENTRY_BYTES = 64 << 20
    # ... and a call on very few pairs (the reference's literal per-pair use): one C call and row copies on the host instead of two
    # uploads, five launches and eight downloads through the framework (one pair: 0.50 -> 0.39 ms, profiles/r06_notes.md section 17)
    _HOST_ENTRY_PAIRS = 2

    def _paths(self, X, Y):
        """Trim + fastdtw of every pair.  Returns numpy (path_i, path_j, path_len, cost, lenx, leny) and a gather
        function ``(src_is_x, path, plen, T_out, dtype) -> aligned array``."""
        resolved = _resolve_dist(self.dist)
        tie = _hip.TIE_FIRST_MIN if getattr(self, "tie_rule", "first") == "first" else _hip.TIE_DIAG_LAST
        dev = _hip.require_gpu()
        if resolved is None:
            _warn_once("callable", "DTWAligner: `dist` is none of the distances the kernel evaluates itself (Euclidean, city-block, "
                                   "squared Euclidean, or a positive multiple such as metrics.melcd): the local costs are evaluated "
                                   "on the host, one Python call per window cell, as upstream fastdtw does")
            if getattr(self, "devices", None) is not None:
                _warn_once("devices", "DTWAligner: `devices` is ignored for a host-evaluated `dist` (the DP runs on the current GPU)")
            if self.verbose > 0:
                print("DTWAligner: host-evaluated local costs (dist = %r)" % (self.dist,))
            return self._paths_callable(X, Y, tie, dev)
        dist_kind, dist_scale = resolved
        if dist_kind != _hip.DIST_L2 and X.shape[2] > _NP_MAX_DIMS:
            # before the route split: device tensors, the host-pointer entry and `devices` all end in the same kernel
            _warn_once("wide", "DTWAligner: the kernel reproduces numpy's summation order of this `dist` for at most %d feature "
                               "dims (got %d): the local costs are evaluated on the host, one Python call per window cell, as "
                               "upstream fastdtw does" % (_NP_MAX_DIMS, X.shape[2]))
            if getattr(self, "devices", None) is not None:
                _warn_once("devices", "DTWAligner: `devices` is ignored for a host-evaluated `dist` (the DP runs on the current GPU)")
            if self.verbose > 0:
                print("DTWAligner: host-evaluated local costs (dist = %r, %d dims)" % (self.dist, X.shape[2]))
            return self._paths_callable(X, Y, tie, dev)
        devices = getattr(self, "devices", None)
        if devices is not None or X.nbytes + Y.nbytes >= self._HOST_ENTRY_BYTES or X.shape[0] <= self._HOST_ENTRY_PAIRS:
            out = _hip.fastdtw_host(X, Y, self.radius, dist_kind, dist_scale, tie_rule=tie,
                                    device=dev.index if devices is None else devices)   # alignment.py:46-50
            return out + ((lambda is_x, path, plen, T_out, dtype: _gather(X if is_x else Y, path, plen, T_out, dtype)),)
        torch = _hip.torch_mod()
        Xd = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
        Yd = torch.from_numpy(np.ascontiguousarray(Y)).to(dev)
        if Xd.dtype not in (torch.float32, torch.float64):
            Xd = Xd.to(torch.float64)
        if Yd.dtype not in (torch.float32, torch.float64):
            Yd = Yd.to(torch.float64)
        lenx = _hip.trim_lengths(Xd)                       # alignment.py:46-49
        leny = _hip.trim_lengths(Yd)
        X64 = Xd if Xd.dtype == torch.float64 else Xd.to(torch.float64)   # fastdtw casts to float
        Y64 = Yd if Yd.dtype == torch.float64 else Yd.to(torch.float64)
        path_i, path_j, path_len, cost = _hip.fastdtw_l2(X64, Y64, lenx, leny, self.radius, dist_kind, dist_scale, tie)   # :50

        def gather(is_x, path, plen, T_out, dtype):
            g = _hip.gather_path(Xd if is_x else Yd, path_i if is_x else path_j, path_len, T_out)   # :52-54,72-73
            return g.cpu().numpy().astype(dtype, copy=False)
        return (path_i.cpu().numpy(), path_j.cpu().numpy(), path_len.cpu().numpy(), cost.cpu().numpy(),
                lenx.cpu().numpy(), leny.cpu().numpy(), gather)

    def _paths_callable(self, X, Y, tie, dev):
        """The same for a ``dist`` only Python can evaluate: trim on the GPU, the local costs of every level's window on
        the host by ``self.dist`` (one call per cell: what upstream fastdtw does with the callable), DP + back-trace +
        window expansion on the GPU."""
        torch = _hip.torch_mod()
        Xd = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
        Yd = torch.from_numpy(np.ascontiguousarray(Y)).to(dev)
        if Xd.dtype not in (torch.float32, torch.float64):
            Xd = Xd.to(torch.float64)
        if Yd.dtype not in (torch.float32, torch.float64):
            Yd = Yd.to(torch.float64)
        lenx = _hip.trim_lengths(Xd).cpu().numpy()         # alignment.py:46-49
        leny = _hip.trim_lengths(Yd).cpu().numpy()
        N = X.shape[0]
        if (lenx <= 0).any() or (leny <= 0).any():
            plen = np.where((lenx > 0) & (leny > 0), 1, 0).astype(np.int32)
            z = np.zeros((N, 1), dtype=np.int32)
            return z, z, plen, np.zeros(N), lenx, leny, None
        xs = [X[n, : int(lenx[n])] for n in range(N)]
        ys = [Y[n, : int(leny[n])] for n in range(N)]
        pi, pj, plen, cost = _hip.fastdtw_callable(xs, ys, self.radius, self.dist, tie, device=dev)   # :50
        d_pi, d_pj, d_pl = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (pi, pj, plen))

        def gather(is_x, path, plen_, T_out, dtype):
            g = _hip.gather_path(Xd if is_x else Yd, d_pi if is_x else d_pj, d_pl, T_out)   # :52-54,72-73
            return g.cpu().numpy().astype(dtype, copy=False)
        return pi, pj, plen, cost, lenx, leny, gather

    def _transform_tensors(self, X, Y):
        """transform() on two CUDA tensors: trim, fastdtw and the gathers on the device, the aligned batches returned as CUDA
        tensors.  One read-back of two integers: the shortest path (the empty-pair error) and the longest (T_out)."""
        torch = _hip.torch_mod()
        for name, t in (("X", X), ("Y", Y)):
            if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 3 and t.dtype in (torch.float32, torch.float64)):
                raise ValueError("DTWAligner: with tensors, X and Y must both be float32 / float64 CUDA tensors of shape (N, T, D) "
                                 "(%s is not)" % name)
        if X.device != Y.device or X.shape[0] != Y.shape[0] or X.shape[2] != Y.shape[2]:
            raise ValueError("DTWAligner: X and Y must be on one device and share N and D, got %s on %s and %s on %s"
                             % (tuple(X.shape), X.device, tuple(Y.shape), Y.device))
        if getattr(self, "devices", None) is not None:
            raise ValueError("DTWAligner: `devices` deals host arrays over several GPUs; tensors are aligned on their own device")
        resolved = _resolve_dist(self.dist)
        if resolved is None:
            raise ValueError("DTWAligner: this `dist` is none of the distances the kernel evaluates itself, so it would have to be "
                             "called on the host once per window cell: pass numpy arrays for that")
        dist_kind, dist_scale = resolved
        if dist_kind != _hip.DIST_L2 and X.shape[2] > _NP_MAX_DIMS:
            raise ValueError("DTWAligner: the kernel reproduces numpy's summation order of this `dist` for at most %d feature dims "
                             "(got %d), so it would have to be evaluated on the host: pass numpy arrays for that" % (_NP_MAX_DIMS, X.shape[2]))
        tie = _hip.TIE_FIRST_MIN if getattr(self, "tie_rule", "first") == "first" else _hip.TIE_DIAG_LAST
        longer = X if X.shape[1] > Y.shape[1] else Y       # alignment.py:44
        N = X.shape[0]
        if N == 0:
            self.path_lengths_ = torch.zeros((0,), dtype=torch.int32, device=X.device)
            return torch.zeros_like(longer), torch.zeros_like(longer)
        _hip.require_gpu(X.device)
        with torch.cuda.device(X.device):
            Xd, Yd = X.contiguous(), Y.contiguous()
            lenx = _hip.trim_lengths(Xd)                   # :46-49
            leny = _hip.trim_lengths(Yd)
            path_i, path_j, path_len, cost = _hip.fastdtw_l2(Xd.to(torch.float64), Yd.to(torch.float64), lenx, leny, self.radius, dist_kind,
                                                             dist_scale, tie)   # :50
            self.path_lengths_ = path_len
            shortest, longest = torch.stack((path_len.min(), path_len.max())).tolist()
            if shortest <= 0:
                bad = int(torch.nonzero(path_len <= 0)[0, 0].item())
                raise ValueError("DTWAligner: pair %d has an empty (all-zero) utterance or could not be aligned" % bad)
            T_out = max(int(longer.shape[1]), int(longest))     # :55-71 (outputs only ever grow)
            Xa = _hip.gather_path(Xd, path_i, path_len, T_out).to(longer.dtype)   # :52-54,72
            Ya = _hip.gather_path(Yd, path_j, path_len, T_out).to(longer.dtype)   # :73
            if self.verbose > 0:
                d = (cost / (lenx + leny)).tolist()             # :51
                for idx in range(N):
                    print("{}, distance: {}".format(idx, d[idx]))
        return Xa, Ya

    def transform(self, XY):
        X, Y = XY
        if not isinstance(X, np.ndarray) or not isinstance(Y, np.ndarray):
            torch = _hip.torch_mod()
            if torch.is_tensor(X) or torch.is_tensor(Y):
                return self._transform_tensors(X, Y)
        assert X.ndim == 3 and Y.ndim == 3                 # alignment.py:42
        longer = X if X.shape[1] > Y.shape[1] else Y       # :44
        N = X.shape[0]
        if N == 0:
            self.path_lengths_ = np.zeros(0, dtype=np.int32)
            return np.zeros_like(longer), np.zeros_like(longer)
        path_i, path_j, plen, cost, lenx, leny, gather = self._paths(X, Y)
        self.path_lengths_ = np.asarray(plen, dtype=np.int32)
        if (plen <= 0).any():
            bad = int(np.flatnonzero(plen <= 0)[0])
            raise ValueError("DTWAligner: pair %d has an empty (all-zero) utterance or could not be aligned" % bad)
        T_out = max(int(longer.shape[1]), int(plen.max()))  # :55-71 (outputs only ever grow)
        Xa = gather(True, path_i, plen, T_out, longer.dtype)   # :52-54,72
        Ya = gather(False, path_j, plen, T_out, longer.dtype)  # :73
        if self.verbose > 0:
            d = cost / (lenx + leny)                        # :51
            for idx in range(N):
                print("{}, distance: {}".format(idx, d[idx]))
        return Xa, Ya


def _gather(src, path, plen, T_out, dtype):
    """out[n, k] = src[n, path[n, k]] for k < plen[n], zeros after: the reference's ``x[pathx]`` written into a
    zero-padded buffer (alignment.py:52-54, 72-73) -- indexing only (row copies), pair by pair."""
    out = np.zeros((src.shape[0], T_out, src.shape[2]), dtype=dtype)
    same = src.dtype == out.dtype
    for n in range(src.shape[0]):
        k = int(plen[n])
        if same:
            np.take(src[n], path[n, :k], axis=0, out=out[n, :k])
        else:
            out[n, :k] = src[n][path[n, :k]]
    return out


class IterativeDTWAligner(object):
    """Align feature matrices iteratively using GMM-based feature conversion
    (alignment.py:79-190): DTW on (converted X, Y) -> joint GMM on the aligned frames ->
    convert X frame-wise with that GMM -> repeat; finally gather the ORIGINAL X along the
    last warping paths.

    The DTW of every iteration is one batched GPU pass over all pairs; the GMM fit is scikit-learn's
    (as in the reference) unless ``gmm="device"`` asks for the float64 EM kernels of
    :func:`nnmnkwii_amd.mixture.fit_gaussian_mixture` (started from scikit-learn's own initialisation on the host, or
    with ``gmm_init="kmeans-device"`` from the same k-means on the device, :func:`nnmnkwii_amd.mixture.kmeans`: an iteration
    then calls neither ``KMeans.fit`` nor ``GaussianMixture.fit``; the posteriors of the conversion come from the device
    E-step too), and the frame-wise conversion is
    :class:`nnmnkwii_amd.baseline.gmm.MLPG` with a static-only window.  Reference behaviours
    kept on purpose: the aligned buffers persist across iterations and only their prefixes are
    rewritten (alignment.py:163-164), the GMM is fitted on the zero padding as well (:175-178), and
    ``random_state`` is left to numpy's global generator (:170-174).  ``dist`` is handled as by
    :class:`DTWAligner` (its ``_paths``), the host-evaluated route for a recognised ``dist`` above 128 dims included.

    Attributes:
        n_iter, dist, radius, verbose, max_iter_gmm, n_components_gmm: as in the reference.
        gmm: "sklearn" (the default) or "device".
        gmm_init: "sklearn" (the default) or "kmeans-device" (with gmm="device" only).
    """

    def __init__(self, n_iter=3, dist=_default_dist, radius=1, max_iter_gmm=100, n_components_gmm=16, verbose=0, *,
                 tie_rule="first", gmm="sklearn", gmm_init="sklearn"):
        if gmm not in ("sklearn", "device"):
            raise ValueError("gmm must be 'sklearn' or 'device', got %r" % (gmm,))
        if gmm_init not in ("sklearn", "kmeans-device"):
            raise ValueError("gmm_init must be 'sklearn' or 'kmeans-device', got %r" % (gmm_init,))
        if gmm_init == "kmeans-device" and gmm != "device":
            raise ValueError("gmm_init='kmeans-device' needs gmm='device'")
        self.gmm = gmm
        self.gmm_init = gmm_init
        self.tie_rule = tie_rule
        self.n_iter = n_iter
        self.dist = dist
        self.radius = radius
        self.max_iter_gmm = max_iter_gmm
        self.n_components_gmm = n_components_gmm
        self.verbose = verbose

    def transform(self, XY):
        from sklearn.mixture import GaussianMixture

        from ..baseline.gmm import MLPG
        from ..mixture import fit_gaussian_mixture

        device_gmm = getattr(self, "gmm", "sklearn") == "device"
        X, Y = XY
        assert X.ndim == 3 and Y.ndim == 3                    # alignment.py:125
        longer = X if X.shape[1] > Y.shape[1] else Y          # :127
        N = len(X)
        Xc = X.copy()                                          # converted X, updated every iteration (:129)
        X_aligned = np.zeros_like(longer)
        Y_aligned = np.zeros_like(longer)
        aligner = DTWAligner(dist=self.dist, radius=self.radius, tie_rule=getattr(self, "tie_rule", "first"))
        path_x, plen = None, None

        for _ in range(self.n_iter):
            path_i, path_j, plen, cost, lenx, leny, gather = aligner._paths(Xc, Y)
            if (plen <= 0).any():
                bad = int(np.flatnonzero(plen <= 0)[0])
                raise ValueError("IterativeDTWAligner: pair %d has an empty (all-zero) utterance" % bad)
            T_out = max(int(X_aligned.shape[1]), int(plen.max()))
            if T_out > X_aligned.shape[1]:                     # outputs only ever grow (:148-162)
                grow = [(0, 0), (0, T_out - X_aligned.shape[1]), (0, 0)]
                X_aligned = np.pad(X_aligned, grow, mode="constant", constant_values=0)
                Y_aligned = np.pad(Y_aligned, grow, mode="constant", constant_values=0)
            Xg = gather(True, path_i, plen, T_out, X_aligned.dtype)
            Yg = gather(False, path_j, plen, T_out, Y_aligned.dtype)
            prefix = (np.arange(T_out)[None, :] < plen[:, None])[:, :, None]
            X_aligned = np.where(prefix, Xg, X_aligned)   # prefix writes (:163-164)
            Y_aligned = np.where(prefix, Yg, Y_aligned)
            path_x = path_i
            if self.verbose > 0:
                dd = cost / (lenx + leny)
                for idx in range(N):
                    print("{}, distance: {}".format(idx, dd[idx]))

            joint = np.concatenate((X_aligned, Y_aligned), axis=-1).reshape(-1, X.shape[-1] * 2)
            if device_gmm:                                     # the same fit (zero padding rows included) by the EM kernels
                gmm = fit_gaussian_mixture(joint, self.n_components_gmm, max_iter=self.max_iter_gmm,
                                           init="kmeans" if getattr(self, "gmm_init", "sklearn") == "kmeans-device" else None)
            else:
                gmm = GaussianMixture(n_components=self.n_components_gmm, covariance_type="full", max_iter=self.max_iter_gmm)
                gmm.fit(joint)                                 # :170-178
            # no delta: frame-wise conversion (:179-180)
            conv = MLPG(gmm, windows=[(0, 0, np.array([1.0]))], posterior="device" if device_gmm else "sklearn")
            nx = lenx                                          # trim_zeros_frames(Xc[idx]) of this iteration
            converted = conv.transform_batch([Xc[idx][: int(nx[idx])] for idx in range(N)])   # one launch (:181-183)
            for idx in range(N):
                Xc[idx][: len(converted[idx])] = converted[idx]

        for idx in range(N):                                   # aligned ORIGINAL X (:186-188)
            n = int(plen[idx])
            X_aligned[idx][:n] = X[idx][path_x[idx, :n]]
        return X_aligned, Y_aligned
