"""GMM-based feature conversion with MLPG on MI355X.

Host-side mirror of /root/reference/nnmnkwii/baseline/gmm.py:46-247 (``MLPGBase``,
``MLPG``).  By default the mixture posteriors come from scikit-learn, as in the reference (``posterior="device"`` takes them
from the E-step kernel of :mod:`nnmnkwii_amd.mixture` instead and keeps them on the GPU); what
the reference does frame by frame in Python (one ``np.linalg.solve`` per frame and
mixture, gmm.py:111-113,225-229) is ONE launch of ``mlpg_hip_gmm_convert`` over all frames
(the M regression matrices ``S_yx S_xx^-1`` are formed once per model on the host), and the
trajectory generation -- the expensive part -- goes to the HIP MLPG kernels through
:func:`nnmnkwii_amd.paramgen.mlpg`.  ``transform_batch`` converts a whole list of utterances
with one launch (what ``IterativeDTWAligner`` calls every iteration).  ``MLPG.transform_padded`` / ``MLPG.transform_batch`` run
the trajectory conversion of a whole padded batch in three launches -- E-step labels, ``mlpg_hip_gmm_trajectory_stats``, batched
MLPG -- with the model resident on the device.  ``MLPG(..., gv=(gv_mean, gv_var))`` adds the ascent on the likelihood with the gv
term (``mlpg_hip_gv_ascent``, a fourth launch) to all three.
"""
import numpy as np
from scipy import linalg as _sla
from sklearn.mixture import GaussianMixture

from .. import _hip
from ..paramgen import mlpg as _mlpg
from ..paramgen import _mlpg as _pg


def _precisions_cholesky_full(covariances):
    """Upper factors U_k with U_k U_k^T = covariances[k]^-1 (what sklearn stores in
    ``precisions_cholesky_`` for covariance_type="full"; gmm.py:8-41 restates sklearn 0.24)."""
    K, F, _ = covariances.shape
    out = np.empty((K, F, F))
    eye = np.eye(F)
    for k in range(K):
        try:
            c = _sla.cholesky(covariances[k], lower=True)
        except _sla.LinAlgError:
            raise ValueError(
                "Fitting the mixture model failed because some components have ill-defined empirical "
                "covariance (for instance caused by singleton or collapsed samples). Try to decrease the "
                "number of components, or increase reg_covar.")
        out[k] = _sla.solve_triangular(c, eye, lower=True).T
    return out


class MLPGBase(object):
    """Frame-wise conversion E[y | x] under a joint source/target GMM (gmm.py:46-120).

    Attributes (same names as the reference): ``num_mixtures, weights, src_means, tgt_means,
    covarXX, covarXY, covarYX, covarYY, px``.

    ``posterior``: "sklearn" (the default: ``px.predict_proba`` / ``px.predict`` on the host, as the reference) or "device" (the
    float64 E-step kernel, ``mlpg_hip_gmm_estep``; the posteriors, or the arg-max mixtures, stay on the GPU between it and
    ``mlpg_hip_gmm_convert``).
    """

    def __init__(self, gmm, swap=False, diff=False, *, posterior="sklearn"):
        assert gmm.covariance_type == "full"
        if posterior not in ("sklearn", "device"):
            raise ValueError("posterior must be 'sklearn' or 'device', got %r" % (posterior,))
        self.posterior = posterior
        half = gmm.means_.shape[1] // 2
        self.num_mixtures = gmm.means_.shape[0]
        self.weights = gmm.weights_
        mu, cov = gmm.means_, gmm.covariances_
        self.src_means, self.tgt_means = mu[:, :half], mu[:, half:]
        self.covarXX, self.covarXY = cov[:, :half, :half], cov[:, :half, half:]
        self.covarYX, self.covarYY = cov[:, half:, :half], cov[:, half:, half:]

        if diff:  # differential GMM: target := target - source (gmm.py:62-66)
            self.tgt_means = self.tgt_means - self.src_means
            self.covarYY = self.covarXX + self.covarYY - self.covarXY - self.covarYX
            self.covarXY = self.covarXY - self.covarXX
            self.covarYX = self.covarXY.transpose(0, 2, 1)
        if swap:  # gmm.py:69-72
            self.src_means, self.tgt_means = self.tgt_means, self.src_means
            self.covarXX, self.covarYY = self.covarYY, self.covarXX
            self.covarXY, self.covarYX = self.covarYX, self.covarXY

        # p(x): marginal source model, used for the mixture posteriors (gmm.py:76-85)
        px = GaussianMixture(n_components=self.num_mixtures, covariance_type="full")
        px.means_, px.covariances_, px.weights_ = self.src_means, self.covarXX, self.weights
        px.precisions_cholesky_ = _precisions_cholesky_full(px.covariances_)
        self.px = px

    def _regression(self):
        """A[m] = S_yx[m] S_xx[m]^-1, (M, Dy, D), formed once per model (host LAPACK, M small systems)."""
        A = getattr(self, "_A", None)
        if A is None:
            # A^T = S_xx^-1 S_xy  (S_xx symmetric)
            A = np.ascontiguousarray(np.linalg.solve(self.covarXX, self.covarYX.transpose(0, 2, 1)).transpose(0, 2, 1))
            self._A = A
        return A

    def _convert(self, src, posterior=None, mix=None):
        """sum_m posterior[n, m] (mu_y[m] + A[m] (x_n - mu_x[m])) for all rows of ``src`` in one GPU launch
        (``mix``: one mixture per row instead of posterior weights).  Returns a float64 ndarray."""
        torch = _hip.torch_mod()
        dev = _hip.require_gpu()
        f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
        x = f64(src)
        post = f64(posterior) if posterior is not None else None
        mx = torch.from_numpy(np.ascontiguousarray(mix, dtype=np.int32)).to(dev) if mix is not None else None
        out = _hip.gmm_convert(x, post, mx, f64(self.src_means), f64(self.tgt_means), f64(self._regression()))
        return out.cpu().numpy()

    def _convert_device(self, src, hard=False):
        """``_convert`` with the posteriors (``hard``: the most likely mixture of each row) taken from the device E-step under
        p(x) and handed to the conversion kernel without leaving the GPU.  Returns (float64 ndarray, int mixtures or None)."""
        from .. import mixture as _mix
        torch = _hip.torch_mod()
        dev = _hip.require_gpu()
        f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
        x = f64(src)
        w, mu, U, log_det = _mix._model(self.px, dev)
        resp, _, labels, _ = _hip.gmm_estep(x, w, mu, U, log_det, want_resp=not hard, want_labels=hard)
        out = _hip.gmm_convert(x, resp, labels, mu, f64(self.tgt_means), f64(self._regression()))
        return out.cpu().numpy(), (labels.cpu().numpy() if hard else None)

    def _transform_frame(self, src):
        """One frame (D,) -> E[p(y|x)] (gmm.py:97-120)."""
        src = np.asarray(src)
        if self.posterior == "device":
            return self._convert_device(np.atleast_2d(src))[0][0]
        posterior = self.px.predict_proba(np.atleast_2d(src))             # (1, M)
        return self._convert(np.atleast_2d(src), posterior)[0]

    def transform(self, src):
        if src.ndim != 2:
            return self._transform_frame(src)
        tgt = np.zeros_like(src)                                          # dtype of src (gmm.py:89)
        if self.posterior == "device":
            tgt[...] = self._convert_device(src)[0]
            return tgt
        posterior = self.px.predict_proba(src)                            # (T, M): scikit-learn, as the reference
        tgt[...] = self._convert(src, posterior)
        return tgt

    def transform_batch(self, utterances):
        """``[transform(x) for x in utterances]`` with one posterior evaluation and one GPU launch over all frames."""
        utterances = [np.asarray(u) for u in utterances]
        if not utterances:
            return []
        allx = np.concatenate(utterances, axis=0)
        y = self._convert_device(allx)[0] if self.posterior == "device" else self._convert(allx, self.px.predict_proba(allx))
        out, o = [], 0
        for u in utterances:
            t = np.zeros_like(u)
            t[...] = y[o:o + len(u)]
            out.append(t)
            o += len(u)
        return out


class MLPG(MLPGBase):
    """Maximum-likelihood trajectory conversion (Toda 2007) with a joint GMM (gmm.py:123-247).

    ``transform(src)``: per frame the most likely mixture m_t under p(x); E_t and a diagonal
    approximation D_t of the conditional covariance; then ``paramgen.mlpg(E, D, windows)`` on the
    GPU.  Static-only inputs (feature dim == static dim) take the frame-wise path of ``MLPGBase``.

    ``gv=(gv_mean, gv_var)``: mean and variance (static_dim,) of the gv of natural target speech (``paramgen.gv_stats``).  The
    trajectory of static+delta input is then the one that also maximises the likelihood of its gv (Toda 2007, section IV):
    ``paramgen.mlpg_gv`` in ``transform``, one more launch in ``transform_padded`` / ``transform_batch`` with the statistics
    resident on the device beside the model.  ``gv_options``: a dict of ``n_iter``, ``step``, ``init``, ``omega_scale``, ``check``
    (``paramgen.mlpg_gv_batch``).  Not with ``diff=True``.  The reference has no such option.
    """

    def __init__(self, gmm, windows=None, swap=False, diff=False, *, posterior="sklearn", gv=None, gv_options=None):
        super(MLPG, self).__init__(gmm, swap, diff, posterior=posterior)
        if windows is None:
            windows = [(0, 0, np.array([1.0])), (1, 1, np.array([-0.5, 0.0, 0.5]))]
        self.windows = windows
        self.static_dim = gmm.means_.shape[-1] // 2 // len(windows)
        self.gv = None
        if gv is None:
            if gv_options is not None:
                raise ValueError("gv_options go with gv=(gv_mean, gv_var)")
        else:
            if diff:
                raise ValueError("gv cannot be combined with diff=True: the gv of a spectral difference is not the gv of speech")
            opts = dict(n_iter=100, step=None, init="scaled", omega_scale=1.0, check=True)
            unknown = set(gv_options or {}) - set(opts)
            if unknown:
                raise ValueError("unknown gv_options: %s" % ", ".join(sorted(unknown)))
            opts.update(gv_options or {})
            gv_mean, gv_var = gv
            self._gv_check = opts.pop("check")
            gm, _ = _pg._gv_options(gv_mean, gv_var, self.static_dim, **opts)
            self.gv = (gm, np.asarray(gv_var, dtype=np.float64).ravel())
            self.gv_options = opts

    def transform(self, src):
        if src.shape[1] == self.static_dim:
            return super(MLPG, self).transform(src)
        if self.posterior == "device":
            E, mix = self._convert_device(src, hard=True)
        else:
            mix = self.px.predict(src)                                    # sub-optimum mixture sequence, eq. 37
            E = self._convert(src, mix=mix)                               # eq. 22 / 40
        dg = lambda a: np.diagonal(a, axis1=1, axis2=2)                   # noqa: E731
        Dm = dg(self.covarYY) - dg(self.covarYX) / dg(self.covarXX) * dg(self.covarXY)   # eq. 23, diagonal approx.
        if self.gv is not None:
            y = _pg.mlpg_gv_batch(E[None], np.ascontiguousarray(Dm[mix])[None], self.windows, self.gv[0], self.gv[1],
                                  check=self._gv_check, **self.gv_options)
            return y[0].astype(E.dtype, copy=False)
        return _mlpg(E, np.ascontiguousarray(Dm[mix]), self.windows)

    def _device_model(self, dev):
        """(mu_x, mu_y, A, cvar, the E-step model of p(x)) as float64 tensors on ``dev``, uploaded once per device."""
        cache = self.__dict__.setdefault("_dev_models", {})
        got = cache.get(dev.index)
        if got is None:
            from .. import mixture as _mix
            torch = _hip.torch_mod()
            f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
            dg = lambda a: np.diagonal(a, axis1=1, axis2=2)               # noqa: E731
            cvar = dg(self.covarYY) - dg(self.covarYX) / dg(self.covarXX) * dg(self.covarXY)   # eq. 23, as in transform
            px = _mix._model(self.px, dev) if self.posterior == "device" else None
            gvs = None if self.gv is None else (f64(self.gv[0]), f64(1.0 / self.gv[1]))   # (gv_mean, gv_prec) beside the model
            got = cache[dev.index] = (f64(self.src_means), f64(self.tgt_means), f64(self._regression()), f64(cvar), px, gvs)
        return got

    def transform_padded(self, X, lengths=None):
        """``transform`` over a zero-padded batch: ``X`` (B, Tmax, D) static+delta features, numpy of any float dtype or a
        float64 CUDA tensor; ``lengths`` (B,) the live frames per utterance (None: all).  With ``gv`` a fourth launch follows
        (``mlpg_hip_gv_ascent``, in place on the trajectory).  Returns (B, Tmax, static_dim) float64
        of the same kind (what the reference's ``mlpg(E, D, windows)`` returns whatever the dtype of ``src``); frames beyond
        ``lengths`` are zero.  Three launches -- the labels (``posterior="device"``: one E-step over all rows;
        ``"sklearn"``: ``px.predict`` on the live rows on the host, uploaded), ``mlpg_hip_gmm_trajectory_stats``, batched MLPG --
        and with ``posterior="device"`` nothing leaves the device between them."""
        from ..paramgen import mlpg_batch as _mlpg_batch
        torch = _hip.torch_mod()
        is_tensor = torch.is_tensor(X)
        if not is_tensor:
            X = np.asarray(X)
        if (X.dim() if is_tensor else X.ndim) != 3:
            raise ValueError("transform_padded takes a (B, Tmax, D) batch")
        B, T, D = X.shape
        if D == self.static_dim:
            raise ValueError("transform_padded is the trajectory conversion of static+delta features; static-only input "
                             "(feature dim == static dim == %d) goes through transform_batch" % D)
        if D != self.src_means.shape[1]:
            raise ValueError("X has %d features, the model has %d" % (D, self.src_means.shape[1]))
        if is_tensor:
            if not X.is_cuda or X.dtype != torch.float64:
                raise ValueError("tensor input must be a float64 CUDA tensor, got %s on %s" % (X.dtype, X.device))
            dev = _hip.require_gpu(X.device)
            x = X.contiguous()
        else:
            dev = _hip.require_gpu()
            x = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to(dev)
        L = None
        if lengths is not None:
            L = (lengths if torch.is_tensor(lengths) else torch.from_numpy(np.asarray(lengths).astype(np.int32))).to(
                device=dev, dtype=torch.int32).contiguous()
            if L.shape != (B,):
                raise ValueError("lengths must have one entry per utterance")
        if B * T == 0:
            y = torch.zeros((B, T, self.static_dim), dtype=torch.float64, device=dev)
            return y if is_tensor else y.cpu().numpy()
        mu_x, mu_y, A, cvar, px, gvs = self._device_model(dev)
        if self.posterior == "device":
            labels = _hip.gmm_estep(x.view(B * T, D), *px, want_resp=False, want_labels=True)[2]
        else:
            xh = x.cpu().numpy() if is_tensor else np.ascontiguousarray(X, dtype=np.float64)
            live = np.arange(T)[None, :] < (np.full(B, T) if L is None else np.clip(L.cpu().numpy(), 0, T))[:, None]
            lab = np.zeros((B, T), dtype=np.int32)
            if live.any():
                lab[live] = self.px.predict(xh[live])
            labels = torch.from_numpy(lab).to(dev)
        mean, var = _hip.gmm_trajectory_stats(x, L, labels, mu_x, mu_y, A, cvar)
        y = _mlpg_batch(mean, var, self.windows, L)
        if gvs is not None:
            y, report, status = _hip.gv_ascent(mean, var, self.windows, y, gvs[0], gvs[1], L, **self.gv_options)
            if self._gv_check:
                _pg.raise_on_gv_status(status, report, self.gv_options["step"])
        return y if is_tensor else y.cpu().numpy()

    def transform_batch(self, utterances):
        """``[transform(x) for x in utterances]``.  Static+delta input: the utterances are packed into one zero-padded batch and
        converted by ``transform_padded``; the result is a list of (T_i, static_dim) float64 arrays.  Static-only input keeps
        the frame-wise conversion of ``MLPGBase.transform_batch``."""
        utterances = [np.asarray(u) for u in utterances]
        if not utterances or utterances[0].shape[1] == self.static_dim:
            return super(MLPG, self).transform_batch(utterances)
        lens = np.array([len(u) for u in utterances], dtype=np.int32)
        X = np.zeros((len(utterances), int(lens.max()), utterances[0].shape[1]), dtype=np.float64)
        for i, u in enumerate(utterances):
            X[i, :len(u)] = u
        Y = self.transform_padded(X, lens)
        return [Y[i, :n].copy() for i, n in enumerate(lens)]
