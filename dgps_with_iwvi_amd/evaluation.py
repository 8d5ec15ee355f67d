"""The evaluation loop of experiments/run_conditional_density_estimation.py:128-169, batched on the GPU.

The reference walks the test set one point at a time: ``predict_y_samples(x, num_predict_samples)``, a Gaussian
``sklearn.neighbors.KernelDensity`` with Silverman's bandwidth fitted to the samples, its log density at y, the squared
error of the sample mean (and a Shapiro-Wilk statistic of the samples, a diagnostic).  Here ``predict_y_samples`` runs on
batches of test points (the layer kernels; prior-mode latent-variable layers, layers.py:73-81) and
``iwvi_kde_loglik`` evaluates every point's estimate in one launch.

``evaluate(on_device=True)`` keeps the whole loop on the device: ``predict_y_samples_fused`` (the fused forward with a sampling tail)
and per batch one ``iwvi_sample_stats`` launch -- a sort of each point's samples in LDS, then the KDE, the squared error, the
Shapiro-Wilk W and any quantiles from it -- with one read-back at the end.

``kde_log_density_grid`` / ``predictive_density_grid`` evaluate each point's estimate on a whole GRID of levels in one
``iwvi_kde_density_grid`` launch: the conditional density picture of the reference's experiments/demo.py (200 inputs x 10 000 samples x
200 levels), with Silverman's bandwidth or a fixed one; ``evaluate(on_device=True, density_levels=...)`` adds it from the same samples.

``evaluate_mixture`` is the evaluation for ANY likelihood -- class labels, counts, several target columns, where a KDE of
``m + z sqrt(v)`` samples means nothing --: the Monte Carlo log predictive density, and the error / accuracy of the predictive mixture's
mean (``model.predict_mixture``: per batch the layer launch and one ``iwvi_lik_predict_mixture`` launch), with one read-back at the end.

``evaluate_scores`` puts proper scoring rules on the exact draws of any likelihood and any number of target columns: per batch one
``iwvi_sample_scores`` launch per column (CRPS, the counts of a PIT / rank histogram, quantiles and their pinball loss, from the one sort
of ``iwvi_sample_stats``) and, for several columns, one ``iwvi_energy_score`` launch (the multivariate CRPS over all pairs of draws).

``evaluate_importance`` is the held-out log density by importance sampling with the encoders as the proposal
(``model.importance_log_density``: per batch the layer launch and one ``iwvi_psis_summary`` launch) with the diagnostics that say whether
it can be trusted -- the Pareto-k of PSIS and the effective sample size --; ``psis_summary`` gives them for any [N, S] log-weights.

``evaluate_sghmc`` is the evaluation of an SGHMC model over its collected posterior samples: one fused y-sample per kept theta and test point."""
import ctypes

import numpy as np
import torch

from . import _abi, settings


def kde_log_density(samples, y):
    """samples [S, N] (device), y [N] -> (logp [N], sqerr [N], mean_std [N, 2]) through ``iwvi_kde_loglik``."""
    samples = _abi.dev_tensor(samples.contiguous(), "samples")
    S, N = samples.shape
    y = _abi.dev_tensor(y.reshape(-1).contiguous(), "y")
    if y.numel() != N:
        raise ValueError("y has %d entries, samples cover %d points" % (y.numel(), N))
    dev = samples.device
    logp, sq = (torch.empty(N, dtype=settings.float_type, device=dev) for _ in range(2))
    ms = torch.empty(N, 2, dtype=settings.float_type, device=dev)
    _abi.check(_abi.lib().iwvi_kde_loglik(_abi.ptr(samples), N, 1, _abi.ptr(y), N, S, _abi.ptr(logp), _abi.ptr(sq),
                                         _abi.ptr(ms), _abi.stream_ptr()))
    return logp, sq, ms


_SW_C1 = (0.0, 0.221157, -0.147981, -2.071190, 4.434685, -2.706056)      # Royston (1992), the polynomials of the two leading coefficients
_SW_C2 = (0.0, 0.042981, -0.293762, -1.752461, 5.682633, -3.582633)
MAX_SAMPLES = 16384                                                      # iwvi_sample_stats: one point's samples sorted in 64 KiB of LDS


def shapiro_coefficients(S):
    """The S // 2 coefficients a_i of the Shapiro-Wilk statistic W = (sum_i a_i (x_(S+1-i) - x_(i)))^2 / sum_i (x_i - mean)^2 by
    Royston's approximation (Applied Statistics algorithm AS R94), float64, host side: normal scores m_i = Phi^-1((i - 3/8) / (S + 1/4)),
    the two leading coefficients corrected by polynomials in S^-1/2 (only the first for S = 4, 5), the rest m_i rescaled so that the
    squares sum to one; S = 3 (and the degenerate S = 2) has the single exact coefficient sqrt(1/2)."""
    S = int(S)
    if S < 2 or S > MAX_SAMPLES:
        raise ValueError("S=%d out of range (2..%d)" % (S, MAX_SAMPLES))
    if S <= 3:
        return np.array([np.sqrt(0.5)])
    from statistics import NormalDist
    nd = NormalDist()
    h = S // 2
    m = np.array([nd.inv_cdf((i - 0.375) / (S + 0.25)) for i in range(1, h + 1)], dtype=np.float64)   # (negative: the lower half)
    summ2 = 2.0 * float(np.dot(m, m))
    ssumm2, rsn = np.sqrt(summ2), 1.0 / np.sqrt(S)
    a = np.empty(h, dtype=np.float64)
    a1 = np.polyval(_SW_C1[::-1], rsn) - m[0] / ssumm2
    if S > 5:
        a2 = np.polyval(_SW_C2[::-1], rsn) - m[1] / ssumm2
        fac = np.sqrt((summ2 - 2.0 * m[0] ** 2 - 2.0 * m[1] ** 2) / (1.0 - 2.0 * a1 ** 2 - 2.0 * a2 ** 2))
        a[:] = -m / fac
        a[0], a[1] = a1, a2
    else:
        fac = np.sqrt((summ2 - 2.0 * m[0] ** 2) / (1.0 - 2.0 * a1 ** 2))
        a[:] = -m / fac
        a[0] = a1
    return a


_sw_cache = {}


def _shapiro_coefficients_dev(S, dev):
    key = (int(S), str(dev))
    if key not in _sw_cache:
        _sw_cache[key] = torch.as_tensor(shapiro_coefficients(S), dtype=torch.float64, device=dev)
    return _sw_cache[key]


def _check_probs(quantiles):
    q = np.asarray(quantiles, dtype=np.float64).reshape(-1)
    if not np.all((q >= 0.0) & (q <= 1.0)):                               # (NaN fails both comparisons)
        raise ValueError("quantiles must lie in [0, 1], got %s" % (q.tolist(),))
    return q


def sample_stats(samples, y=None, shapiro=True, quantiles=None):
    """samples [S, N] (device, any strides), y [N] or None -> dict of device tensors through one ``iwvi_sample_stats`` launch:
    ``mean_std`` [N, 2] always; ``logp`` and ``sqerr`` [N] (as ``kde_log_density``) when ``y`` is given; ``W`` [N] (Shapiro-Wilk) when
    ``shapiro``; ``quantiles`` [N, len(quantiles)] (NumPy's default linear rule) when asked for.  2 <= S <= 16384."""
    probs = None if quantiles is None else _check_probs(quantiles)
    if not isinstance(samples, torch.Tensor) or samples.dim() != 2:
        raise ValueError("samples must be a [S, N] tensor")
    S, N = samples.shape
    if S < 2 or S > MAX_SAMPLES:
        raise ValueError("S=%d out of range (2..%d)" % (S, MAX_SAMPLES))
    if N > 0 and min(samples.stride()) <= 0:                             # (an expanded view: the kernel takes positive strides)
        samples = samples.contiguous()
    if not samples.is_cuda or samples.dtype != settings.float_type:
        _abi.dev_tensor(samples.contiguous(), "samples")                 # (raises: no CPU fallback, float32 only)
    dev = samples.device
    if y is not None:
        y = _abi.dev_tensor(y.reshape(-1).contiguous(), "y")
        if y.numel() != N:
            raise ValueError("y has %d entries, samples cover %d points" % (y.numel(), N))
    out = {"mean_std": torch.empty(N, 2, dtype=settings.float_type, device=dev)}
    if y is not None:
        out["logp"], out["sqerr"] = (torch.empty(N, dtype=settings.float_type, device=dev) for _ in range(2))
    coef = None
    if shapiro:
        coef = _shapiro_coefficients_dev(S, dev)
        out["W"] = torch.empty(N, dtype=settings.float_type, device=dev)
    pr = None
    if probs is not None:
        pr = torch.as_tensor(probs, dtype=torch.float64, device=dev)
        out["quantiles"] = torch.empty(N, len(probs), dtype=settings.float_type, device=dev)
    if N == 0:
        return out
    ss, sn = samples.stride()
    _abi.check(_abi.lib().iwvi_sample_stats(ctypes.c_void_p(samples.data_ptr()), ss, sn, _abi.ptr(y), N, S, _abi.ptr(coef), _abi.ptr(pr),
                                           0 if probs is None else len(probs), _abi.ptr(out.get("logp")), _abi.ptr(out.get("sqerr")),
                                           _abi.ptr(out["mean_std"]), _abi.ptr(out.get("W")), _abi.ptr(out.get("quantiles")),
                                           _abi.stream_ptr()))
    return out


KDE_GRID_TILE = 64                                                       # csrc/kde_grid.hip: levels per workgroup (KG_TILE) ...
KDE_GRID_CHUNK = 2048                                                    # ... and samples staged in LDS per step (KG_CHUNK)


def _check_bandwidth(bandwidth):
    """None -> 0.0 (the library's Silverman per point); otherwise a finite positive float."""
    if bandwidth is None:
        return 0.0
    h = float(bandwidth)
    if not np.isfinite(h) or h <= 0.0:
        raise ValueError("bandwidth must be None (Silverman's rule per point) or a finite positive number, got %r" % (bandwidth,))
    return h


def _check_levels(levels, N=None):
    """levels [G] or [N, G], G >= 1 (a tensor or anything NumPy takes); returns it unchanged.  ``N`` None: the row count is not checked."""
    shape = tuple(levels.shape) if isinstance(levels, torch.Tensor) else np.shape(levels)
    if len(shape) not in (1, 2) or shape[-1] < 1 or (len(shape) == 2 and N is not None and shape[0] != N):
        raise ValueError("levels must be [G] or [N, G]%s with G >= 1, got %s" % ("" if N is None else " (N = %d)" % N, shape))
    return levels


def kde_log_density_grid(samples, levels, bandwidth=None):
    """samples [S, N] (device, any strides), levels [G] (shared) or [N, G] (per point) -> dict of device tensors through one
    ``iwvi_kde_density_grid`` launch: ``logdens`` [N, G], the log density of each point's Gaussian KDE at each level; ``mean_std`` [N, 2];
    ``bandwidth`` [N], the bandwidth used -- Silverman's 1.06 std S^(-1/5) per point (``bandwidth=None``, S >= 2) or the fixed positive
    value given (S >= 1).  The samples are streamed, not sorted: S is not capped at ``MAX_SAMPLES``."""
    h = _check_bandwidth(bandwidth)
    if not isinstance(samples, torch.Tensor) or samples.dim() != 2:
        raise ValueError("samples must be a [S, N] tensor")
    if samples.dtype != settings.float_type:
        raise ValueError("samples must be %s, got %s" % (settings.float_type, samples.dtype))
    S, N = samples.shape
    if S < (2 if h == 0.0 else 1):
        raise ValueError("S=%d: %s" % (S, "Silverman's bandwidth needs S >= 2" if S == 1 else "no samples"))
    _check_levels(levels, N)
    if isinstance(levels, torch.Tensor) and levels.dtype != settings.float_type:
        raise ValueError("levels must be %s, got %s" % (settings.float_type, levels.dtype))
    if N > 0 and min(samples.stride()) <= 0:                             # (an expanded view: the kernel takes positive strides)
        samples = samples.contiguous()
    if not samples.is_cuda:
        _abi.dev_tensor(samples.contiguous(), "samples")                 # (raises: no CPU fallback)
    dev = samples.device
    if not isinstance(levels, torch.Tensor):
        levels = torch.as_tensor(np.asarray(levels, dtype=np.float32), device=dev)
    levels = _abi.dev_tensor(levels.contiguous(), "levels")
    G = levels.shape[-1]
    out = {"logdens": torch.empty(N, G, dtype=settings.float_type, device=dev),
           "mean_std": torch.empty(N, 2, dtype=settings.float_type, device=dev),
           "bandwidth": torch.empty(N, dtype=settings.float_type, device=dev)}
    if N == 0:
        return out
    ss, sn = samples.stride()
    _abi.check(_abi.lib().iwvi_kde_density_grid(ctypes.c_void_p(samples.data_ptr()), ss, sn, N, S, _abi.ptr(levels),
                                               G if levels.dim() == 2 else 0, G, h, _abi.ptr(out["logdens"]), _abi.ptr(out["mean_std"]),
                                               _abi.ptr(out["bandwidth"]), _abi.stream_ptr()))
    return out


def predictive_density_grid(model, X, levels, num_samples=10000, predict_batch_size=None, bandwidth=None):
    """[N, G] (device): log density of the model's predictive at ``levels`` ([G] or [N, G]) for every row of ``X``, estimated as the
    reference's demo does -- ``num_samples`` predictive samples per input, a Gaussian KDE with Silverman's bandwidth (or a fixed one) --
    with per batch of inputs one sampling launch (``predict_y_samples_fused``; layer by layer for a non-Gaussian likelihood) and one
    ``iwvi_kde_density_grid`` launch.  One output column.  ``predict_batch_size`` None: as many inputs per batch as the sampling launch's
    row budget allows, at least one, so a ``num_samples`` beyond that budget still runs."""
    from .likelihoods import is_gaussian, target_dim
    h = _check_bandwidth(bandwidth)
    S = int(num_samples)
    if S < (2 if h == 0.0 else 1):
        raise ValueError("num_samples=%d too small (Silverman's bandwidth needs 2)" % S)
    # (the TARGET's width: a HeteroskedasticGaussian over one target column has a final layer of two outputs)
    if target_dim(getattr(model, "likelihood", None), model._output_dim()) != 1:
        raise ValueError("the density grid is for one output column, the model has %s" % (model._output_dim(),))
    dev = model.X.device
    X = torch.as_tensor(np.asarray(X, dtype=np.float32), device=dev) if not isinstance(X, torch.Tensor) else X.to(dev, settings.float_type)
    N = X.shape[0]
    _check_levels(levels, N)
    levels = torch.as_tensor(np.asarray(levels, dtype=np.float32), device=dev) if not isinstance(levels, torch.Tensor) else levels.to(dev, settings.float_type)
    bs = max(1, model._PREDICT_ROWS // S) if predict_batch_size is None else int(predict_batch_size)
    if bs < 1:
        raise ValueError("predict_batch_size must be >= 1")
    out = torch.empty(N, levels.shape[-1], dtype=settings.float_type, device=dev)
    fused = is_gaussian(getattr(model, "likelihood", None))
    for lo in range(0, N, bs):
        x = X[lo:lo + bs]
        smp = (model.predict_y_samples_fused(x, S, batch_size=bs) if fused else model.predict_y_samples(x, S))[:, :, 0]    # [S, n]
        out[lo:lo + bs] = kde_log_density_grid(smp, levels if levels.dim() == 1 else levels[lo:lo + bs], bandwidth)["logdens"]
    return out


def _evaluate_on_device(model, X_test, Y_test, num_predict_samples, predict_batch_size, quantiles, density_levels=None):
    parts, grids = [], []
    for lo in range(0, X_test.shape[0], predict_batch_size):
        x, y = X_test[lo:lo + predict_batch_size], Y_test[lo:lo + predict_batch_size]
        smp = model.predict_y_samples_fused(x, num_predict_samples)[:, :, 0]       # [S, n], a point's samples contiguous
        parts.append(sample_stats(smp, y, shapiro=True, quantiles=quantiles))
        if density_levels is not None:                                             # the same samples, one more launch
            lv = density_levels if density_levels.dim() == 1 else density_levels[lo:lo + predict_batch_size]
            grids.append(kde_log_density_grid(smp, lv)["logdens"])
    cat = {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
    # one read-back: the three scalars in one tensor (NumPy's median: the mean of the two middle values for an even count)
    W = cat["W"].double().sort().values
    med = 0.5 * (W[(W.numel() - 1) // 2] + W[W.numel() // 2])
    vals = torch.stack([cat["logp"].double().mean(), cat["sqerr"].double().mean().sqrt(), med]).cpu().numpy()
    res = {"test_loglik": float(vals[0]), "test_rmse": float(vals[1]), "test_shapiro_W_median": float(vals[2])}
    if quantiles is not None:
        res["test_quantiles"] = cat["quantiles"].cpu().numpy()
    if density_levels is not None:
        res["test_density_grid"] = torch.cat(grids).cpu().numpy()
    return res


def evaluate(model, X_test, Y_test, num_predict_samples=2000, predict_batch_size=1000, shapiro=False, mc_loglik=False,
             on_device=False, quantiles=None, density_levels=None):
    """-> dict(test_loglik, test_rmse[, test_shapiro_W_median]) as the reference's ``res`` (:167-169); Y one column.
    ``mc_loglik``: also ``test_loglik_mc``, the mean Monte Carlo log predictive density (``model.predict_log_density`` with
    ``num_predict_samples`` draws per point), the usual DGP test metric beside the reference's KDE estimate.
    ``on_device``: per batch ``predict_y_samples_fused`` and one ``iwvi_sample_stats`` launch, one read-back at the end;
    ``test_shapiro_W_median`` is then always in the result (the reference's row), and ``quantiles=[...]`` (on-device only) adds
    ``test_quantiles`` [N, len(quantiles)], the predictive quantiles per test point; ``density_levels`` ([G] or [N, G], on-device only)
    adds ``test_density_grid`` [N, G], the KDE's log density at those levels from the same samples (``kde_log_density_grid``)."""
    if density_levels is not None:
        if not on_device:
            raise ValueError("density_levels need on_device=True")
        _check_levels(density_levels, np.shape(X_test)[0])
    if quantiles is not None:
        if not on_device:
            raise ValueError("quantiles need on_device=True")
        _check_probs(quantiles)
    dev = model.X.device
    X_test = torch.as_tensor(np.asarray(X_test, dtype=np.float32), device=dev) if not isinstance(X_test, torch.Tensor) else X_test.to(dev, settings.float_type)
    Y_test = torch.as_tensor(np.asarray(Y_test, dtype=np.float32), device=dev) if not isinstance(Y_test, torch.Tensor) else Y_test.to(dev, settings.float_type)
    if Y_test.dim() == 2 and Y_test.shape[1] != 1:
        raise ValueError("the reference's evaluation is for one output column")
    N = X_test.shape[0]
    if N == 0 or Y_test.shape[0] != N:
        raise ValueError("X_test has %d rows, Y_test %d" % (N, Y_test.shape[0]))
    if on_device:
        if density_levels is not None and not isinstance(density_levels, torch.Tensor):
            density_levels = np.asarray(density_levels, dtype=np.float32)
        if density_levels is not None:
            density_levels = torch.as_tensor(density_levels).to(dev, settings.float_type)
        res = _evaluate_on_device(model, X_test, Y_test, num_predict_samples, predict_batch_size, quantiles, density_levels)
        if mc_loglik:
            lp = model.predict_log_density(X_test, Y_test.reshape(N, -1), num_predict_samples, batch_size=predict_batch_size)
            res["test_loglik_mc"] = float(lp.double().mean())
        return res
    logps, sqs, Ws = [], [], []
    for lo in range(0, N, predict_batch_size):
        x, y = X_test[lo:lo + predict_batch_size], Y_test[lo:lo + predict_batch_size]
        smp = model.predict_y_samples(x, num_predict_samples)[:, :, 0]              # [S, n]  (:154-156)
        lp, sq, ms = kde_log_density(smp, y)
        logps.append(lp)
        sqs.append(sq)
        if shapiro:                                                                # diagnostic only; host side like the reference (:164)
            from scipy.stats import shapiro as _shapiro
            z = ((smp - ms[:, 0]) / ms[:, 1]).cpu().numpy()
            Ws += [float(_shapiro(z[:, i])[0]) for i in range(z.shape[1])]
    res = {"test_loglik": float(torch.cat(logps).double().mean()), "test_rmse": float(torch.cat(sqs).double().mean()) ** 0.5}
    if shapiro:
        res["test_shapiro_W_median"] = float(np.median(Ws))
    if mc_loglik:
        lp = model.predict_log_density(X_test, Y_test.reshape(N, -1), num_predict_samples, batch_size=predict_batch_size)
        res["test_loglik_mc"] = float(lp.double().mean())
    return res


def evaluate_sghmc(model, posterior_samples, X_test, Y_test, predict_batch_size=1000, quantiles=None, zs=None, z_y=None,
                   return_samples=False):
    """The reference's evaluation of an SGHMC model (run_conditional_density_estimation.py:136-156): the predictive sample set of a test
    point is ONE ``predict_y_samples(x, 1)`` per kept theta.  ``posterior_samples``: per GP layer a device tensor [S, M, R]
    (``sghmc.SGHMC.collect_samples``).  Every K_uu is factorised once; per kept theta only the layers' q(u) images are re-packed
    (``precompute(q_moved=...)``: IWVI_GP_REUSE_FACTOR) and per batch of points one fused y-sample launch (``iwvi_dgp_predict_samples``,
    S = 1) writes row j of an [S, N] buffer -- column j of its [N, S] transpose --; then one ``iwvi_sample_stats`` pass per batch reads
    each point's S samples through the strides.  Same result keys as ``evaluate(on_device=True)``.  The model's q_mu are restored.
    ``zs`` (per layer [S, N, dim] or None) / ``z_y`` [S, N, Dy]: injected noise (tests); ``return_samples``: also ``samples`` [N, S]."""
    from .layers import GPLayer
    from .likelihoods import is_gaussian
    if not is_gaussian(model.likelihood):
        raise NotImplementedError("evaluate_sghmc adds Gaussian noise in the sampling launch's tail")
    if not model.layers or not all(isinstance(l, GPLayer) for l in model.layers):
        raise NotImplementedError("evaluate_sghmc: a stack of GP layers (no latent-variable layer under SGHMC)")
    if quantiles is not None:
        _check_probs(quantiles)
    if len(posterior_samples) != len(model.layers):
        raise ValueError("posterior_samples needs one [S, M, R] tensor per GP layer")
    S = int(posterior_samples[0].shape[0])
    for l, ps in zip(model.layers, posterior_samples):
        _abi.dev_tensor(ps, "posterior_samples")
        if tuple(ps.shape) != (S,) + tuple(l.q_mu.shape):
            raise ValueError("posterior_samples: expected %s, got %s" % ((S,) + tuple(l.q_mu.shape), tuple(ps.shape)))
    if S < 2 or S > MAX_SAMPLES:
        raise ValueError("S=%d kept samples out of range (2..%d)" % (S, MAX_SAMPLES))
    if model._output_dim() != 1:
        raise ValueError("the reference's evaluation is for one output column")
    dev = model.X.device
    X_test = torch.as_tensor(np.asarray(X_test, dtype=np.float32), device=dev) if not isinstance(X_test, torch.Tensor) else X_test.to(dev, settings.float_type)
    Y_test = torch.as_tensor(np.asarray(Y_test, dtype=np.float32), device=dev) if not isinstance(Y_test, torch.Tensor) else Y_test.to(dev, settings.float_type)
    N = X_test.shape[0]
    if N == 0 or Y_test.shape[0] != N or Y_test.numel() != N:
        raise ValueError("X_test has %d rows, Y_test must be one column of as many, got %s" % (N, tuple(Y_test.shape)))
    if X_test.dim() != 2 or X_test.shape[1] != model._input_dim():
        raise ValueError("X_test must be [N, %s], got %s" % (model._input_dim(), tuple(X_test.shape)))
    bs = int(predict_batch_size)
    if bs < 1:
        raise ValueError("predict_batch_size must be >= 1")
    zs = model._check_predict_noise("evaluate_sghmc", S, N, zs)
    if z_y is not None and tuple(z_y.shape) != (S, N, 1):
        raise ValueError("z_y must be [S, N, 1] = %s, got %s" % ((S, N, 1), tuple(z_y.shape)))
    X_test = X_test.contiguous()
    buf = torch.empty(S, N, dtype=settings.float_type, device=dev)
    moved = set(range(len(model.layers)))
    chain = [l.q_mu.clone() for l in model.layers]
    try:
        model.precompute()                                           # the one factorisation
        for j in range(S):
            for l, ps in zip(model.layers, posterior_samples):
                l.q_mu.copy_(ps[j])
            model.precompute(q_moved=moved)
            for lo in range(0, N, bs):
                hi = min(N, lo + bs)
                nb = hi - lo
                zb = [None if z is None else z[j, lo:hi].to(dev, settings.float_type).reshape(nb, -1).contiguous() for z in zs]
                zyb = None if z_y is None else _abi.dev_tensor(z_y[j, lo:hi].to(dev, settings.float_type).reshape(nb, 1).contiguous(), "z_y")
                model._fused_forward(nb, 1, nb, (nb,), zs=zb, want_logw=False, use_encoder=False, X=X_test[lo:hi],
                                     predict=dict(S=1, out_y=buf[j, lo:hi].view(nb, 1, 1), z_y=zyb))
    finally:
        for l, t in zip(model.layers, chain):
            l.q_mu.copy_(t)
    parts = [sample_stats(buf[:, lo:lo + bs], Y_test.reshape(-1)[lo:lo + bs], shapiro=True, quantiles=quantiles) for lo in range(0, N, bs)]
    cat = {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
    W = cat["W"].double().sort().values
    med = 0.5 * (W[(W.numel() - 1) // 2] + W[W.numel() // 2])
    vals = torch.stack([cat["logp"].double().mean(), cat["sqerr"].double().mean().sqrt(), med]).cpu().numpy()   # the one read-back
    res = {"test_loglik": float(vals[0]), "test_rmse": float(vals[1]), "test_shapiro_W_median": float(vals[2])}
    if quantiles is not None:
        res["test_quantiles"] = cat["quantiles"].cpu().numpy()
    if return_samples:
        res["samples"] = buf.t()
    return res


def evaluate_mixture(model, X_test, Y_test, num_predict_samples=2000, predict_batch_size=1000, return_predictions=False):
    """-> dict from ``model.predict_mixture(X_test, num_predict_samples, Y_test)``, any likelihood, any number of target columns:
    ``test_loglik_mc``, the mean Monte Carlo log predictive density (taken in float64); ``test_rmse``, the mixture mean against Y (every
    likelihood but ``MultiClass``); ``test_accuracy``: ``Bernoulli`` -- mixture mean > 1/2 against Y --, ``MultiClass`` -- the arg-max of the
    mixture's class probabilities against the label, the first maximum on ties.  ``return_predictions``: also ``mean`` and ``var``
    [N, Dout] (NumPy).  One read-back at the end."""
    from .likelihoods import Bernoulli
    dev = model.X.device
    X_test = torch.as_tensor(np.asarray(X_test, dtype=np.float32), device=dev) if not isinstance(X_test, torch.Tensor) else X_test.to(dev, settings.float_type)
    Y_host = None if isinstance(Y_test, torch.Tensor) else np.asarray(Y_test, dtype=np.float32)
    Y_test = torch.as_tensor(Y_host, device=dev) if Y_host is not None else Y_test.to(dev, settings.float_type)
    N = X_test.shape[0]
    if N == 0 or Y_test.dim() != 2 or Y_test.shape[0] != N:
        raise ValueError("X_test has %d rows, Y_test must be [%d, columns], got %s" % (N, N, tuple(Y_test.shape)))
    # (targets given on the host are checked there, by predict_mixture, without a read-back)
    pm = model.predict_mixture(X_test, num_predict_samples, Y=Y_test if Y_host is None else Y_host, batch_size=predict_batch_size)
    stats = [pm["log_density"].double().mean()]
    names = ["test_loglik_mc"]
    if getattr(model.likelihood, "num_classes", None) is not None:
        # torch.argmax does not promise the first maximum: the smallest index at which the row's maximum is attained
        C = pm["mean"].shape[1]
        idx = torch.arange(C, device=dev).expand_as(pm["mean"])
        first = torch.where(pm["mean"] == pm["mean"].max(1, keepdim=True).values, idx, torch.full_like(idx, C)).min(1).values
        stats.append((first == Y_test[:, 0].to(torch.int64)).double().mean())
        names.append("test_accuracy")
    else:
        stats.append(((pm["mean"] - Y_test).double() ** 2).mean().sqrt())
        names.append("test_rmse")
        if isinstance(model.likelihood, Bernoulli):
            stats.append(((pm["mean"] > 0.5) == (Y_test == 1)).double().mean())
            names.append("test_accuracy")
    vals = torch.stack(stats).cpu().numpy()                          # the one read-back of the scalars
    res = {k: float(v) for k, v in zip(names, vals)}
    if return_predictions:
        res["mean"], res["var"] = pm["mean"].cpu().numpy(), pm["var"].cpu().numpy()
    return res


def evaluate_draws(model, X_test, Y_test, num_predict_samples=2000, predict_batch_size=1000, interval=0.9):
    """Posterior-predictive check of ONE target column, any likelihood, from the exact draws of ``model.predict_y_draws``: per batch of
    ``predict_batch_size`` points one draw of ``num_predict_samples`` targets per point and one ``sample_stats`` launch (one sort) ->
    ``test_coverage``, the share of targets inside the central ``interval`` of their draws (the empirical quantiles at (1 -+ interval) / 2,
    both ends included: the draws of a count or a label are discrete); ``test_interval_width``, that interval's mean width;
    ``test_rmse``, the draws' mean against Y; and for the continuous likelihoods (Gaussian, Student-t, Exponential, Gamma, Beta)
    ``test_loglik``, the reference's KDE test log-likelihood (run_conditional_density_estimation.py:148-165) from the same launch.
    One read-back at the end."""
    from .likelihoods import target_dim
    if not 0.0 < float(interval) < 1.0:
        raise ValueError("interval must lie in (0, 1), got %r" % (interval,))
    dev = model.X.device
    X_test = torch.as_tensor(np.asarray(X_test, dtype=np.float32), device=dev) if not isinstance(X_test, torch.Tensor) else X_test.to(dev, settings.float_type)
    Y_test = torch.as_tensor(np.asarray(Y_test, dtype=np.float32), device=dev) if not isinstance(Y_test, torch.Tensor) else Y_test.to(dev, settings.float_type)
    N = X_test.shape[0]
    if target_dim(model.likelihood, model._output_dim()) != 1:
        raise ValueError("evaluate_draws is for one target column, the model has %s" % (model._output_dim(),))
    if N == 0 or Y_test.numel() != N:
        raise ValueError("X_test has %d rows, Y_test must be [%d, 1], got %s" % (N, N, tuple(Y_test.shape)))
    Y_test = Y_test.reshape(N)
    continuous = not isinstance(model.likelihood, _discrete_likelihoods())
    probs = [0.5 * (1.0 - float(interval)), 0.5 * (1.0 + float(interval))]
    parts = []
    for lo in range(0, N, int(predict_batch_size)):
        x, y = X_test[lo:lo + predict_batch_size], Y_test[lo:lo + predict_batch_size]
        smp = model.predict_y_draws(x, num_predict_samples)[:, :, 0]                # [S, n], a point's draws contiguous
        parts.append(sample_stats(smp, y, shapiro=False, quantiles=probs))
    cat = {k: torch.cat([p[k] for p in parts]) for k in parts[0]}
    q = cat["quantiles"].double()
    inside = (Y_test.double() >= q[:, 0]) & (Y_test.double() <= q[:, 1])
    stats = [inside.double().mean(), (q[:, 1] - q[:, 0]).mean(), cat["sqerr"].double().mean().sqrt()]
    names = ["test_coverage", "test_interval_width", "test_rmse"]
    if continuous:
        stats.append(cat["logp"].double().mean())
        names.append("test_loglik")
    vals = torch.stack(stats).cpu().numpy()                                         # the one read-back
    return {k: float(v) for k, v in zip(names, vals)}


# ---- proper scoring rules of predictive draws: CRPS, PIT, pinball loss, energy score ----------------------------------------------------
def _discrete_likelihoods():
    """The likelihoods whose targets are counts or labels (``evaluate_draws``: no KDE; ``evaluate_scores``: a randomized PIT)."""
    from .likelihoods import Bernoulli, MultiClass, Ordinal, Poisson
    return (Bernoulli, MultiClass, Ordinal, Poisson)


def sample_scores(samples, y, quantiles=None):
    """samples [S, N] (device, any strides), y [N] -> dict of device tensors through one ``iwvi_sample_scores`` launch (one sort per
    point, the one of ``sample_stats``): ``crps`` and ``crps_fair`` [N], the CRPS of the draws' empirical distribution and its fair
    (unbiased) version; ``below`` and ``equal`` [N] (int32), the number of draws below y and equal to y (``pit_values`` turns them into a
    PIT); ``quantiles`` [N, len(quantiles)] (bit-equal to ``sample_stats``'s) and ``pinball`` [N, len(quantiles)], the quantile loss of
    each, when asked for.  A point with a NaN draw or a NaN y: NaN, and -1 in both counts.  2 <= S <= 16384."""
    probs = None if quantiles is None else _check_probs(quantiles)
    if not isinstance(samples, torch.Tensor) or samples.dim() != 2:
        raise ValueError("samples must be a [S, N] tensor")
    S, N = samples.shape
    if S < 2 or S > MAX_SAMPLES:
        raise ValueError("S=%d out of range (2..%d)" % (S, MAX_SAMPLES))
    if not isinstance(y, torch.Tensor) or y.numel() != N:
        raise ValueError("y must be a tensor of %d entries, one per point of samples" % N)
    if N > 0 and min(samples.stride()) <= 0:                             # (an expanded view: the kernel takes positive strides)
        samples = samples.contiguous()
    if not samples.is_cuda or samples.dtype != settings.float_type:
        _abi.dev_tensor(samples.contiguous(), "samples")                 # (raises: no CPU fallback, float32 only)
    dev = samples.device
    y = _abi.dev_tensor(y.reshape(-1).contiguous(), "y")
    crps = torch.empty(N, 2, dtype=settings.float_type, device=dev)
    counts = torch.empty(N, 2, dtype=torch.int32, device=dev)
    out = {"crps": crps[:, 0], "crps_fair": crps[:, 1], "below": counts[:, 0], "equal": counts[:, 1]}
    pr = None
    if probs is not None:
        pr = torch.as_tensor(probs, dtype=torch.float64, device=dev)
        out["quantiles"], out["pinball"] = (torch.empty(N, len(probs), dtype=settings.float_type, device=dev) for _ in range(2))
    if N == 0:
        return out
    ss, sn = samples.stride()
    _abi.check(_abi.lib().iwvi_sample_scores(ctypes.c_void_p(samples.data_ptr()), ss, sn, _abi.ptr(y), N, S, _abi.ptr(pr),
                                            0 if probs is None else len(probs), _abi.ptr(crps), _abi.ptr(counts),
                                            _abi.ptr(out.get("quantiles")), _abi.ptr(out.get("pinball")), _abi.stream_ptr()))
    return out


def energy_score(samples, Y):
    """samples [S, N, D] (device, any positive strides -- the [N, S, D] view of ``predict_y_draws`` included), Y [N, D] -> dict of device
    tensors through one ``iwvi_energy_score`` launch: ``energy`` and ``energy_fair`` [N], (1/S) sum_s |x_s - y| - B / S^2 and
    - B / (S (S - 1)) with B = sum_{s<t} |x_s - x_t|: the multivariate CRPS (D = 1: the CRPS itself).  2 <= S <= 16384, 1 <= D <= 32."""
    if not isinstance(samples, torch.Tensor) or samples.dim() != 3:
        raise ValueError("samples must be a [S, N, D] tensor")
    S, N, D = samples.shape
    if S < 2 or S > MAX_SAMPLES:
        raise ValueError("S=%d out of range (2..%d)" % (S, MAX_SAMPLES))
    if D < 1 or D > _abi.MAX_P:
        raise ValueError("D=%d out of range (1..%d)" % (D, _abi.MAX_P))
    if not isinstance(Y, torch.Tensor) or tuple(Y.shape) != (N, D):
        raise ValueError("Y must be a [N, D] = %s tensor, got %s" % ((N, D), tuple(Y.shape) if isinstance(Y, torch.Tensor) else type(Y).__name__))
    if N > 0 and min(samples.stride()) <= 0:
        samples = samples.contiguous()
    if not samples.is_cuda or samples.dtype != settings.float_type:
        _abi.dev_tensor(samples.contiguous(), "samples")                 # (raises: no CPU fallback, float32 only)
    Y = _abi.dev_tensor(Y.contiguous(), "Y")
    es = torch.empty(N, 2, dtype=settings.float_type, device=samples.device)
    if N > 0:
        ss, sn, sd = samples.stride()
        _abi.check(_abi.lib().iwvi_energy_score(ctypes.c_void_p(samples.data_ptr()), ss, sn, sd, _abi.ptr(Y), N, S, D, _abi.ptr(es),
                                               _abi.stream_ptr()))
    return {"energy": es[:, 0], "energy_fair": es[:, 1]}


def pit_values(below, equal, S, randomized=False, generator=None):
    """The probability integral transform of each target among its S draws, from the counts of ``sample_scores``, float64 on the counts'
    device: the mid-rank (below + equal / 2 + 1/2) / (S + 1) by default; ``randomized``: uniform in [below, below + equal + 1) / (S + 1)
    (``torch.rand`` on that device, ``generator`` optional) -- what a discrete target, whose draws tie with it all the time, needs for a
    flat histogram under a calibrated model.  A point the kernel marked invalid (counts -1) gets NaN."""
    S = int(S)
    if S < 1:
        raise ValueError("S=%d: no draws" % S)
    b, e = below.to(torch.float64), equal.to(torch.float64)
    if b.shape != e.shape:
        raise ValueError("below %s and equal %s differ in shape" % (tuple(b.shape), tuple(e.shape)))
    if randomized:
        u = torch.rand(b.shape, dtype=torch.float64, device=b.device, generator=generator)
        pit = (b + u * (e + 1.0)) / (S + 1.0)
    else:
        pit = (b + 0.5 * e + 0.5) / (S + 1.0)
    return torch.where(b < 0, torch.full_like(pit, float("nan")), pit)


def _pit_summary(pit, bins):
    """[bins + 1] float64 on pit's device: the histogram's counts over ``bins`` equal bins of [0, 1], then sup_u |ECDF(u) - u|."""
    pit = pit.reshape(-1).to(torch.float64)
    n = pit.numel()
    idx = torch.clamp((pit * bins).to(torch.int64), 0, bins - 1)
    counts = torch.zeros(bins, dtype=torch.float64, device=pit.device).scatter_add_(0, idx, torch.ones_like(pit))
    p = pit.sort().values
    i = torch.arange(1, n + 1, dtype=torch.float64, device=pit.device)
    ks = torch.maximum(i / n - p, p - (i - 1.0) / n).max()
    return torch.cat([counts, ks.reshape(1)])


def pit_histogram(pit, bins=10):
    """-> dict(counts [bins] (NumPy int64): the PIT / rank histogram over equal bins of [0, 1]; calibration_error: the Kolmogorov distance
    sup_u |ECDF_PIT(u) - u| between the PIT values and the uniform distribution, 0 for a calibrated predictive).  Device ops, one read-back."""
    bins = int(bins)
    if bins < 1:
        raise ValueError("bins must be >= 1")
    if not isinstance(pit, torch.Tensor) or pit.numel() == 0:
        raise ValueError("pit must be a non-empty tensor")
    v = _pit_summary(pit, bins).cpu().numpy()
    return {"counts": v[:bins].astype(np.int64), "calibration_error": float(v[bins])}


def evaluate_scores(model, X_test, Y_test, num_predict_samples=2000, predict_batch_size=1000, quantiles=(0.05, 0.25, 0.5, 0.75, 0.95),
                    pit_bins=10, randomized_pit=None):
    """Proper scoring rules and calibration of the predictive distribution, for ANY likelihood and any number Dt >= 1 of target columns,
    from the exact draws of ``model.predict_y_draws`` (``predict_y_samples`` for a ``cvae.CVAE``): per batch of ``predict_batch_size``
    points one draw of ``num_predict_samples`` targets per point, one ``iwvi_sample_scores`` launch per target column and, for Dt > 1,
    one ``iwvi_energy_score`` launch.  Means over the test points: ``test_crps``, ``test_crps_fair``; ``test_pinball`` (one per entry of
    ``quantiles``); ``test_pit_hist`` (``pit_bins`` counts) and ``test_calibration_error`` (``pit_histogram``) -- each a list with one
    entry per column when Dt > 1, which then also has ``test_energy_score`` / ``test_energy_score_fair``.  ``randomized_pit`` None: the
    randomized PIT exactly for the discrete likelihoods (Bernoulli, MultiClass, Ordinal, Poisson), the mid-rank otherwise.
    One read-back at the end."""
    from .cvae import CVAE
    from .likelihoods import target_dim
    probs = _check_probs(quantiles)
    if probs.size == 0:
        raise ValueError("evaluate_scores needs at least one quantile")
    S, bs, bins = int(num_predict_samples), int(predict_batch_size), int(pit_bins)
    if S < 2 or S > MAX_SAMPLES:
        raise ValueError("num_predict_samples=%d out of range (2..%d)" % (S, MAX_SAMPLES))
    if bs < 1 or bins < 1:
        raise ValueError("predict_batch_size and pit_bins must be >= 1")
    dev = model.X.device
    X_test = torch.as_tensor(np.asarray(X_test, dtype=np.float32), device=dev) if not isinstance(X_test, torch.Tensor) else X_test.to(dev, settings.float_type)
    Y_test = torch.as_tensor(np.asarray(Y_test, dtype=np.float32), device=dev) if not isinstance(Y_test, torch.Tensor) else Y_test.to(dev, settings.float_type)
    N = X_test.shape[0]
    is_cvae = isinstance(model, CVAE)
    Dt = model._output_dim() if is_cvae else target_dim(model.likelihood, model._output_dim())
    if N == 0 or Y_test.dim() != 2 or tuple(Y_test.shape) != (N, Dt):
        raise ValueError("X_test has %d rows, Y_test must be [%d, %d], got %s" % (N, N, Dt, tuple(Y_test.shape)))
    if Dt > _abi.MAX_P:
        raise ValueError("%d target columns: the energy score takes up to %d" % (Dt, _abi.MAX_P))
    if randomized_pit is None:
        randomized_pit = isinstance(model.likelihood, _discrete_likelihoods())
    Y_test = Y_test.contiguous()
    cols, energy = [[] for _ in range(Dt)], []
    for lo in range(0, N, bs):
        x, y = X_test[lo:lo + bs], Y_test[lo:lo + bs]
        smp = model.predict_y_samples(x, S) if is_cvae else model.predict_y_draws(x, S)         # [S, n, Dt], a point's draws contiguous
        for d in range(Dt):
            cols[d].append(sample_scores(smp[:, :, d], y[:, d], quantiles=probs))
        if Dt > 1:
            energy.append(energy_score(smp, y))
    stats = []
    for d in range(Dt):
        cat = {k: torch.cat([p[k] for p in cols[d]]) for k in cols[d][0]}
        pit = pit_values(cat["below"], cat["equal"], S, randomized=bool(randomized_pit))
        stats += [cat["crps"].double().mean().reshape(1), cat["crps_fair"].double().mean().reshape(1), cat["pinball"].double().mean(0),
                  _pit_summary(pit, bins)]
    if Dt > 1:
        stats += [torch.cat([e[k] for e in energy]).double().mean().reshape(1) for k in ("energy", "energy_fair")]
    vals = torch.cat(stats).cpu().numpy()                                           # the one read-back
    nq, per = len(probs), 2 + len(probs) + bins + 1
    by_col = []
    for d in range(Dt):
        v = vals[d * per:(d + 1) * per]
        by_col.append(dict(test_crps=float(v[0]), test_crps_fair=float(v[1]), test_pinball=[float(t) for t in v[2:2 + nq]],
                           test_pit_hist=[int(t) for t in v[2 + nq:2 + nq + bins]], test_calibration_error=float(v[per - 1])))
    res = dict(by_col[0]) if Dt == 1 else {k: [c[k] for c in by_col] for k in by_col[0]}
    if Dt > 1:
        res["test_energy_score"], res["test_energy_score_fair"] = float(vals[Dt * per]), float(vals[Dt * per + 1])
    return res


def psis_summary(logw):
    """Importance log-weights ``logw`` [N, S] (device float32, any strides -- the transposed [S, N] view or a slice included) -> dict of
    device tensors [N] through one ``iwvi_psis_summary`` launch: ``log_mean`` = logsumexp_s - log S, ``log_mean_psis`` (the same with the
    Pareto-smoothed tail), ``khat`` (the Pareto-k diagnostic: below 0.5 good, below 0.7 usable, from 0.7 on the weights cannot be trusted
    at any practical S; +inf: no fit) and ``ess`` (Kish).  S <= 16384.  The training log-weights are one input:
    ``psis_summary(model._logw().view(B, K))`` -- its ``ess`` is ``model.importance_ess()``, and its ``khat`` says what the effective
    sample size cannot: whether the weights have a tail that one more draw could overturn."""
    from . import psis
    if not isinstance(logw, torch.Tensor) or logw.dim() != 2:
        raise ValueError("logw must be a [N, S] tensor")
    if logw.dtype != settings.float_type:
        raise TypeError("logw must be %s, got %s" % (settings.float_type, logw.dtype))
    if not logw.is_cuda:
        raise _abi.IwviError("logw is on %s: iwvi_psis_summary is a gfx950 HIP kernel (there is no CPU fallback)" % logw.device)
    N, S = logw.shape
    sn, ss = logw.stride()
    if sn < 0 or ss < 0:
        raise ValueError("logw strides must not be negative")
    r = psis.summarise(N, S, sn, ss, terms=logw, n_terms=1)
    return {"log_mean": r["raw"], "log_mean_psis": r["psis"], "khat": r["khat"], "ess": r["ess"]}


def evaluate_importance(model, X_test, Y_test, num_importance_samples=5000, predict_batch_size=None, proposal="encoder"):
    """-> dict from ``model.importance_log_density(X_test, Y_test, num_importance_samples, proposal)``: ``test_loglik_is``, the mean
    importance-sampled log density (taken in float64), ``test_loglik_psis``, the mean of its Pareto-smoothed form, and what says whether
    either can be trusted: ``test_khat_median``, ``test_khat_max``, ``test_khat_bad_share`` (the share of points with khat > 0.7),
    ``test_ess_median``, ``test_ess_min``.  One read-back at the end."""
    dev = model.X.device
    X_test = torch.as_tensor(np.asarray(X_test, dtype=np.float32), device=dev) if not isinstance(X_test, torch.Tensor) else X_test.to(dev, settings.float_type)
    Y_test = torch.as_tensor(np.asarray(Y_test, dtype=np.float32), device=dev) if not isinstance(Y_test, torch.Tensor) else Y_test.to(dev, settings.float_type)
    N = X_test.shape[0]
    if N == 0 or Y_test.dim() != 2 or Y_test.shape[0] != N:
        raise ValueError("X_test has %d rows, Y_test must be [%d, columns], got %s" % (N, N, tuple(Y_test.shape)))
    r = model.importance_log_density(X_test, Y_test, num_importance_samples, proposal=proposal, batch_size=predict_batch_size)
    kh, ess = r["khat"].double(), r["ess"].double()
    stats = [r["log_density"].double().mean(), r["log_density_psis"].double().mean(), kh.median(), kh.max(), (kh > 0.7).double().mean(),
             ess.median(), ess.min()]
    names = ["test_loglik_is", "test_loglik_psis", "test_khat_median", "test_khat_max", "test_khat_bad_share", "test_ess_median", "test_ess_min"]
    vals = torch.stack(stats).cpu().numpy()                          # the one read-back of the scalars
    return {k: float(v) for k, v in zip(names, vals)}
