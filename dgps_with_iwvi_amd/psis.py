"""``iwvi_psis_summary`` (csrc/psis.hip) from Python: per point over its S draws the importance-sampled log-mean weight, Kish's effective
sample size, the Pareto-k diagnostic of PSIS and the Pareto-smoothed log-mean weight, in one launch.  ``models.DGP_VI.importance_log_density``
feeds it the layer launch's moments and local regularisers; ``evaluation.psis_summary`` feeds it log-weights that already exist.

Reading khat (Vehtari, Simpson, Gelman, Yao, Gabry): below 0.5 good, 0.5 to 0.7 usable, from 0.7 on the estimate is not reliable at any
practical S.  +inf: the tail was too short for a fit (S < 21, or fewer than five distinct weights above the cutoff)."""
import ctypes

import torch

from . import _abi, settings

MAX_S = _abi.PSIS_MAX_S
KEYS = ("raw", "ess", "khat", "psis")


def summarise(N, S, stride_n, stride_s, terms=None, n_terms=1, fmean=None, fvar=None, Y=None, Dy=0, var_exp=False, lik_variance=1.0,
              lik_variance_dev=None, kls=(), want_logw=False, out=None, want=KEYS):
    """One launch -> dict of device tensors ``raw``, ``ess``, ``khat``, ``psis`` [N] (those named in ``want``) and, with ``want_logw``,
    ``logw`` [N, S].  Row (n, s) of every per-row array is n*stride_n + s*stride_s.  Terms mode: ``terms`` [rows, n_terms]; moments mode:
    ``fmean``, ``fvar`` [rows, Dy] and ``Y`` [N, Dy] with the Gaussian's variance.  ``kls``: [rows, width] arrays subtracted from the
    log-weight.  ``out``: preallocated result tensors (contiguous float32) to write into instead of fresh ones."""
    S, N = int(S), int(N)
    if not 1 <= S <= MAX_S:
        raise ValueError("S must be in 1..%d (one sort of a point's draws in LDS: csrc/sample_sort.h), got %d" % (MAX_S, S))
    if len(kls) > _abi.MAX_KL:
        raise ValueError("more than %d local-regulariser arrays (IWVI_MAX_KL)" % _abi.MAX_KL)
    ref = terms if terms is not None else fmean
    dev = ref.device
    res = {} if out is None else dict(out)
    for k in want:
        if k not in res:
            res[k] = torch.empty(N, dtype=settings.float_type, device=dev)
    if want_logw and "logw" not in res:
        res["logw"] = torch.empty(N, S, dtype=settings.float_type, device=dev)
    for k, t in res.items():
        _abi.dev_tensor(t, k)
    d = _abi.PsisDesc()
    if terms is not None:
        d.terms, d.n_terms = terms.data_ptr(), int(n_terms)
    else:
        d.fmean, d.fvar, d.Y = fmean.data_ptr(), fvar.data_ptr(), Y.data_ptr()
        d.Dy, d.var_exp, d.lik_variance = int(Dy), 1 if var_exp else 0, float(lik_variance)
        d.lik_variance_dev = lik_variance_dev if not isinstance(lik_variance_dev, torch.Tensor) else lik_variance_dev.data_ptr()
    kls = [_abi.dev_tensor(k, "local kl") for k in kls]
    kl_p = _abi.ptr_array(kls)
    kl_n = (ctypes.c_int32 * max(len(kls), 1))(*[k.shape[-1] for k in kls])
    d.kl_local, d.kl_dims, d.n_kl = kl_p, kl_n, len(kls)
    d.N, d.S, d.stride_n, d.stride_s = N, S, int(stride_n), int(stride_s)
    for k, f in (("logw", "out_logw"), ("raw", "out_raw"), ("ess", "out_ess"), ("khat", "out_khat"), ("psis", "out_psis")):
        if k in res:
            setattr(d, f, res[k].data_ptr())
    _abi.check(_abi.lib().iwvi_psis_summary(ctypes.byref(d), _abi.stream_ptr()))
    return res
