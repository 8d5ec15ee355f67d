"""k-means on the device: ``scipy.cluster.vq.kmeans2`` as the reference calls it for the first-layer inducing inputs
(reference ``experiments/build_models.py:179-180``: ``kmeans2(X, M, minit="points")[0]``), through ``iwvi_kmeans`` (csrc/kmeans.hip).

The subset of SciPy's signature the reference uses.  The loop is SciPy's -- nearest centroid by the squared Euclidean distance summed in
dimension order, ties to the lowest index, means of the members, an empty cluster keeps its row, the labels of the last assignment -- in
float64 formed from the float32 data; the start for ``minit="points"`` is SciPy's own draw, ``data[rng.choice(N, size=k, replace=False)]``
from NumPy's global stream unless ``rng`` is given, so after the same ``np.random.seed(s)`` both start from the same rows and leave the
stream in the same place.  There is no CPU fallback.
"""
import numpy as np
import torch

from . import _abi, settings

__all__ = ["kmeans2", "kmeans2_f64"]


def _to_device(a, name):
    """NumPy array or tensor on any device -> contiguous float32 [rows, D] on ``settings.default_device()``."""
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    if t.dim() != 2:
        raise ValueError("%s must be two-dimensional [rows, D], got shape %s" % (name, tuple(t.shape)))
    return t.detach().to(device=settings.default_device(), dtype=torch.float32).contiguous()


def kmeans2(data, k, iter=10, minit="points", rng=None, check_finite=True, return_inertia=False, return_f64=False):
    """``(centroids, labels)`` as device tensors, float32 [M, D] and int32 [N] (``return_f64``: the centroids before their rounding to
    float32, float64), and the inertia of the last assignment as a Python float when ``return_inertia``.

    ``data`` [N, D]: a NumPy array or a tensor on any device, brought to float32 on ``settings.default_device()`` once.  ``k``: the number
    of clusters with ``minit="points"`` (k <= N), the [M, D] start with ``minit="matrix"``.  ``rng``: a ``numpy.random.RandomState`` or
    ``Generator``; None is NumPy's global stream.  ``check_finite`` raises ValueError for non-finite data, as SciPy does (one reduction and
    one synchronisation); without it such a point gets label -1 and takes no part."""
    if minit not in ("points", "matrix"):
        raise ValueError("minit=%r: the device k-means starts from 'points' or 'matrix'" % (minit,))
    iters = int(iter)
    if iters < 1:
        raise ValueError("iter=%r must be at least 1" % (iter,))
    X = _to_device(data, "data")
    N, D = X.shape
    if N < 1 or not 1 <= D <= _abi.MAX_D:
        raise ValueError("data [%d, %d]: N >= 1 and 1 <= D <= %d" % (N, D, _abi.MAX_D))
    if minit == "matrix":
        Z = _to_device(k, "k")
        if Z.shape[1] != D:
            raise ValueError("k [%d, %d] does not have the data's %d columns" % (Z.shape[0], Z.shape[1], D))
        Z = Z.clone()                                             # (the centroids are written over the start)
    else:
        M = int(k)
        if M < 1 or M > N:
            raise ValueError("k=%r: 1 <= k <= N = %d with minit='points'" % (k, N))
        rng = np.random.mtrand._rand if rng is None else rng
        idx = rng.choice(N, size=M, replace=False)                # SciPy's draw (_kpoints)
        Z = X[torch.as_tensor(np.asarray(idx, dtype=np.int64), device=X.device)].contiguous()
    M = Z.shape[0]
    if not 1 <= M <= _abi.MAX_M:
        raise ValueError("%d clusters: 1 .. %d" % (M, _abi.MAX_M))
    _abi.dev_tensor(X, "data")                                    # (raises off a ROCm device: no CPU fallback)
    if check_finite and not (bool(torch.isfinite(X).all()) and bool(torch.isfinite(Z).all())):
        raise ValueError("data and start must not contain infs or NaNs")
    dev = X.device
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    Z64 = torch.empty(M, D, dtype=torch.float64, device=dev) if return_f64 else None
    inertia = torch.empty(1, dtype=torch.float64, device=dev) if return_inertia else None
    ws = torch.empty(int(_abi.lib().iwvi_kmeans_ws_bytes(N, M, D)), dtype=torch.uint8, device=dev)
    _abi.check(_abi.lib().iwvi_kmeans(_abi.ptr(X), N, D, _abi.ptr(Z), M, iters, _abi.ptr(Z), _abi.ptr(Z64), _abi.ptr(labels), None,
                                      _abi.ptr(inertia), _abi.ptr(ws), _abi.stream_ptr()))
    out = (Z64 if return_f64 else Z, labels)
    return out + (float(inertia.item()),) if return_inertia else out


def kmeans2_f64(data, k, **kw):
    """``kmeans2`` with the float64 centroids (``out_Z64`` of ``iwvi_kmeans``), for comparisons."""
    return kmeans2(data, k, return_f64=True, **kw)
