"""NumPy float64 restatement of ``iwvi_kmeans`` (csrc/kmeans.hip), which is the loop of ``scipy.cluster.vq.kmeans2``, and the inputs its
tests share.  tests/test_kmeans_reference_host.py pins it to SciPy bit for bit; tests/test_gpu_kmeans.py holds the kernels to it."""
import numpy as np

ITERS = 10
# (N, M, D, seed): what each can break is listed in tests/test_gpu_kmeans.py
CASES = [(1, 1, 1, 0), (63, 2, 1, 1), (257, 16, 3, 2), (4099, 128, 8, 3), (4099, 128, 9, 6), (1500, 512, 32, 4), (70001, 16, 2, 5),
         (300, 128, 8, 7)]
# beyond 131 072 points: a lane owns two points at D <= 16 (the first and the last case), and there are more chunks than the step launch
# has workgroups (512: the first two cases), so some workgroups walk two
LARGE_CASES = [(263001, 4, 1, 8), (131329, 3, 17, 9), (140001, 5, 12, 10)]


def case_inputs(N, M, D, seed):
    """Standard normal float32 data and the start SciPy's minit="points" takes after np.random.seed(seed)."""
    X = np.random.RandomState(seed).randn(N, D).astype(np.float32)
    np.random.seed(seed)
    return X, X[np.random.choice(N, size=M, replace=False)].copy()


def kmeans_reference(X, C0, iters):
    """(centroids [M, D], labels [N] of the last assignment, counts [M] and inertia at that assignment, min_gap).  ``min_gap``: the smallest
    (d2 - d1) / (d2 + d1) over all points and iterations, d1 <= d2 a point's two smallest squared distances (inf for M = 1): how far the
    nearest tie is from flipping a label."""
    assert X.dtype == np.float32 and C0.dtype == np.float32
    X, C = X.astype(np.float64), C0.astype(np.float64).copy()
    min_gap = np.inf
    for _ in range(iters):
        # the distance table [N, M], 1024 rows at a time (the same numbers as in one piece; the piece at M = 512, D = 32 would be 200 MB)
        d = np.concatenate([((X[i:i + 1024, None, :] - C[None]) ** 2).sum(-1) for i in range(0, X.shape[0], 1024)], 0)
        labels = d.argmin(1)                                      # (the first minimum: ties to the lowest index)
        if C.shape[0] > 1:
            d2 = np.partition(d, 1, axis=1)[:, :2]
            den = d2[:, 1] + d2[:, 0]                             # (0: a point on two coinciding centroids, an exact tie)
            min_gap = min(min_gap, float(np.where(den > 0, (d2[:, 1] - d2[:, 0]) / np.where(den > 0, den, 1.0), 0.0).min()))
        counts = np.bincount(labels, minlength=C.shape[0])
        inertia = float(d[np.arange(X.shape[0]), labels].sum())
        # a cluster's members added up in point order, as SciPy does (bincount runs through the points once; a .sum() would go pairwise)
        sums = np.stack([np.bincount(labels, weights=X[:, j], minlength=C.shape[0]) for j in range(X.shape[1])], 1)
        live = counts > 0                                         # an empty cluster keeps its row
        C[live] = sums[live] / counts[live, None]
    return C, labels.astype(np.int32), counts.astype(np.int32), inertia, min_gap
