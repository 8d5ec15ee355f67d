"""``iwvi_kmeans`` (csrc/kmeans.hip) on the MI355X, through the C-ABI and through ``kmeans.kmeans2``, against the float64 restatement
tests/kmeans_reference.py (pinned to ``scipy.cluster.vq.kmeans2`` bit for bit by tests/test_kmeans_reference_host.py).

Data: ``RandomState(seed).randn(N, D).astype(float32)``; start: ``np.random.seed(seed)`` and SciPy's draw; ten iterations.

    N      M    D  seed  what it can break
    1      1    1  0     degenerate sizes
    63     2    1  1     less than one wave, D = 1
    257    16   3  2     one point past 256, odd D
    4099   128  8  3     the workload's M and D, ragged N
    4099   128  9  6     D just past a template ceiling
    1500   512  32 4     the envelope's corner: the centroids walked in tiles, the clusters in two ranges, 64 doubles of a point in registers
    70001  16   2  5     274 workgroups, the last chunk ragged (a workgroup's walk over several chunks: LARGE_CASES and the switch, below)
    300    128  8  7     clusters of two or three points
and tests/kmeans_reference.py: LARGE_CASES, past the sizes at which the step kernel changes its shape (two points per lane, more chunks than
workgroups).

Before any GPU call every case asserts ON THE REFERENCE ALONE that min_gap > 1e-10: a float64 distance summed in another order (or with
fused multiply-adds) moves by a relative D 2^-52 <= 1e-14, so a gap four orders above that cannot flip a label, and then
  labels, counts   equal the reference's exactly;
  out_Z64          within (N + 1) 2^-52 max|X| of it entrywise (two orders of summing n <= N float64 terms differ by at most
                   2 (n - 1) 2^-53 sum|x_i|; after the division by n, 2 (n - 1) 2^-53 max|x| plus one rounding of the quotient);
  out_Z            the float32 rounding of out_Z64, bitwise;
  out_inertia      within a relative (N + 4 D) 2^-52 (every term is non-negative: each partial sum is bounded by the total)."""
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import kmeans_reference as R   # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def _reference(case, iters=R.ITERS):
    X, C0 = R.case_inputs(*case)
    return (X, C0) + R.kmeans_reference(X, C0, iters)


def _run(dev, X, Z0, iters=R.ITERS, alias=False, with_optional=True):
    """One ``iwvi_kmeans`` call -> dict of NumPy arrays (Z, Z64, labels, counts, inertia)."""
    from dgps_with_iwvi_amd import _abi
    N, D = X.shape
    M = Z0.shape[0]
    Xd = torch.as_tensor(np.ascontiguousarray(X), device=dev)
    Zi = torch.as_tensor(np.ascontiguousarray(Z0), device=dev)
    out = {"Z": Zi if alias else torch.full((M, D), 7.0, dtype=torch.float32, device=dev)}
    if with_optional:
        out.update(Z64=torch.full((M, D), 7.0, dtype=torch.float64, device=dev), labels=torch.full((N,), -7, dtype=torch.int32, device=dev),
                   counts=torch.full((M,), -7, dtype=torch.int32, device=dev), inertia=torch.full((1,), -7.0, dtype=torch.float64, device=dev))
    nbytes = _abi.lib().iwvi_kmeans_ws_bytes(N, M, D)
    assert 0 < nbytes <= 513 * M * D * 8 + 512 * (M * 4 + 8) + 4 * 256                 # the centroids and at most 512 partials, whatever N is
    ws = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=dev)                    # (arbitrary contents)
    p = lambda k: _abi.ptr(out[k]) if k in out else None
    _abi.check(_abi.lib().iwvi_kmeans(_abi.ptr(Xd), N, D, _abi.ptr(Zi), M, iters, p("Z"), p("Z64"), p("labels"), p("counts"), p("inertia"),
                                      _abi.ptr(ws), _abi.stream_ptr()))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _compare(got, ref, X, tag, rows=None):
    """``ref`` = (C, labels, counts, inertia) of the restatement on X (float32); ``rows``: the rows of the device's data the reference ran on."""
    C, labels, counts, inertia = ref
    N, D = X.shape
    glabels = got["labels"] if rows is None else got["labels"][rows]
    ztol = (N + 1) * EPS * float(np.abs(X).max())
    zerr = float(np.abs(got["Z64"] - C).max())
    ierr = abs(float(got["inertia"][0]) - inertia) / inertia if inertia > 0 else abs(float(got["inertia"][0]))
    print("%s: labels differing %d, counts differing %d, max |Z64 - ref| %.3e (bound %.3e), inertia rel. %.3e (bound %.3e)" % (
        tag, int((glabels != labels).sum()), int((got["counts"] != counts).sum()), zerr, ztol, ierr, (N + 4 * D) * EPS))
    assert np.array_equal(glabels, labels) and np.array_equal(got["counts"], counts)
    assert zerr <= ztol
    assert np.array_equal(got["Z"].view(np.uint32), got["Z64"].astype(np.float32).view(np.uint32))
    assert ierr <= (N + 4 * D) * EPS


@pytest.mark.parametrize("max_wg", (2, 3))
@pytest.mark.parametrize("case", [(4099, 128, 8, 3), (4099, 128, 9, 6), (1500, 512, 32, 4), (70001, 16, 2, 5)], ids=lambda c: "N%d-M%d-D%d" % c[:3])
def test_a_workgroup_walks_several_chunks(gpu_device, case, max_wg):
    """The development switch IWVI_KM_MAX_WG caps the step launch's grid at two or three workgroups: every workgroup walks a run of chunks
    (17, 6 or 274 chunks of 256 points over 2 or 3 workgroups), carries its sums across them and, at the envelope's corner, restages the
    centroid tiles for each.  Same reference, same bounds."""
    from dgps_with_iwvi_amd import _abi
    X, C0, C, labels, counts, inertia, gap = _reference(case)
    assert gap > 1e-10
    _abi.set_debug_option("IWVI_KM_MAX_WG", max_wg)
    try:
        got = _run(gpu_device, X, C0)
    finally:
        _abi.set_debug_option("IWVI_KM_MAX_WG", 0)
    _compare(got, (C, labels, counts, inertia), X, "N=%d M=%d D=%d, %d workgroups" % (case[:3] + (max_wg,)))


@pytest.mark.parametrize("case", R.CASES + R.LARGE_CASES, ids=lambda c: "N%d-M%d-D%d" % c[:3])
def test_kmeans_matches_the_reference(gpu_device, case):
    X, C0, C, labels, counts, inertia, gap = _reference(case)
    assert gap > 1e-10                                            # the precondition, on the reference alone
    got = _run(gpu_device, X, C0)
    _compare(got, (C, labels, counts, inertia), X, "N=%d M=%d D=%d" % case[:3])
    # the Python entry: the same draw from NumPy's global stream, the same numbers
    from dgps_with_iwvi_amd import kmeans
    np.random.seed(case[3])
    Z, lab, ine = kmeans.kmeans2(X, case[1], iter=R.ITERS, minit="points", return_inertia=True)
    assert Z.dtype == torch.float32 and lab.dtype == torch.int32 and Z.is_cuda and lab.is_cuda and isinstance(ine, float)
    assert np.array_equal(Z.cpu().numpy().view(np.uint32), got["Z"].view(np.uint32)) and np.array_equal(lab.cpu().numpy(), labels)
    assert ine == float(got["inertia"][0])
    Z64, lab2 = kmeans.kmeans2_f64(torch.as_tensor(X), torch.as_tensor(C0), iter=R.ITERS, minit="matrix")
    assert Z64.dtype == torch.float64 and np.array_equal(Z64.cpu().numpy(), got["Z64"]) and np.array_equal(lab2.cpu().numpy(), labels)


def test_ties_go_to_the_lower_index_and_an_empty_cluster_keeps_its_row(gpu_device):
    rng = np.random.RandomState(0)
    X = rng.randn(40, 3).astype(np.float32)
    X[3] = [100.0, -100.0, 50.0]                                  # far from every other point: its cluster holds it and its copies alone,
    X[10:20] = X[3]                                               # and the mean of eleven copies of a float32 point is that point exactly
    C0 = X[[3, 25, 3, 31]].copy()                                 # rows 0 and 2 identical, in every iteration: 2 can never win
    C, labels, counts, inertia, gap = R.kmeans_reference(X, C0, 3)
    assert gap == 0.0 and counts[2] == 0 and counts[0] == 11 and np.array_equal(C[2], C0[2].astype(np.float64)) and np.array_equal(C[0], C[2])
    got = _run(gpu_device, X, C0, iters=3)
    assert np.array_equal(got["labels"], labels) and np.array_equal(got["counts"], counts) and not (got["labels"] == 2).any()
    assert np.array_equal(got["Z"][2].view(np.uint32), C0[2].view(np.uint32)) and np.array_equal(got["Z64"][2], C0[2].astype(np.float64))
    assert np.abs(got["Z64"] - C).max() <= 41 * EPS * np.abs(X).max()
    assert abs(got["inertia"][0] - inertia) <= (40 + 12) * EPS * inertia


def test_more_centroids_than_points_with_a_matrix_start(gpu_device):
    X = np.random.RandomState(1).randn(5, 2).astype(np.float32)
    C0 = np.concatenate([X + np.float32(0.01), np.full((3, 2), 50.0, dtype=np.float32) + np.arange(6, dtype=np.float32).reshape(3, 2)], 0)
    C, labels, counts, inertia, gap = R.kmeans_reference(X, C0, R.ITERS)
    assert gap > 1e-10 and counts[5:].sum() == 0
    got = _run(gpu_device, X, C0)
    _compare(got, (C, labels, counts, inertia), X, "N=5 M=8 D=2")
    assert np.array_equal(got["Z"][5:].view(np.uint32), C0[5:].view(np.uint32))


def test_one_iteration_labels_against_the_start_and_two_iterations(gpu_device):
    case = (257, 16, 3, 2)
    X, C0 = R.case_inputs(*case)
    for iters in (1, 2):
        C, labels, counts, inertia, gap = R.kmeans_reference(X, C0, iters)
        assert gap > 1e-10
        _compare(_run(gpu_device, X, C0, iters=iters), (C, labels, counts, inertia), X, "iters=%d" % iters)
    d0 = ((X.astype(np.float64)[:, None, :] - C0.astype(np.float64)[None]) ** 2).sum(-1)
    assert np.array_equal(_run(gpu_device, X, C0, iters=1)["labels"], d0.argmin(1))


def test_two_calls_give_the_same_bits(gpu_device):
    X, C0 = R.case_inputs(70001, 16, 2, 5)
    a, b = _run(gpu_device, X, C0), _run(gpu_device, X, C0)
    for k in ("Z", "Z64", "labels", "counts", "inertia"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_a_non_finite_point_gets_label_minus_one_and_takes_no_part(gpu_device):
    from dgps_with_iwvi_amd import kmeans
    X, C0 = R.case_inputs(257, 16, 3, 2)
    X = X.copy()
    X[100, 1] = np.nan
    X[256, 0] = np.inf                                            # (the point past 256)
    rows = np.array([i for i in range(257) if i not in (100, 256)])
    C, labels, counts, inertia, gap = R.kmeans_reference(X[rows], C0, R.ITERS)
    assert gap > 1e-10
    got = _run(gpu_device, X, C0)
    assert got["labels"][100] == -1 and got["labels"][256] == -1
    _compare(got, (C, labels, counts, inertia), X[rows], "two non-finite rows", rows=rows)
    assert got["counts"].sum() == 255
    with pytest.raises(ValueError):
        kmeans.kmeans2(X, C0, minit="matrix", check_finite=True)
    Z, lab = kmeans.kmeans2(X, C0, minit="matrix", check_finite=False)
    assert np.array_equal(Z.cpu().numpy().view(np.uint32), got["Z"].view(np.uint32)) and np.array_equal(lab.cpu().numpy(), got["labels"])


def test_out_Z_may_be_the_start(gpu_device):
    X, C0 = R.case_inputs(4099, 128, 9, 6)
    a, b = _run(gpu_device, X, C0), _run(gpu_device, X, C0, alias=True)
    for k in ("Z", "Z64", "labels", "counts", "inertia"):
        assert a[k].tobytes() == b[k].tobytes(), k
    c = _run(gpu_device, X, C0, with_optional=False)              # every optional output left out
    assert c["Z"].tobytes() == a["Z"].tobytes()


def test_refusals_leave_the_outputs_untouched(gpu_device):
    from dgps_with_iwvi_amd import _abi
    lib = _abi.lib()
    X = torch.zeros(100, 8, device=gpu_device)
    Z = torch.zeros(16, 8, device=gpu_device)
    outs = [torch.full((16, 8), 7.0, device=gpu_device), torch.full((16, 8), 7.0, dtype=torch.float64, device=gpu_device),
            torch.full((100,), -7, dtype=torch.int32, device=gpu_device), torch.full((16,), -7, dtype=torch.int32, device=gpu_device),
            torch.full((1,), -7.0, dtype=torch.float64, device=gpu_device)]
    before = [o.clone() for o in outs]
    ws = torch.zeros(lib.iwvi_kmeans_ws_bytes(100, 16, 8), dtype=torch.uint8, device=gpu_device)
    good = dict(X=_abi.ptr(X), N=100, D=8, Z=_abi.ptr(Z), M=16, iters=10, out=_abi.ptr(outs[0]), ws=_abi.ptr(ws))
    for bad in (dict(X=None), dict(Z=None), dict(out=None), dict(ws=None), dict(N=0), dict(N=-1), dict(N=1 << 31), dict(D=0), dict(D=33),
                dict(M=0), dict(M=513), dict(iters=0), dict(iters=-3)):
        a = dict(good, **bad)
        rc = lib.iwvi_kmeans(a["X"], a["N"], a["D"], a["Z"], a["M"], a["iters"], a["out"], _abi.ptr(outs[1]), _abi.ptr(outs[2]),
                             _abi.ptr(outs[3]), _abi.ptr(outs[4]), a["ws"], _abi.stream_ptr())
        assert rc == _abi.ERR_ARG == -1 and b"iwvi_kmeans" in lib.iwvi_last_error(), bad
    torch.cuda.synchronize()
    for o, b in zip(outs, before):
        assert torch.equal(o, b)


# ---- the model factory ------------------------------------------------------------------------------------------------------------------
def test_build_layers_on_the_device_equals_the_host_to_one_ulp(gpu_device):
    from scipy.cluster.vq import kmeans2 as scipy_kmeans2
    from dgps_with_iwvi_amd import build_models
    X = np.random.RandomState(11).randn(600, 4).astype(np.float32).astype(np.float64)     # float32-valued
    np.random.seed(11)
    start = X[np.random.choice(600, size=32, replace=False)].astype(np.float32)
    assert R.kmeans_reference(X.astype(np.float32), start, 10)[4] > 1e-10
    np.random.seed(11)
    Zs = scipy_kmeans2(X, 32, minit="points")[0]                  # the direct call: what the host mode is, bit for bit
    def gp_layers(**kw):                                          # 'L1_G3': a latent dimension widens the GP layers' inputs to five columns
        np.random.seed(11)
        return [layer for layer in build_models.build_layers("L1_G3", X, 32, **kw) if isinstance(layer, build_models.GPLayer)]

    host, plain, device = gp_layers(kmeans="host"), gp_layers(), gp_layers(kmeans="device")
    assert len(device) == 2 and device[0]._Z().shape == (32, 5)
    z = lambda layer: layer._Z().detach().cpu().numpy()
    for a, b in zip(host, plain):                                 # the default did not move
        assert np.array_equal(z(a), z(b))
    assert np.array_equal(z(host[0])[:, :4], Zs.astype(z(host[0]).dtype))
    for h, d in zip(host, device):
        zh, zd = z(h), z(d)
        assert zh.dtype == zd.dtype and zh.shape == zd.shape
        ulp = np.spacing(np.abs(Zs.astype(np.float32))).astype(np.float64)
        assert np.all(np.abs(zd[:, :4].astype(np.float64) - Zs) <= ulp)              # the float32 rounding of a float64 within (N + 1) 2^-52 of the host's
        assert np.array_equal(zh[:, 4:], zd[:, 4:])                                   # the N(0, 1) columns: the stream stood in the same place
    assert np.array_equal(z(device[1])[:, :4], z(device[0])[:, :4])                   # the deeper layer shares the columns


def test_build_model_with_device_kmeans_trains_one_step(gpu_device):
    from dgps_with_iwvi_amd import build_models
    rng = np.random.default_rng(0)
    X = rng.standard_normal((200, 6)).astype(np.float32)
    Y = (np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.standard_normal((200, 1))).astype(np.float32)
    args = types.SimpleNamespace(mode="IWAE", configuration="L1_G5", M=16, likelihood_variance=0.01, minibatch_size=32, num_IW_samples=4,
                                 use_graph=False, kmeans="device")
    np.random.seed(5)
    model = build_models.build_model(args, X, Y, device=gpu_device)
    assert np.isfinite(float(model.train_op()))
    with pytest.raises(ValueError, match="kmeans"):
        build_models.build_model(types.SimpleNamespace(**dict(vars(args), kmeans="elsewhere")), X, Y, device=gpu_device)
