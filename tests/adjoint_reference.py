"""The float64 reference of one GP layer's adjoint (``iwvi_gp_layer_backward``), restricted to a set of live rows, and the shapes the
layer-adjoint tests share (test_adjoint_reference_host.py, test_gpu_adjoint_live_rows.py, test_gpu_shape_envelope.py).

The reference is ``_layer_reference`` of test_gpu_backward.py generalised: float64 autograd of ``oracle/ref_torch_cpu.py::
CpuDGP._conditional`` under the objective ``sum(cs * sample + cm * mean + cv * var) - klw * KL``, with the mixing matrix W and the Linear
mean function's A as leaves too.  It takes the full [T, .] arrays and an index array ``rows`` and evaluates those rows only: the
objective is a sum over rows, so the parameter gradients are exactly those of the full batch whose other cotangents are zero -- a
reference for T = 20 000 rows then costs what its <= 2048 live rows cost.

``live_rows(T)`` is the live set of every large-T case: a live row in every 16-row tile (hence in every workgroup of every route and in
every 512-row split), the live lane walking through all 16 positions, and the first and last tiles whole."""
import os
import sys
from collections import namedtuple

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.ref_torch_cpu import CpuDGP   # noqa: E402

RTOL = 3e-3              # float32 kernels against float64 autograd, max-norm relative per array (test_gpu_backward.py)
KL_WEIGHT = 0.7
MAX_LIVE = 2048
CHAIN, MID, GEMM = 1, 2, 3


def live_rows(T):
    """All rows of the first and of the last whole 16-row tile, row 16 i + (i mod 16) of every tile i, and the rows of a final partial
    tile -> sorted int64 indices (every row while T <= 32)."""
    T = int(T)
    nt = T // 16
    idx = [np.arange(min(T, 16))]
    if nt:
        i = np.arange(nt)
        idx += [16 * i + i % 16, np.arange(16 * (nt - 1), 16 * nt)]
    idx.append(np.arange(16 * nt, T))
    rows = np.unique(np.concatenate(idx)).astype(np.int64)
    assert len(rows) <= MAX_LIVE, (T, len(rows))
    return rows


def layer_inputs(spec, li, T, seed):
    """N(0, 1) float32 inputs of T rows for GP layer li of the spec -> F [T, D], z [T, R], cs, cm, cv [T, P]."""
    l = spec["layers"][li]
    D, R = l["Z"].shape[1], l["q_mu"].shape[1]
    P = l["W"].shape[0] if l["W"] is not None else R
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((T, D)).astype(np.float32)
    z = rng.standard_normal((T, R)).astype(np.float32)
    cs, cm, cv = (rng.standard_normal((T, P)).astype(np.float32) for _ in range(3))
    return F, z, cs, cm, cv


def mask_rows(rows, *arrays):
    """Zero every row outside ``rows``, in place."""
    dead = np.ones(len(arrays[0]), dtype=bool)
    dead[rows] = False
    for a in arrays:
        a[dead] = 0
    return arrays


PARAM_ARRAYS = ("Z", "ls", "var", "q_mu", "q_sqrt", "W", "A")


def _leaves(L, F=None, override=None, grad=True):
    """Float64 leaf tensors of the layer's parameters (and of the rows F): Z, ls, var, q_mu, q_sqrt, and W, A where the layer has them."""
    val = {k: L[k] for k in PARAM_ARRAYS if k == "var" or L[k] is not None}
    if F is not None:
        val["F"] = F
    val.update(override or {})
    return {k: torch.as_tensor(v.detach().numpy() if torch.is_tensor(v) else np.asarray(v, dtype=np.float64)).clone().requires_grad_(grad)
            for k, v in val.items()}


def _data_term(m, L, P, kern, F, z, cs, cm, cv):
    """sum(cs * sample + cm * mean + cv * var) of the layer on rows F [n, D] (tensors), parameters from the leaves P."""
    Ld = dict(L, Z=P["Z"], ls=P["ls"], q_mu=P["q_mu"], q_sqrt=torch.tril(P["q_sqrt"]), var=P["var"], kern=kern)
    s, mu, v = m._conditional(Ld, F[None], False, z[None])
    if "W" in P:
        s, mu, v = s @ P["W"].T, mu @ P["W"].T, v @ (P["W"] ** 2).T
    if "A" in P:
        s, mu = s + F[None] @ P["A"], mu + F[None] @ P["A"]
    return (cs[None] * s).sum() + (cm[None] * mu).sum() + (cv[None] * v).sum()


def layer_objective(spec, li, F, z, cs, cm, cv, klw, rows=None, kern=None, override=None, grad=True):
    """The objective on the rows ``rows`` (all when None) of the full [T, .] arrays -> (value, leaves): ``leaves`` maps F (the live
    rows only), Z, ls, var, q_mu, q_sqrt and -- where the layer has them -- W, A to float64 leaf tensors.  ``override`` replaces leaf
    values by name (finite differences)."""
    rows = np.arange(len(F)) if rows is None else np.asarray(rows, dtype=np.int64)
    m = CpuDGP(spec, torch.float64)
    L = m.layers[li]
    P = _leaves(L, np.asarray(F)[rows], override, grad)
    t = lambda a: torch.as_tensor(np.asarray(a)[rows], dtype=torch.float64)
    obj = _data_term(m, L, P, kern, P["F"], t(z), t(cs), t(cm), t(cv))
    M, R = L["q_mu"].shape
    Lq = torch.tril(P["q_sqrt"])
    obj = obj - klw * 0.5 * ((P["q_mu"] ** 2).sum() - M * R - torch.log(torch.diagonal(Lq, dim1=-2, dim2=-1) ** 2).sum() + (Lq ** 2).sum())
    return obj, P


def layer_reference(spec, li, F, z, cs, cm, cv, klw, rows=None, kern=None):
    """d objective / d{F[rows], Z, ls, var, q_mu, q_sqrt, W, A} (float64 autograd) -> dict of numpy arrays, W [P, R] and A [D, P] only
    where the layer has a mixing matrix / a Linear mean function."""
    obj, P = layer_objective(spec, li, F, z, cs, cm, cv, klw, rows, kern)
    obj.backward()
    return {k: p.grad.numpy() for k, p in P.items()}


def solo_norms(spec, li, F, z, cs, cm, cv, rows, kern=None):
    """The max-norm of each parameter gradient when row rows[i] alone is live (kl_weight = 0) -> (names, [len(rows), len(names)]):
    one single-row evaluation of the reference's graph per row."""
    m = CpuDGP(spec, torch.float64)
    L = m.layers[li]
    P = _leaves(L)
    names = list(P)
    t = lambda a: torch.as_tensor(np.asarray(a)[rows], dtype=torch.float64)
    Ft, zt, cst, cmt, cvt = t(F), t(z), t(cs), t(cm), t(cv)
    out = np.zeros((len(rows), len(names)))
    for i in range(len(rows)):
        obj = _data_term(m, L, P, kern, Ft[i:i + 1], zt[i:i + 1], cst[i:i + 1], cmt[i:i + 1], cvt[i:i + 1])
        out[i] = [float(g.abs().max()) for g in torch.autograd.grad(obj, [P[k] for k in names])]
    return names, out


# ------------------------------------------------------------------------------------------------------------------------------------
# the shapes: one table for the host test (visibility of every live row) and the GPU test (the adjoint itself)
# ------------------------------------------------------------------------------------------------------------------------------------
# li = 0: the inner layer (D = Dx inputs, R latent GPs, W [Dx, R], Linear mean function), li = 1: the final layer (R = Dy outputs, no W).
# ``fused``: IWVI_BW_FUSED, ``f32``: settings.bw_f32_chain, ``rows``: "live" = live_rows(T), "all" = every row.
# ``route`` = (route, D bucket of the kernel-adjoint template, samples per workgroup) as iwvi_debug_last_backward_routes reports it,
# derived by hand from chain_plan (ns, fits, products) / mid_ok / splitk_chunk of csrc/backward.hip (the comment beside each row).
Case = namedtuple("Case", "id M Dx R li T fused f32 rows route kern")


def _c(id, M, Dx, R, li, T, route, fused=0, f32=False, rows="live", kern=None):
    return Case(id, M, Dx, R, li, T, fused, f32, rows, route, kern)


CASES = [
    # chain_plan: NS = ceil(T / 4096) capped at 5 for M <= 128, lowered to a divisor of T / 16; M = 128 has 8 blocks: split-f16 chain;
    # T / (16 NS) <= 1024 workgroups and M <= 128: dLm / G_r shares formed in the chain (ChainPlan::products)
    _c("chain-ns2", 128, 8, 5, 0, 8192, (CHAIN, 8, 32)),
    _c("chain-ns3", 128, 8, 5, 0, 9600, (CHAIN, 8, 48)),                      # ceil(9600 / 4096) = 3, 600 tiles = 3 * 200
    _c("chain-ns4", 128, 8, 5, 0, 16384, (CHAIN, 8, 64)),
    _c("chain-ns5-final", 128, 8, 1, 1, 20480, (CHAIN, 8, 80)),
    _c("chain-ns5-to-3", 128, 8, 5, 0, 20496, (CHAIN, 8, 48)),               # 1281 tiles = 3 * 7 * 61: 5, 4 do not divide
    _c("chain-ns1-1031-shares", 64, 8, 2, 0, 16496, (CHAIN, 8, 16)),         # 1031 tiles, prime: NS = 1; > 1024 shares: products by split-K GEMM
    _c("chain-ns5-dm16", 128, 12, 5, 0, 20480, (CHAIN, 16, 80)),
    # DM = 32 at NS = 5: at M = 128 the three [M x 84] tiles of the split-f16 chain + the staging of D = 20 are ~182 KB, the plan's `fits` is
    # false at any T > 16384 (the default rule then launches k_bw_mid) -- so M = 64 for the split-f16 chain, and the issue's M = 128
    # shape on the two-tile fp32 chain, which does fit
    _c("chain-ns5-dm32-m64", 64, 20, 5, 0, 20480, (CHAIN, 32, 80)),
    _c("chain-ns5-dm32-f32", 128, 20, 5, 0, 20480, (CHAIN, 32, 80), f32=True),
    _c("chain-m256-32", 256, 20, 2, 0, 16384, (CHAIN, 32, 32)),              # chain_plan's ns: 64 samples do not fit beside D = 20 -> 2 * 16
    _c("gemm-m256-16-splits", 256, 20, 20, 0, 8192, (GEMM, 32, 16)),         # R = 20: the chain does not fit; M > 128: no k_bw_mid by default
    _c("chain-m176-f32-64", 176, 20, 2, 0, 16384, (CHAIN, 32, 64)),          # 11 blocks (odd): fp32 chain, two tiles, 4 * 16 samples fit
    _c("chain-m512-s16", 512, 8, 1, 1, 1024, (CHAIN, 8, 16), rows="all"),    # the plan is ok by s16 (32 blocks); three [512 x 20] tiles fit
    _c("mid-forced-m64", 64, 24, 32, 0, 20480, (MID, 32, 64), fused=1),
    _c("mid-forced-m256", 256, 20, 20, 0, 8192, (MID, 32, 64), fused=1),
    _c("mid-default", 128, 32, 32, 0, 16384, (MID, 32, 64)),                 # the chain does not fit, M = 128, T >= 16384, T % 64 == 0
    _c("gemm-33-splits", 128, 32, 32, 0, 16400, (GEMM, 32, 16)),             # T % 64 != 0: no k_bw_mid; 32 splits of 512 + one of 16
    _c("gemm-ragged", 40, 6, 2, 0, 1541, (GEMM, 8, 16)),                     # Mp = 48 != M; 3 splits of 512 + one of 5
    _c("chain-matern52", 64, 8, 5, 0, 16384, (CHAIN, 8, 64), kern="matern52"),
    # IWVI_BW_F32_CHAIN at even block counts: the flag changes the arithmetic, not the route
    _c("flag-m128-s16", 128, 8, 5, 0, 2048, (CHAIN, 8, 16), rows="all"),
    _c("flag-m128-f32", 128, 8, 5, 0, 2048, (CHAIN, 8, 16), f32=True, rows="all"),
    _c("flag-m256-s16", 256, 8, 5, 0, 2048, (CHAIN, 8, 16), rows="all"),
    _c("flag-m256-f32", 256, 8, 5, 0, 2048, (CHAIN, 8, 16), f32=True, rows="all"),
]


def case_spec(c):
    """The spec of a case: as test_gpu_shape_envelope.py builds its layer cases (the shapes both tables hold are the same cases)."""
    from dgps_with_iwvi_amd import synthetic
    return synthetic.make_spec(L=2, M=c.M, B=8, K=2, Dx=c.Dx, R=c.R if c.li == 0 else 5, Dy=c.R if c.li == 1 else 1, mixing="dense",
                               seed=c.M + c.Dx + c.R)


def case_seed(c):
    return c.T + c.Dx


def case_rows(c):
    return np.arange(c.T, dtype=np.int64) if c.rows == "all" else live_rows(c.T)


def case_inputs(c, spec=None):
    """F, z, cs, cm, cv of a case, the cotangents zeroed outside its live rows; a final layer's cs is zero everywhere (the model passes
    d_sample = None there: the final layer's draw feeds nothing)."""
    F, z, cs, cm, cv = layer_inputs(spec or case_spec(c), c.li, c.T, case_seed(c))
    mask_rows(case_rows(c), cs, cm, cv)
    if c.li == 1:
        cs[:] = 0
    return F, z, cs, cm, cv


def worst_entry(got, ref):
    """(index of the worst entry, its error) -- printed when a max-norm comparison fails."""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    i = np.unravel_index(int(err.argmax()), err.shape)
    return tuple(int(x) for x in i), float(err[i])
