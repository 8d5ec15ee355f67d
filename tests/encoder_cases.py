"""The recognition network (reference layers.py:137-152) at the four places the library evaluates it, as ONE table of cases and a float64
restatement that a host test (tests/test_encoder_cases_host.py) and a GPU test (tests/test_gpu_encoder_envelope.py) both read.
TEST INFRASTRUCTURE ONLY: plain numpy / torch float64 on the CPU, nothing here touches a device.

Sites (include/iwvi_hip.h):
  A  iwvi_lv_layer_forward_act: the layer kernel, one encoder row per sample (csrc/dgp_forward.hip, LV branch of k_dgp_forward)
  B  iwvi_dgp_forward the way a model calls it: the encoder runs once per data point, K samples share its row
  C  iwvi_model_precompute: role_encoder (csrc/precompute.hip), 256 rows per workgroup, up to two encoders, optional sampling tail
  D  iwvi_encoder_backward_act: k_enc_bwd / k_enc_reduce (csrc/backward.hip)

The MLP: for layer l, Z <- Z W_l + b_l; the activation on every layer but the last; Z += Z_in where din == dout.  A missing bias is zero.
Its output is [means (Lw) | raw (Lw)], q_sqrt = softplus(raw - 3) (layers.py:149-150); the layer itself (layers.py:83-103) is ``lv_tail``.

Tolerances.  For each case ``ERR32[id]`` records the maximum absolute error of a float32 restatement of the same arithmetic (``mlp32``,
``lv_tail32``, ``mlp_grads32``: float32 products and sums in a fixed order, elementary functions correctly rounded) against the float64
one, measured on the CPU over all ``MAX_ROWS`` rows (gradients: over every row count of site D, relative to each tensor's maximum).  The
GPU bound of a quantity is ``bound(err32, ref)`` = 8 x that number + 1e-6 x max |ref|.  The factor 8 is an allowance for the kernels'
fmaf accumulation in another order and for __expf / __logf; it is not a measurement, and nothing here is derived from what a kernel returned.

Out of scope: raw - 3 below about -84, where __expf underflows to 0, q_sqrt is 0 and the regulariser is +inf.  Every case that reaches a
regulariser keeps raw - 3 above -84 (asserted on the host); ``raw_ramp`` walks it from -80 (q_sqrt about 1e-35) to 20."""
import collections

import numpy as np

ACTS = ("tanh", "relu", "sigmoid", "softplus", "identity")     # position = IWVI_ACT_* code
MAX_ENC, MAX_D, MAX_WIDTH = 8, 32, 64                           # IWVI_MAX_ENC, IWVI_MAX_D, the encoder width cap of every site
A_ROWS = (1, 17, 100)                                          # sites A and D
C_ROWS = (255, 256, 257, 513)                                  # site C: one short of a block, a block, one past, two blocks and a row
MAX_ROWS = max(C_ROWS)
B_POINTS, B_SAMPLES = 3, 7                                     # site B: npts != samples, last 16-sample tile partly empty (T = 21)
RAW_FLOOR = -84.0                                              # raw - 3 below this is out of scope (see above)
RELU_MARGIN = 1e-4                                             # every reference pre-activation of a relu case is further from the kink
SAT = 30.0                                                     # "saturated": some hidden pre-activation beyond +-SAT
LDS_LIMIT = 160 * 1024

Case = collections.namedtuple("Case", "id dims act bias scale edges seed init last_scale K sampled_kl")


def _case(id, dims, act, edges, bias="all", scale=1.0, seed=0, init="xavier", last_scale=1.0, K=3, sampled_kl=1):
    assert act in ACTS and bias in ("all", "none", "some") and dims[-1] % 2 == 0
    return Case(id, tuple(dims), act, bias, float(scale), tuple(edges), seed, init, float(last_scale), K, sampled_kl)


# The smallest shapes that reach each edge.  ``edges``: what the case is there for (tests/test_encoder_cases_host.py checks that every name
# of EDGES is claimed, and the structural ones against the dims).  ``seed``: the relu cases' seeds were searched for the margin above.
_ACT_DIMS = (7, 12, 12, 8)                                     # Lw = 4, a skip in the middle, XYd % 4 != 0
CASES = [
    _case("base20", (9, 20, 20, 4), "tanh", ("oracle-pin", "skip-middle"), seed=1, K=1, sampled_kl=0),
    # depth
    _case("depth1", (5, 2), "tanh", ("depth-1", "Lw-1", "K-1", "skl-1"), seed=2, K=1, sampled_kl=1),
    _case("depth1_skip", (4, 4), "tanh", ("depth-1-skip", "skip-last"), seed=3, K=3, sampled_kl=0),
    _case("depth8_w6", (7, 6, 6, 6, 6, 6, 6, 6, 6), "softplus", ("depth-max", "skip-middle", "skip-last", "Lw-3", "K-3", "skl-0"), seed=4,
          K=3, sampled_kl=0),
    # width
    _case("w1", (1, 1, 2), "tanh", ("width-1", "skip-first-unaligned", "Lw-1"), seed=5, K=3, sampled_kl=1),
    _case("w33", (3, 33, 2), "sigmoid", ("width-odd", "skip-none", "bias-none"), bias="none", seed=6, K=1, sampled_kl=0),
    _case("w63_64", (9, 63, 64, 6), "tanh", ("width-63", "width-64", "width-odd", "skip-none", "bias-some", "Lw-3"), bias="some", seed=7),
    _case("w64_skip_first", (64, 64, 2), "tanh", ("width-64", "skip-first-aligned"), seed=8, K=1),
    _case("out62", (5, 62, 62), "tanh", ("out-62", "skip-last", "Dx+Lw-cap"), seed=9, K=3, sampled_kl=1),
    _case("skip_first5", (5, 5, 7, 4), "tanh", ("skip-first-unaligned",), seed=10, K=1, sampled_kl=1),
    _case("lw5", (8, 11, 10), "tanh", ("Lw-5", "K-1", "skl-0", "skip-none"), seed=11, K=1, sampled_kl=0),
    # activations at scale 1 and saturated (unbounded activations: a small last layer keeps raw - 3 inside the scope)
    _case("act_tanh_s1", _ACT_DIMS, "tanh", ("act-tanh", "Lw-4", "K-3", "skl-1"), seed=20),
    _case("act_relu_s1", _ACT_DIMS, "relu", ("act-relu", "relu-margin"), seed=120),
    _case("act_sigmoid_s1", _ACT_DIMS, "sigmoid", ("act-sigmoid",), seed=22, sampled_kl=0),
    _case("act_softplus_s1", _ACT_DIMS, "softplus", ("act-softplus",), seed=23),
    _case("act_identity_s1", _ACT_DIMS, "identity", ("act-identity",), seed=24, sampled_kl=0),
    _case("act_tanh_sat", _ACT_DIMS, "tanh", ("sat-tanh",), scale=40.0, seed=30),
    _case("act_relu_sat", _ACT_DIMS, "relu", ("sat-relu", "relu-margin"), scale=40.0, seed=100, last_scale=0.05),
    _case("act_sigmoid_sat", _ACT_DIMS, "sigmoid", ("sat-sigmoid",), scale=40.0, seed=32),
    _case("act_softplus_sat", _ACT_DIMS, "softplus", ("sat-softplus",), scale=40.0, seed=33, last_scale=0.05),
    _case("act_identity_sat", _ACT_DIMS, "identity", ("sat-identity",), scale=40.0, seed=34, last_scale=0.05),
    # raw - 3 = 100 x - 80 for x in [0, 1]: softplus_f and __logf(q_sqrt) from q_sqrt ~ 1e-35 up to the x > 20 branch
    _case("raw_ramp", (1, 2), "tanh", ("softplus-log-range", "depth-1"), seed=40, init="ramp", K=1, sampled_kl=1),
    _case("raw_ramp_kl", (1, 2), "tanh", ("softplus-log-range",), seed=41, init="ramp", K=3, sampled_kl=0),
    # beyond site C's LDS (see LDS and AB_PLAN below)
    _case("over_3x64", (64, 64, 64, 2), "tanh", ("beyond-C-3x64",), seed=50),
    _case("over_full", (64,) * 8 + (2,), "tanh", ("beyond-C-full", "depth-max"), seed=51),
]
BY_ID = {c.id: c for c in CASES}

# two encoders of different shape, activation and row count in ONE precompute launch: the first one's last block is ragged (257 rows: blocks
# 0 and 1), the second starts at blk0 = 2
PAIRS = [dict(id="pair_w33_relu", first=("w33", 257), second=("act_relu_s1", 40), edges=("two-encoders",))]

EDGES = ("oracle-pin", "depth-1", "depth-1-skip", "depth-max", "width-1", "width-odd", "width-63", "width-64", "out-62",
         "skip-first-unaligned", "skip-first-aligned", "skip-middle", "skip-last", "skip-none",
         "act-tanh", "act-relu", "act-sigmoid", "act-softplus", "act-identity",
         "sat-tanh", "sat-relu", "sat-sigmoid", "sat-softplus", "sat-identity", "softplus-log-range", "relu-margin",
         "bias-none", "bias-some", "Lw-1", "Lw-3", "Lw-4", "Lw-5", "K-1", "K-3", "skl-0", "skl-1", "Dx+Lw-cap", "two-encoders",
         "beyond-C-3x64", "beyond-C-full")

# What each site must do with a case, worked out from the code, and the dynamic LDS bytes behind the decision.
#   C  (weights + 4 + 2 * 256 * 65) floats (csrc/precompute.hip, iwvi_model_precompute): above 160 KiB the call is refused BEFORE any launch.
#   D  ((n + 5) * 4 * 65 + weights) floats (csrc/backward.hip, enc_bwd_impl): the full 8 x 64 stack needs 146 640 B, so every admitted
#      encoder is evaluated.
#   A / B  the weights sit in the layer's constant block beside 2 * nsamp * up4(maxdim) floats of activations and the launch's fixed tables
#      (csrc/dgp_forward.hip, fw_plan_lds); plan_fit shrinks the chunk to 16 samples before it gives up.  ``ab``: the bytes
#      iwvi_debug_forward_plan reports for the site-A call at 100 rows and for the site-B call, recorded for the cases beyond C (the plan
#      runs on the host; the GPU test asks again and compares).
# ``expect(case id, site)`` below reads the decision from the recorded tables.


def n_weights(dims):
    return sum(a * b + b for a, b in zip(dims[:-1], dims[1:]))


# ---- recorded figures (regenerate with ``python tests/encoder_cases.py``; the host test recomputes and compares) ----------------------
# id -> (site C bytes, site D bytes, evaluated by C?)
LDS = {
    'base20': (135952, 11136, True),
    'depth1': (133184, 6288, True),
    'depth1_skip': (133216, 6320, True),
    'depth8_w6': (134504, 14888, True),
    'w1': (133160, 7304, True),
    'w33': (133936, 8080, True),
    'w63_64': (153600, 28784, True),
    'w64_skip_first': (150296, 24440, True),
    'out62': (150248, 24392, True),
    'skip_first5': (133552, 8736, True),
    'lw5': (134012, 8156, True),
    'act_tanh_s1': (134560, 9744, True),
    'act_relu_s1': (134560, 9744, True),
    'act_sigmoid_s1': (134560, 9744, True),
    'act_softplus_s1': (134560, 9744, True),
    'act_identity_s1': (134560, 9744, True),
    'act_tanh_sat': (134560, 9744, True),
    'act_relu_sat': (134560, 9744, True),
    'act_sigmoid_sat': (134560, 9744, True),
    'act_softplus_sat': (134560, 9744, True),
    'act_identity_sat': (134560, 9744, True),
    'raw_ramp': (133152, 6256, True),
    'raw_ramp_kl': (133152, 6256, True),
    'over_3x64': (166936, 42120, False),
    'over_full': (250136, 130520, False),
}
# id -> bytes of the forward plan (site A at 100 rows, site B), cases beyond C only
AB_PLAN = {
    'over_3x64': (52912, 52912),
    'over_full': (136112, 136112),
}
# id -> float32-versus-float64 maximum absolute error of: the MLP output, q_sqrt, the layer's sample, its variance, its regulariser (both
# forms), site C's regulariser summed over the latent dimensions (the case's own form), and the parameter gradients relative to each
# tensor's maximum
ERR32 = {
    'base20': dict(out=9.064e-07, sg=5.309e-07, sample=9.658e-07, var=1.510e-06, kl=1.340e-06, kl_sum=1.598e-06, grad=3.307e-07),
    'depth1': dict(out=3.228e-07, sg=1.642e-07, sample=4.313e-07, var=3.257e-07, kl=1.264e-06, kl_sum=1.264e-06, grad=2.617e-07),
    'depth1_skip': dict(out=4.165e-07, sg=1.509e-07, sample=5.367e-07, var=2.453e-07, kl=2.569e-06, kl_sum=2.858e-06, grad=1.737e-07),
    'depth8_w6': dict(out=7.230e-06, sg=5.107e-06, sample=1.517e-05, var=2.758e-04, kl=1.380e-03, kl_sum=6.042e-04, grad=5.410e-07),
    'w1': dict(out=9.004e-08, sg=1.049e-08, sample=4.521e-08, var=1.883e-09, kl=4.313e-07, kl_sum=4.313e-07, grad=2.244e-05),
    'w33': dict(out=5.147e-07, sg=2.696e-08, sample=5.433e-07, var=4.735e-09, kl=6.995e-07, kl_sum=6.023e-07, grad=3.239e-07),
    'w63_64': dict(out=4.786e-07, sg=4.179e-08, sample=4.675e-07, var=1.270e-08, kl=1.092e-06, kl_sum=1.470e-06, grad=3.366e-07),
    'w64_skip_first': dict(out=1.208e-06, sg=7.003e-07, sample=1.211e-06, var=1.456e-06, kl=2.351e-06, kl_sum=2.281e-06, grad=4.009e-07),
    'out62': dict(out=6.663e-07, sg=6.617e-08, sample=6.982e-07, var=3.404e-08, kl=1.274e-06, kl_sum=2.277e-05, grad=4.280e-07),
    'skip_first5': dict(out=2.393e-07, sg=3.746e-08, sample=1.932e-07, var=1.702e-08, kl=4.082e-07, kl_sum=7.113e-07, grad=4.179e-07),
    'lw5': dict(out=3.505e-07, sg=3.642e-08, sample=2.896e-07, var=1.825e-08, kl=7.469e-07, kl_sum=1.826e-06, grad=3.296e-07),
    'act_tanh_s1': dict(out=7.267e-07, sg=1.894e-07, sample=4.492e-07, var=1.979e-07, kl=1.531e-06, kl_sum=2.074e-06, grad=3.157e-07),
    'act_relu_s1': dict(out=1.265e-06, sg=1.769e-07, sample=8.059e-07, var=1.390e-07, kl=2.913e-06, kl_sum=3.759e-06, grad=4.927e-07),
    'act_sigmoid_s1': dict(out=3.876e-07, sg=4.182e-08, sample=4.015e-07, var=1.398e-08, kl=1.282e-06, kl_sum=2.232e-06, grad=3.975e-07),
    'act_softplus_s1': dict(out=8.175e-07, sg=3.270e-07, sample=9.617e-07, var=3.956e-07, kl=2.964e-06, kl_sum=4.806e-06, grad=5.348e-07),
    'act_identity_s1': dict(out=9.664e-07, sg=3.008e-07, sample=6.559e-07, var=5.646e-07, kl=2.068e-06, kl_sum=2.904e-06, grad=3.302e-07),
    'act_tanh_sat': dict(out=2.857e-06, sg=3.754e-07, sample=2.848e-06, var=4.731e-07, kl=6.031e-06, kl_sum=7.415e-06, grad=7.404e-06),
    'act_relu_sat': dict(out=1.065e-06, sg=7.515e-07, sample=1.197e-06, var=4.454e-06, kl=1.411e-05, kl_sum=1.587e-05, grad=2.455e-07),
    'act_sigmoid_sat': dict(out=7.429e-07, sg=1.063e-07, sample=4.438e-07, var=5.842e-08, kl=1.396e-06, kl_sum=3.001e-06, grad=8.576e-07),
    'act_softplus_sat': dict(out=1.027e-06, sg=1.161e-06, sample=2.182e-06, var=1.555e-05, kl=3.761e-05, kl_sum=4.114e-05, grad=3.803e-07),
    'act_identity_sat': dict(out=2.441e-06, sg=2.355e-06, sample=3.657e-06, var=1.868e-05, kl=4.180e-05, kl_sum=3.053e-05, grad=3.096e-07),
    'raw_ramp': dict(out=2.861e-06, sg=2.902e-06, sample=6.442e-06, var=9.868e-05, kl=1.284e-04, kl_sum=1.284e-04, grad=2.463e-07),
    'raw_ramp_kl': dict(out=2.861e-06, sg=2.902e-06, sample=5.812e-06, var=9.868e-05, kl=2.524e-04, kl_sum=4.245e-05, grad=3.334e-07),
    'over_3x64': dict(out=1.691e-06, sg=5.237e-07, sample=1.628e-06, var=1.203e-06, kl=6.466e-06, kl_sum=6.466e-06, grad=4.655e-07),
    'over_full': dict(out=2.248e-06, sg=1.961e-06, sample=2.830e-06, var=1.681e-05, kl=3.061e-05, kl_sum=3.061e-05, grad=6.225e-07),
}


def expect(case_id, site):
    """'evaluate' or 'refuse' (before any launch, with a message)."""
    if site == "C":
        return "evaluate" if LDS[case_id][2] else "refuse"
    return "evaluate"


def latent_dim(case):
    return case.dims[-1] // 2


def layer_width(case):
    """D of the F a site-A / B call carries beside the latent columns, Dx of site C's sampling tail: 3, or what IWVI_MAX_D leaves."""
    return min(3, MAX_D - latent_dim(case))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def make_inputs(case):
    """Everything a site needs, float32 (the reference reads the same rounded values): Ws, bs (None: enc_b == NULL; an entry None: that
    layer has no bias), XY [MAX_ROWS, d0], F / X [MAX_ROWS, layer_width], z [MAX_ROWS * 3, Lw], d_out [MAX_ROWS, 2 Lw].  A site with fewer
    rows takes the leading ones, so the sites see the same rows of the same network."""
    rng = np.random.default_rng(1000 + case.seed)
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    dims, n, Lw = case.dims, len(case.dims) - 1, latent_dim(case)
    if case.init == "ramp":
        assert dims == (1, 2)
        Ws, bs = [f32([[0.5, 100.0]])], [f32([0.1, -77.0])]
        XY = f32(((np.arange(MAX_ROWS) * 37) % 101) / 100.0).reshape(-1, 1)       # any 101 consecutive rows cover 0, 0.01, ..., 1
    else:
        Ws = [f32(rng.standard_normal((a, b)) * (2.0 / (a + b)) ** 0.5) for a, b in zip(dims[:-1], dims[1:])]
        Ws[-1] = f32(Ws[-1] * case.last_scale)
        bs = [f32(rng.standard_normal(b) * 0.2) for b in dims[1:]]
        XY = f32(case.scale * rng.standard_normal((MAX_ROWS, dims[0])))
    if case.bias == "none":
        bs = None
    elif case.bias == "some":
        bs = [b if l % 2 == 0 else None for l, b in enumerate(bs)]
        assert any(b is None for b in bs) and any(b is not None for b in bs)
    return dict(Ws=Ws, bs=bs, XY=XY, F=f32(rng.standard_normal((MAX_ROWS, layer_width(case)))),
                z=f32(rng.standard_normal((MAX_ROWS * 3, Lw))), d_out=f32(rng.standard_normal((MAX_ROWS, 2 * Lw))))


def _bias(bs, l):
    return None if bs is None or bs[l] is None else bs[l]


# ---- float64 restatement ---------------------------------------------------------------------------------------------------------------
def act64(name, x):
    if name == "tanh":
        return np.tanh(x)
    if name == "relu":
        return np.maximum(x, 0.0)
    if name == "sigmoid":
        return np.exp(-np.logaddexp(0.0, -x))
    if name == "softplus":
        return np.logaddexp(0.0, x)
    assert name == "identity"
    return x


def act_grad64(name, x):
    """d act / d x at the pre-activation x."""
    if name == "tanh":
        return 1.0 - np.tanh(x) ** 2
    if name == "relu":
        return (x > 0.0).astype(np.float64)
    if name == "sigmoid":
        s = act64("sigmoid", x)
        return s * (1.0 - s)
    if name == "softplus":
        return act64("sigmoid", x)
    return np.ones_like(x)


def mlp(XY, Ws, bs, dims, act, pre=None):
    """[rows, d0] -> [rows, 2 Lw] in float64.  ``pre``: a list that receives every hidden pre-activation (before the activation)."""
    Z, n = np.asarray(XY, np.float64), len(Ws)
    assert Z.shape[1] == dims[0] and len(dims) == n + 1
    for l, (W, din, dout) in enumerate(zip(Ws, dims[:-1], dims[1:])):
        assert W.shape == (din, dout)
        Z0, b = Z, _bias(bs, l)
        Z = Z @ np.asarray(W, np.float64) + (0.0 if b is None else np.asarray(b, np.float64))
        if l < n - 1:
            if pre is not None:
                pre.append(Z)
            Z = act64(act, Z)
        if din == dout:
            Z = Z + Z0
    return Z


def lv_tail(enc_out, F, z, sampled_kl):
    """layers.py:83-103 on [means | raw] rows -> sample [rows, D + Lw], mean, var, kl [rows, Lw] (per dimension), float64.  The sampled form
    is log q(W) - log p(W) with (W - mu) / q_sqrt written as z, which it is."""
    E, F, z = np.asarray(enc_out, np.float64), np.asarray(F, np.float64), np.asarray(z, np.float64)
    Lw = E.shape[1] // 2
    mu, sg = E[:, :Lw], np.logaddexp(0.0, E[:, Lw:] - 3.0)
    w = mu + z * sg
    if sampled_kl:
        kl = -0.5 * z * z - np.log(sg) + 0.5 * w * w
    else:
        kl = 0.5 * (sg * sg + mu * mu - 1.0) - np.log(sg)
    return np.concatenate([F, w], 1), np.concatenate([F, mu], 1), np.concatenate([np.zeros_like(F), sg * sg], 1), kl


def mlp_grads(XY, Ws, bs, dims, act, d_out):
    """d <mlp(XY), d_out> / d (W_l, b_l) by float64 autograd -> (dWs, dbs); dbs[l] is None where the bias is missing."""
    import torch
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)
    fn = {"tanh": torch.tanh, "relu": torch.relu, "sigmoid": torch.sigmoid, "softplus": torch.nn.functional.softplus,
          "identity": (lambda x: x)}[act]
    W = [t(w).requires_grad_() for w in Ws]
    B = [None if _bias(bs, l) is None else t(_bias(bs, l)).requires_grad_() for l in range(len(Ws))]
    Z, n = t(XY), len(Ws)
    for l, (din, dout) in enumerate(zip(dims[:-1], dims[1:])):
        Z0 = Z
        Z = Z @ W[l] if B[l] is None else Z @ W[l] + B[l]
        if l < n - 1:
            Z = fn(Z)
        if din == dout:
            Z = Z + Z0
    leaves = W + [b for b in B if b is not None]
    g = torch.autograd.grad((Z * t(d_out)).sum(), leaves)
    dW, rest = [x.numpy() for x in g[:n]], [x.numpy() for x in g[n:]]
    db = [None if b is None else rest.pop(0) for b in B]
    return dW, db


# ---- the same arithmetic in float32 (for the tolerances only) --------------------------------------------------------------------------
def _r32(x):
    return np.asarray(x, dtype=np.float32)


def _affine32(X, W, b):
    """X W + b with float32 products and sums, input unit by input unit in order (no fused multiply-add, no library GEMM: the same
    number on every host)."""
    acc = np.zeros((X.shape[0], W.shape[1]), np.float32) if b is None else np.broadcast_to(_r32(b), (X.shape[0], W.shape[1])).copy()
    for i in range(W.shape[0]):
        acc = acc + X[:, i:i + 1] * W[i][None, :]
    assert acc.dtype == np.float32
    return acc


def mlp32(XY, Ws, bs, dims, act, keep=None):
    """``mlp`` in float32: products and sums rounded one by one, the activation correctly rounded (float64 value, rounded once)."""
    Z, n = _r32(XY), len(Ws)
    for l, (W, din, dout) in enumerate(zip(Ws, dims[:-1], dims[1:])):
        Z0 = Z
        Z = _affine32(Z, _r32(W), _bias(bs, l))
        if keep is not None:
            keep.append((Z0, Z))                                 # the layer's input and pre-activation
        if l < n - 1:
            Z = _r32(act64(act, Z.astype(np.float64)))
        if din == dout:
            Z = Z + Z0
    return Z


def lv_tail32(enc_out, F, z, sampled_kl):
    E, z = _r32(enc_out), _r32(z)
    Lw = E.shape[1] // 2
    mu = E[:, :Lw]
    sg = _r32(np.logaddexp(0.0, (E[:, Lw:] - np.float32(3.0)).astype(np.float64)))
    lg = _r32(np.log(sg.astype(np.float64)))
    w = mu + z * sg
    h = np.float32(0.5)
    if sampled_kl:
        kl = -h * z * z - lg + h * w * w
    else:
        kl = h * (sg * sg + mu * mu - np.float32(1.0)) - lg
    assert kl.dtype == np.float32
    return np.concatenate([_r32(F), w], 1), np.concatenate([_r32(F), mu], 1), np.concatenate([np.zeros_like(_r32(F)), sg * sg], 1), kl, sg


def mlp_grads32(XY, Ws, bs, dims, act, d_out):
    """``mlp_grads`` by hand in float32: the forward of ``mlp32``, deltas from the correctly rounded derivative at the float32
    pre-activation, every sum in a fixed order."""
    keep, n = [], len(Ws)
    mlp32(XY, Ws, bs, dims, act, keep)
    g = _r32(d_out)                                              # d / d output of layer l
    dW, db = [None] * n, [None] * n
    for l in range(n - 1, -1, -1):
        Zin, pre = keep[l]
        delta = g if l == n - 1 else g * _r32(act_grad64(act, pre.astype(np.float64)))
        accW, accb = np.zeros(Ws[l].shape, np.float32), np.zeros(Ws[l].shape[1], np.float32)
        for r in range(Zin.shape[0]):
            accW = accW + Zin[r][:, None] * delta[r][None, :]
            accb = accb + delta[r]
        dW[l], db[l] = accW, (None if _bias(bs, l) is None else accb)
        W = _r32(Ws[l])
        gin = np.zeros(Zin.shape, np.float32)
        for o in range(W.shape[1]):
            gin = gin + delta[:, o:o + 1] * W[:, o][None, :]
        g = gin + g if dims[l] == dims[l + 1] else gin
    return dW, db


def rel_to_max(got, ref):
    """max |got - ref| / max |ref| of one tensor (a tensor that is zero throughout: the absolute error)."""
    ref = np.asarray(ref, np.float64)
    m = np.abs(ref).max()
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / (m if m > 0 else 1.0))


def measure_err32(case):
    """The figures ERR32 records for a case (see the module docstring)."""
    inp = make_inputs(case)
    Ws, bs, dims, act = inp["Ws"], inp["bs"], case.dims, case.act
    ref = mlp(inp["XY"], Ws, bs, dims, act)
    got = mlp32(inp["XY"], Ws, bs, dims, act)
    e = dict(out=float(np.abs(got - ref).max()), sample=0.0, var=0.0, kl=0.0, kl_sum=0.0, sg=0.0, grad=0.0)
    z = inp["z"][:MAX_ROWS]
    for skl in (0, 1):
        r = lv_tail(ref, inp["F"], z, skl)
        g = lv_tail32(got, inp["F"], z, skl)
        e["sample"] = max(e["sample"], float(np.abs(g[0] - r[0]).max()))
        e["var"] = max(e["var"], float(np.abs(g[2] - r[2]).max()))
        if np.isfinite(r[3]).all() and np.isfinite(g[3]).all():
            e["kl"] = max(e["kl"], float(np.abs(g[3] - r[3]).max()))
        else:
            e["kl"] = float("inf")
        e["sg"] = max(e["sg"], float(np.abs(g[4] - np.sqrt(r[2][:, inp["F"].shape[1]:])).max()))
        if skl == case.sampled_kl:                               # site C's per-sample regulariser: the Lw terms summed in float32, in order
            acc = np.zeros(g[3].shape[0], np.float32)
            for l in range(g[3].shape[1]):
                acc = acc + g[3][:, l]
            assert acc.dtype == np.float32
            e["kl_sum"] = float(np.abs(acc - r[3].sum(1)).max())
    for rows in A_ROWS:
        rW, rb = mlp_grads(inp["XY"][:rows], Ws, bs, dims, act, inp["d_out"][:rows])
        gW, gb = mlp_grads32(inp["XY"][:rows], Ws, bs, dims, act, inp["d_out"][:rows])
        for a, b in zip(gW + gb, rW + rb):
            assert (a is None) == (b is None)
            if b is not None:
                e["grad"] = max(e["grad"], rel_to_max(a, b))
    return e


def bound(err32, ref, factor=8.0, floor=1e-6):
    """The GPU bound of a quantity whose float32 restatement missed float64 by ``err32``: factor x err32 + floor x max |ref|."""
    return factor * err32 + floor * float(np.abs(np.asarray(ref, np.float64)).max())


def site_c_bytes(dims):
    return (n_weights(dims) + 4 + 2 * 256 * 65) * 4


def site_d_bytes(dims):
    return ((len(dims) - 1 + 5) * 4 * 65 + n_weights(dims)) * 4


def lv_plan(case, T, row_div, row_mod):
    """iwvi_debug_forward_plan of a lone latent-variable layer with the case's encoder -> (status, [variant, grid, LDS bytes])."""
    import ctypes
    from dgps_with_iwvi_amd import _abi
    n, fake = len(case.dims) - 1, 4096                           # (the plan dereferences no data pointer: null or not is all it reads)
    d = _abi.LayerDesc()
    d.type, d.D, d.latent_dim, d.sampled_kl = _abi.LAYER_LV, layer_width(case), latent_dim(case), 1
    W, b = (ctypes.c_void_p * n)(*[fake] * n), (ctypes.c_void_p * n)(*[fake] * n)
    dims = (ctypes.c_int32 * (n + 1))(*case.dims)
    d.enc_W, d.enc_b, d.enc_dims, d.n_enc, d.enc_act = W, b, dims, n, ACTS.index(case.act)
    d.noise, d.zero_noise = fake, 1
    d.sample = d.mean = d.var = d.kl_local = fake
    out = (ctypes.c_int64 * 3)()
    rc = _abi.lib().iwvi_debug_forward_plan((_abi.LayerDesc * 1)(d), 1, fake, d.D, fake, case.dims[0], None, 0, T, row_div, row_mod,
                                            1.0, 0, None, None, None, None, _abi.FW_TAIL_BOUND, out)
    return rc, list(out)


if __name__ == "__main__":                                       # prints the recorded tables
    print("LDS = {")
    for c in CASES:
        print("    %r: (%d, %d, %s)," % (c.id, site_c_bytes(c.dims), site_d_bytes(c.dims), site_c_bytes(c.dims) <= LDS_LIMIT))
    print("}\nERR32 = {")
    for c in CASES:
        e = measure_err32(c)
        print("    %r: dict(%s)," % (c.id, ", ".join("%s=%.3e" % (k, e[k]) for k in ("out", "sg", "sample", "var", "kl", "kl_sum", "grad"))))
    print("}")
