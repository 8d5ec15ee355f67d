"""A restatement of the CVAE baseline (reference experiments/build_models.py:29-142) in torch on the CPU, written from its semantics -- test
infrastructure like tests/lik_restatement.py: the GPU tests compare the kernels of csrc/cvae.hip against it in float64, and the host tests
run it in float32 to show that the tolerances the GPU tests apply are ten times the arithmetic's own noise.

  encoder  [x, y] -> (means | raw), tanh after every linear map but the last, no skip connections
  raw_c = clip(raw, ln 1e-12, ln 1e10) with zero gradient outside (tf.clip_by_value);  sigma = exp(raw_c / 2);  z = mu + eps sigma
  decoder  [z, x] -> yhat
  elbo = sum_{n,d} log N(y_nd; yhat_nd, variance) - sum_{n,j} KL(N(mu_nj, sigma_nj^2) || N(0, 1)), over the rows given, no N / B scale

``dtype=torch.float32`` runs every per-row quantity in float32 and adds the rows up in float64, which is what the kernels do.
"""
import math

import numpy as np
import torch

CLIP_LO, CLIP_HI = math.log(1e-12), math.log(1e10)
ACTS = {"tanh": torch.tanh, "relu": torch.relu, "sigmoid": torch.sigmoid, "softplus": torch.nn.functional.softplus, "identity": lambda t: t}


def widths(hidden, Dx, Dy, L):
    hidden = list(hidden)
    return [Dx + Dy] + hidden + [2 * L], [L + Dx] + hidden + [Dy]


def mlp(h, Ws, bs, act):
    for i, (W, b) in enumerate(zip(Ws, bs)):
        h = h @ W + b
        if i < len(Ws) - 1:
            h = act(h)
    return h


def clip_raw(raw):
    """tf.clip_by_value: the value is clamped, the gradient passes where lo <= raw <= hi and is zero elsewhere."""
    inside = ((raw >= CLIP_LO) & (raw <= CLIP_HI)).to(raw.dtype)
    lo, hi = torch.tensor(CLIP_LO, dtype=raw.dtype), torch.tensor(CLIP_HI, dtype=raw.dtype)
    clamped = torch.minimum(torch.maximum(raw.detach(), lo), hi)
    return raw * inside + (clamped - raw.detach() * inside)


def kl_to_standard_normal(mu, sigma2, log_sigma2):
    return 0.5 * (sigma2 + mu * mu - 1.0 - log_sigma2)


def gaussian_log_density(y, mean, variance):
    return -0.5 * math.log(2.0 * math.pi) - 0.5 * torch.log(variance) - 0.5 * (y - mean) ** 2 / variance


def decoder(p, z, x, act="tanh"):
    return mlp(torch.cat([z, x], 1), p["Ws_dec"], p["bs_dec"], ACTS[act])


def bound(p, X, Y, eps, act="tanh"):
    """-> (elbo, sum log p, sum KL) as float64 scalars carrying autograd history; p: dict of tensors Ws, bs, Ws_dec, bs_dec, variance."""
    L = eps.shape[1]
    enc = mlp(torch.cat([X, Y], 1), p["Ws"], p["bs"], ACTS[act])
    mu, raw = enc[:, :L], enc[:, L:]
    rc = clip_raw(raw)
    sigma = torch.exp(0.5 * rc)
    yhat = decoder(p, mu + eps * sigma, X, act)
    logp = gaussian_log_density(Y, yhat, p["variance"]).double().sum()
    kl = kl_to_standard_normal(mu, sigma * sigma, rc).double().sum()
    return logp - kl, logp, kl


def to_params(case, dtype, requires_grad=True):
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype, requires_grad=requires_grad)
    return {"Ws": [t(w) for w in case["Ws"]], "bs": [t(b) for b in case["bs"]], "Ws_dec": [t(w) for w in case["Ws_dec"]],
            "bs_dec": [t(b) for b in case["bs_dec"]], "variance": t(case["variance"])}


def value_and_grads(case, dtype=torch.float64, act="tanh"):
    """-> dict of NumPy float64: elbo, logp, kl, and the gradients dWs, dbs, dWs_dec, dbs_dec (lists), dvariance, plus `raw` [B, L]."""
    p = to_params(case, dtype)
    X, Y, eps = (torch.tensor(case[k], dtype=dtype) for k in ("X", "Y", "eps"))
    elbo, logp, kl = bound(p, X, Y, eps, act)
    elbo.backward()
    g = lambda t: t.grad.detach().double().numpy()
    with torch.no_grad():
        raw = mlp(torch.cat([X, Y], 1), p["Ws"], p["bs"], ACTS[act])[:, eps.shape[1]:].double().numpy()
    return {"elbo": elbo.item(), "logp": logp.item(), "kl": kl.item(), "dWs": [g(w) for w in p["Ws"]], "dbs": [g(b) for b in p["bs"]],
            "dWs_dec": [g(w) for w in p["Ws_dec"]], "dbs_dec": [g(b) for b in p["bs_dec"]], "dvariance": float(p["variance"].grad), "raw": raw}


def samples(case, Xs, z, z_y, dtype=torch.float64, act="tanh", y_noise=True):
    """predict_y_samples in the kernels' layout: z [N, S, L], z_y [N, S, Dy] -> [N, S, Dy] (NumPy float64)."""
    p = to_params(case, dtype, requires_grad=False)
    Xs, z = torch.tensor(Xs, dtype=dtype), torch.tensor(z, dtype=dtype)
    N, S, L = z.shape
    x = Xs[:, None, :].expand(N, S, Xs.shape[1]).reshape(N * S, -1)
    y = decoder(p, z.reshape(N * S, L), x, act)
    if y_noise:
        y = y + torch.sqrt(p["variance"]) * torch.tensor(z_y, dtype=dtype).reshape(N * S, -1)
    return y.reshape(N, S, -1).double().numpy()


def make_case(hidden, Dx, Dy, L, B, seed=0, variance=0.05, clip=False):
    """Inputs for one shape: Xavier weights as the reference draws them (N(0, 2 / (in + out))), small non-zero biases so that the bias
    gradients are exercised, X, Y, eps ~ N(0, 1).  clip: the last encoder map's raw columns are scaled so that the raw output spreads over
    about +-60 -- rows below ln 1e-12 and rows above ln 1e10."""
    rng = np.random.RandomState(1000 + seed)
    enc, dec = widths(hidden, Dx, Dy, L)
    f = lambda a: np.asarray(a, dtype=np.float32)
    case = {"hidden": list(hidden), "Dx": Dx, "Dy": Dy, "L": L, "B": B, "variance": np.float32(variance)}
    for name, dims in (("", enc), ("_dec", dec)):
        case["Ws" + name] = [f(rng.randn(i, o) * (2.0 / (i + o)) ** 0.5) for i, o in zip(dims[:-1], dims[1:])]
        case["bs" + name] = [f(0.1 * rng.randn(o)) for o in dims[1:]]
    case["X"], case["Y"], case["eps"] = f(rng.randn(B, Dx)), f(rng.randn(B, Dy)), f(rng.randn(B, L))
    if clip:
        xy = np.concatenate([case["X"], case["Y"]], 1).astype(np.float64)
        h = xy
        for W, b in zip(case["Ws"][:-1], case["bs"][:-1]):
            h = np.tanh(h @ W + b)
        raw = h @ case["Ws"][-1][:, L:] + case["bs"][-1][L:]
        scale = 30.0 / max(raw.std(), 1e-3)
        case["Ws"][-1][:, L:] *= np.float32(scale)
        case["bs"][-1][L:] *= np.float32(scale)
    return case


# the shapes of tests/test_gpu_cvae_kernel.py: (hidden widths, Dx, Dy, L, B)
KERNEL_CASES = [([], 1, 1, 1, 1), ([], 5, 1, 1, 37), ([7], 5, 1, 1, 37), ([50], 8, 1, 1, 512), ([33, 17], 5, 3, 3, 130),
                ([100, 100], 8, 1, 1, 512), ([100, 100], 31, 1, 1, 1000), ([128, 128, 128], 120, 8, 8, 65)]
CLIP_CASE = ([7], 5, 1, 1, 37)
SAMPLER_SHAPES = [(1, 1), (3, 77), (130, 2), (3, 2000)]
# (the last net is beyond what the sampler keeps resident in LDS: it stages every map per tile)
SAMPLER_NETS = [([], 5, 1, 1), ([33, 17], 5, 3, 3), ([100, 100], 8, 1, 1), ([128, 128, 128], 120, 8, 8)]
BOUND_RTOL, GRAD_RTOL, SAMPLE_RTOL = 1e-5, 1e-4, 1e-5


def sampler_inputs(hidden, Dx, Dy, L, N, S, seed=0):
    case = make_case(hidden, Dx, Dy, L, 1, seed=seed)
    rng = np.random.RandomState(2000 + seed)
    f = lambda a: np.asarray(a, dtype=np.float32)
    return case, f(rng.randn(N, Dx)), f(rng.randn(N, S, L)), f(rng.randn(N, S, Dy))


def max_norm_err(got, ref):
    """max |got - ref| / max |ref| (the project's max-norm form, tests/test_gpu_backward.py: _close)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))
