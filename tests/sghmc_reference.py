"""NumPy float64 restatement of the SGHMC mode's two formulas, written from the update rule as include/iwvi_hip.h states it
(iwvi_sghmc_step, iwvi_neg_log_prior), for the tests of csrc/sghmc.hip.

State of one sampled tensor theta: xi = 1, g = 1, g2 = 1, p = 0 (``init_state``).  One step, every right-hand side reading the values
from before it, with grad = d nll / d theta = -(d bound / d theta):

    r      = 1 / (xi + 1)
    g'     = (1 - r) g + r grad
    g2'    = (1 - r) g2 + r grad^2
    xi'    = 1 + xi (1 - g^2 / (g2 + 1e-16))
    Minv   = 1 / (sqrt(g2 + 1e-16) + 1e-16)
    eps_s  = epsilon / sqrt(num_data)
    sigma  = sqrt(max(2 eps_s^2 mdecay Minv, 1e-16))
    p'     = p - epsilon^2 Minv grad - mdecay p + sigma n,   n ~ N(0, 1)
    theta' = theta + p'

The sample op writes theta and p only, the burn-in op xi, g, g2 as well.

``step`` also returns, per updated quantity, the sum of the absolute values of the terms that enter it (``mag``): a float64 evaluation
of a recurrence of n_ops roundings is within n_ops 2^-53 mag of the exact value, whatever the order of its operations, which is what the GPU
test asserts of the device's state.
"""
import numpy as np

EPS_G2 = 1e-16
U64 = 2.0 ** -53                                                # unit round-off of float64


def init_state(theta):
    theta = np.asarray(theta, dtype=np.float64)
    return dict(theta=theta.copy(), xi=np.ones_like(theta), g=np.ones_like(theta), g2=np.ones_like(theta), p=np.zeros_like(theta))


def neg_log_prior(q_mu):
    """-log N(q_mu; 0, I) over all M R entries of a whitened q_mu."""
    q = np.asarray(q_mu, dtype=np.float64)
    return 0.5 * float(np.sum(q * q)) + 0.5 * q.size * float(np.log(2.0 * np.pi))


def step(state, grad_bound, noise, epsilon, mdecay, num_data, burn_in):
    """-> (new state, mag).  ``grad_bound`` = d bound / d theta (what the adjoints leave); ``noise`` the N(0, 1) draws."""
    s = {k: np.asarray(v, dtype=np.float64) for k, v in state.items()}
    grad = -np.asarray(grad_bound, dtype=np.float64)
    n = np.asarray(noise, dtype=np.float64)
    xi, g, g2, p, theta = s["xi"], s["g"], s["g2"], s["p"], s["theta"]
    r = 1.0 / (xi + 1.0)
    g_t = (1.0 - r) * g + r * grad
    g2_t = (1.0 - r) * g2 + r * (grad * grad)
    ratio = g * g / (g2 + EPS_G2)
    xi_t = 1.0 + xi * (1.0 - ratio)
    Minv = 1.0 / (np.sqrt(g2 + EPS_G2) + 1e-16)
    eps_s = epsilon / np.sqrt(float(num_data))
    sigma = np.sqrt(np.maximum(2.0 * (eps_s * eps_s) * mdecay * Minv, 1e-16))
    p_t = p - epsilon * epsilon * Minv * grad - mdecay * p + sigma * n
    theta_t = theta + p_t
    new = dict(theta=theta_t, p=p_t, xi=xi.copy(), g=g.copy(), g2=g2.copy())
    if burn_in:
        new.update(xi=xi_t, g=g_t, g2=g2_t)
    mag_p = np.abs(p) + np.abs(epsilon * epsilon * Minv * grad) + np.abs(mdecay * p) + np.abs(sigma * n)
    mag = dict(p=mag_p, theta=np.abs(theta) + mag_p,
               g=np.abs((1.0 - r) * g) + np.abs(r * grad), g2=np.abs((1.0 - r) * g2) + np.abs(r * grad * grad),
               xi=1.0 + np.abs(xi) + np.abs(xi * ratio))
    return new, mag
