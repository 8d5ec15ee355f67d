"""make_spec's opt-in knobs for wide shapes (CPU): the defaults stay byte-identical (bench.py, the goldens and every suite build on them),
mixing="dense" reaches every latent GP, distinct_y gives Dy different output functions, and neither moves anything else of the spec."""
import hashlib

import numpy as np
import pytest

from dgps_with_iwvi_amd import synthetic


def _digest(spec):
    h = hashlib.sha256()

    def add(x):
        if isinstance(x, dict):
            for k in sorted(x):
                h.update(k.encode()); add(x[k])
        elif isinstance(x, (list, tuple)):
            for v in x:
                add(v)
        elif isinstance(x, np.ndarray):
            h.update(str(x.shape).encode()); h.update(np.ascontiguousarray(x).tobytes())
        else:
            h.update(repr(x).encode())
    add(spec)
    return h.hexdigest()[:16]


@pytest.mark.parametrize("kw,digest", [
    (dict(), "8346eca793298a1b"),
    (dict(L=3, M=40, B=16, K=3, Dx=5, Dy=3, R=7, with_lv=True, seed=4, latent_dim=2), "4f5aeec3da96681b"),
    (dict(L=2, M=32, B=8, K=2, Dx=3, R=2, parity=False, seed=9), "35bbfbaaaeab5264")])
def test_default_specs_are_unchanged(kw, digest):
    assert _digest(synthetic.make_spec(**kw)) == digest


def test_dense_mixing_and_distinct_outputs():
    kw = dict(L=3, M=24, B=40, K=2, Dx=4, R=9, Dy=5, with_lv=True, seed=3)
    base = synthetic.make_spec(**kw)
    wide = synthetic.make_spec(mixing="dense", distinct_y=True, **kw)
    for lb, lw in zip(base["layers"], wide["layers"]):
        for k in ("Z", "q_mu", "q_sqrt"):
            if k in lb:
                np.testing.assert_array_equal(lb[k], lw[k])
        if lb.get("W") is not None:
            assert (lb["W"][:, kw["Dx"]:] == 0).all()          # the reference's mixing: latent GPs r >= Dx never reach the output
            assert (lw["W"] != 0).all() and lw["W"].shape == lb["W"].shape
    np.testing.assert_array_equal(base["X"], wide["X"])
    Y = wide["Y"]
    assert Y.shape == (40, 5) and all(not np.allclose(Y[:, 0], Y[:, j]) for j in range(1, 5))
    assert all(np.allclose(base["Y"][:, 0], base["Y"][:, j]) for j in range(1, 5))
    with pytest.raises(ValueError):
        synthetic.make_spec(mixing="full")
