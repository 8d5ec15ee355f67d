"""tests/adjoint_reference.py on the host: the reference restricted to live rows is the full reference with the other cotangents zeroed,
its dW / dmf_A agree with central differences, and -- the condition that keeps the GPU tests from hiding a fault -- every workgroup of
every layer-adjoint case with T > 512 holds a live row whose loss alone would break the GPU tolerance.

Visibility is sampled: every fourth live row of a case, plus the first live row of every workgroup span that would otherwise hold no
sampled row (a single-row gradient costs 2 - 10 ms; all ~21 000 live rows of the table would take over a minute).  A span whose
sampled rows are all too faint has its other live rows tried before it counts as blind."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adjoint_reference as ar   # noqa: E402

VISIBLE = ar.RTOL           # a row counts as visible when its solo gradient reaches the GPU tolerance in some parameter array
MAX_FAINT = 0.02            # at most this share of the sampled live rows may stay below it


def _small(li):
    from dgps_with_iwvi_amd import synthetic
    spec = synthetic.make_spec(L=2, M=32, B=8, K=2, Dx=6, R=3, Dy=2, mixing="dense", seed=11)
    return spec, ar.layer_inputs(spec, li, 96, seed=96 + li)


def test_live_rows_cover_every_tile_and_every_lane():
    for T in (16, 40, 96, 1541, 8192, 16400, 20480, 20496):
        rows = ar.live_rows(T)
        assert np.all(np.diff(rows) > 0) and rows[0] == 0 and rows[-1] == T - 1
        assert set(range(min(T, 16))) <= set(rows) and set(range(T // 16 * 16 - 16 if T >= 16 else 0, T)) <= set(rows)
        tiles = np.unique(rows // 16)
        assert len(tiles) == (T + 15) // 16                                   # a live row in every 16-row tile, the ragged one included
        if T >= 16 * 18:
            inner = rows[(rows >= 16) & (rows < T // 16 * 16 - 16)]
            assert len(inner) == T // 16 - 2 and np.array_equal(inner % 16, (inner // 16) % 16)
            assert set(inner[:64] % 16) == set(range(16))                     # the live lane walks through all 16 positions
    assert len(ar.live_rows(20480)) == 1310


@pytest.mark.parametrize("li", [0, 1])
def test_restricted_reference_equals_the_zeroed_full_reference(li):
    spec, (F, z, cs, cm, cv) = _small(li)
    rows = ar.live_rows(96)
    assert 16 < len(rows) < 96
    got = ar.layer_reference(spec, li, F, z, cs, cm, cv, ar.KL_WEIGHT, rows)
    ar.mask_rows(rows, cs, cm, cv)
    full = ar.layer_reference(spec, li, F, z, cs, cm, cv, ar.KL_WEIGHT)
    assert sorted(got) == sorted(full) == sorted(["F", "Z", "ls", "var", "q_mu", "q_sqrt"] + (["W", "A"] if li == 0 else []))
    dead = np.setdiff1d(np.arange(96), rows)
    assert np.abs(full["F"][dead]).max() == 0.0
    full["F"] = full["F"][rows]
    for k in got:
        assert got[k].shape == full[k].shape, k
        assert np.abs(got[k] - full[k]).max() <= 1e-12 * np.abs(full[k]).max(), k
    assert np.abs(np.triu(got["q_sqrt"], 1)).max() == 0.0


def test_dW_and_dmf_A_agree_with_central_differences():
    """Every entry of dW [P, R] and dmf_A [D, P] against (f(x + h) - f(x - h)) / 2h of the float64 objective, h = 1e-6, to 1e-6 of the
    array's max-norm (truncation ~h^2, rounding ~1e-16 |f| / h ~ 1e-8)."""
    li = 0
    spec, (F, z, cs, cm, cv) = _small(li)
    rows = ar.live_rows(96)
    g = ar.layer_reference(spec, li, F, z, cs, cm, cv, ar.KL_WEIGHT, rows)
    L = spec["layers"][li]
    h = 1e-6
    for name, base in (("W", np.asarray(L["W"], dtype=np.float64)), ("A", np.asarray(L["mf"][1], dtype=np.float64))):
        assert g[name].shape == base.shape
        fd = np.zeros_like(base)
        for idx in np.ndindex(*base.shape):
            v = []
            for sgn in (1.0, -1.0):
                x = base.copy()
                x[idx] += sgn * h
                v.append(float(ar.layer_objective(spec, li, F, z, cs, cm, cv, ar.KL_WEIGHT, rows, override={name: x}, grad=False)[0]))
            fd[idx] = (v[0] - v[1]) / (2 * h)
        assert np.abs(fd - g[name]).max() <= 1e-6 * np.abs(g[name]).max(), (name, np.abs(fd - g[name]).max(), np.abs(g[name]).max())


# ------------------------------------------------------------------------------------------------------------------------------------
# visibility: every distinct (spec, seed, T) of the GPU cases
# ------------------------------------------------------------------------------------------------------------------------------------
def _matern_case_of_test_gpu_backward():
    """test_gpu_backward.py::test_matern52_layer_backward_matches_autodiff at T = 16384: its own spec, seed and kl_weight."""
    from dgps_with_iwvi_amd import synthetic
    M, T, li = 64, 16384, 0
    spec = synthetic.make_spec(L=2, M=M, B=8, K=2, with_lv=False, seed=3 * M + li)
    return spec, li, T, ar.layer_inputs(spec, li, T, seed=T), 1.0, "matern52", ar.live_rows(T), 64


def _table_case(c, span):
    spec = ar.case_spec(c)
    return spec, c.li, c.T, ar.case_inputs(c, spec), ar.KL_WEIGHT, c.kern, ar.case_rows(c), span


def _visibility_cases():
    out = {}
    for c in ar.CASES:                                                        # (the flag pairs and the forced / unforced pair share inputs)
        key = (c.M, c.Dx, c.R, c.li, c.T, c.kern)
        span = min(c.route[2], out[key][1]) if key in out else c.route[2]
        out[key] = (c, span)
    cases = [pytest.param(lambda c=c, span=span: _table_case(c, span), id=c.id)
             for c, span in out.values()]
    return cases + [pytest.param(_matern_case_of_test_gpu_backward, id="test_gpu_backward-matern52-16384")]


@pytest.mark.parametrize("make", _visibility_cases())
def test_every_workgroup_holds_a_visible_live_row(make):
    spec, li, T, (F, z, cs, cm, cv), klw, kern, rows, span = make()
    full = ar.layer_reference(spec, li, F, z, cs, cm, cv, klw, rows, kern)
    group = rows // span                                                      # the workgroup (or 16-row tile) of each live row
    nspan = (T + span - 1) // span
    assert len(np.unique(group)) == nspan
    pick = np.zeros(len(rows), dtype=bool)
    pick[::4] = True
    covered = np.zeros(nspan, dtype=bool)
    covered[group[pick]] = True
    first = np.unique(group, return_index=True)[1]
    pick[first[~covered]] = True

    def visible(sel):
        names, solo = ar.solo_norms(spec, li, F, z, cs, cm, cv, rows[sel], kern)
        scale = np.array([np.abs(full[k]).max() for k in names])
        return (solo / scale).max(1) >= VISIBLE
    sel = np.flatnonzero(pick)
    vis = visible(sel)
    seen = np.zeros(nspan, dtype=bool)
    seen[group[sel[vis]]] = True
    for g in np.flatnonzero(~seen):                                           # (nothing on the rows sampled here)
        rest = np.flatnonzero((group == g) & ~pick)
        seen[g] = len(rest) > 0 and bool(visible(rest).any())
    assert seen.all(), "workgroups without a visible live row: %s" % np.flatnonzero(~seen)[:10]
    assert (~vis).sum() <= MAX_FAINT * len(sel), "%d of %d sampled live rows below %.0e" % ((~vis).sum(), len(sel), VISIBLE)
