"""tests/encoder_cases.py on the CPU: the float64 restatement against the oracle's Encoder and LatentVariableLayer, the table's claims
against its own shapes, the recorded float32 figures against what the restatement produces now, and the recorded LDS sizes against the
formulas of the kernels' host drivers (restated once, here).  No device: the forward plans come from iwvi_debug_forward_plan, which calls
no HIP function."""
import numpy as np
import pytest

import encoder_cases as ec
import philox_reference as pr
from oracle import iwvi_oracle as O


def _outputs(case, pre=None):
    inp = ec.make_inputs(case)
    return inp, ec.mlp(inp["XY"], inp["Ws"], inp["bs"], case.dims, case.act, pre)


def test_restatement_equals_the_oracle_on_the_20_20_network():
    case = ec.BY_ID["base20"]
    assert case.dims[1:-1] == (20, 20) and case.act == "tanh" and case.bias == "all"
    inp, out = _outputs(case)
    Lw = ec.latent_dim(case)
    enc = O.Encoder(Lw, case.dims[0], list(case.dims[1:-1]))
    enc.Ws = [w.astype(np.float64) for w in inp["Ws"]]
    enc.bs = [b.astype(np.float64) for b in inp["bs"]]
    mu, sg = enc(inp["XY"])
    np.testing.assert_allclose(out[:, :Lw], mu, rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.logaddexp(0.0, out[:, Lw:] - 3.0), sg, rtol=0, atol=1e-12)
    z = inp["z"][:ec.MAX_ROWS]
    for sampled in (False, True):
        ref = O.LatentVariableLayer(Lw, encoder=enc).propagate(inp["F"], inp["XY"], sampled, z=z)
        got = ec.lv_tail(out, inp["F"], z, sampled)
        for name, a, b in zip(("sample", "mean", "var", "kl"), got, ref):
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-12, err_msg=name)


def test_gradient_restatement_equals_central_differences():
    """mlp_grads is autograd of a second statement of the MLP (torch ops): pin it to ``mlp`` itself by central differences in float64."""
    for cid in ("skip_first5", "w63_64", "act_softplus_s1", "depth1_skip"):
        case = ec.BY_ID[cid]
        inp = ec.make_inputs(case)
        XY, d_out = inp["XY"][:17], inp["d_out"][:17].astype(np.float64)
        Ws = [w.astype(np.float64) for w in inp["Ws"]]
        bs = None if inp["bs"] is None else [None if b is None else b.astype(np.float64) for b in inp["bs"]]
        dW, db = ec.mlp_grads(XY, Ws, bs, case.dims, case.act, d_out)
        rng, h = np.random.default_rng(0), 1e-6
        f = lambda: float((ec.mlp(XY, Ws, bs, case.dims, case.act) * d_out).sum())
        for l in range(len(Ws)):
            for t, g in ((Ws[l], dW[l]), (None if bs is None else bs[l], db[l])):
                assert (t is None) == (g is None)
                if t is None:
                    continue
                idx = tuple(rng.integers(0, s) for s in t.shape)
                keep = t[idx]
                t[idx] = keep + h
                up = f()
                t[idx] = keep - h
                dn = f()
                t[idx] = keep
                assert abs((up - dn) / (2 * h) - g[idx]) <= 1e-6 * max(1.0, np.abs(g).max()), (cid, l, idx)


def test_ids_are_unique_and_every_edge_is_claimed():
    ids = [c.id for c in ec.CASES] + [p["id"] for p in ec.PAIRS]
    assert len(set(ids)) == len(ids)
    claimed = {e for c in ec.CASES for e in c.edges} | {e for p in ec.PAIRS for e in p["edges"]}
    assert claimed == set(ec.EDGES), (claimed ^ set(ec.EDGES))
    assert ec.A_ROWS == (1, 17, 100) and ec.C_ROWS == (255, 256, 257, 513) and (ec.B_POINTS, ec.B_SAMPLES) == (3, 7)
    assert set(ec.LDS) == set(ec.ERR32) == {c.id for c in ec.CASES}


# what a claim means in terms of the case's own fields
def _skips(c):
    return [l for l, (a, b) in enumerate(zip(c.dims[:-1], c.dims[1:])) if a == b]


_CLAIMS = {
    "depth-1": lambda c: len(c.dims) == 2,
    "depth-1-skip": lambda c: len(c.dims) == 2 and c.dims[0] == c.dims[1],
    "depth-max": lambda c: len(c.dims) - 1 == ec.MAX_ENC,
    "width-1": lambda c: 1 in c.dims[1:-1],
    "width-odd": lambda c: any(d % 2 for d in c.dims[1:-1]),
    "width-63": lambda c: 63 in c.dims,
    "width-64": lambda c: 64 in c.dims,
    "out-62": lambda c: c.dims[-1] == 62,
    "skip-first-unaligned": lambda c: len(c.dims) > 2 and c.dims[0] == c.dims[1] and c.dims[0] % 4 != 0,
    "skip-first-aligned": lambda c: len(c.dims) > 2 and c.dims[0] == c.dims[1] and c.dims[0] % 4 == 0,
    "skip-middle": lambda c: any(0 < l < len(c.dims) - 2 for l in _skips(c)),
    "skip-last": lambda c: len(c.dims) - 2 in _skips(c),
    "skip-none": lambda c: not _skips(c),
    "bias-none": lambda c: c.bias == "none",
    "bias-some": lambda c: c.bias == "some",
    "Dx+Lw-cap": lambda c: ec.layer_width(c) + ec.latent_dim(c) == ec.MAX_D,
    "two-encoders": lambda c: False,
    "beyond-C-3x64": lambda c: c.dims == (64, 64, 64, 2) and not ec.LDS[c.id][2],
    "beyond-C-full": lambda c: c.dims == (64,) * ec.MAX_ENC + (2,) and not ec.LDS[c.id][2],
}
_CLAIMS.update({"act-" + a: (lambda c, a=a: c.act == a and c.scale == 1.0 and len(c.dims) > 2) for a in ec.ACTS})
_CLAIMS.update({"Lw-%d" % n: (lambda c, n=n: ec.latent_dim(c) == n) for n in (1, 3, 4, 5)})
_CLAIMS.update({"K-%d" % n: (lambda c, n=n: c.K == n) for n in (1, 3)})
_CLAIMS.update({"skl-%d" % n: (lambda c, n=n: c.sampled_kl == n) for n in (0, 1)})


@pytest.mark.parametrize("case", ec.CASES, ids=lambda c: c.id)
def test_a_case_is_what_it_claims(case):
    assert all(1 <= d <= ec.MAX_WIDTH for d in case.dims) and 1 <= len(case.dims) - 1 <= ec.MAX_ENC
    assert ec.layer_width(case) + ec.latent_dim(case) <= ec.MAX_D
    pre = []
    inp, out = _outputs(case, pre)
    raw3 = out[:, ec.latent_dim(case):] - 3.0
    assert raw3.min() > ec.RAW_FLOOR, raw3.min()                 # the regulariser stays finite: the scope of the table
    hidden = np.concatenate([p.ravel() for p in pre]) if pre else np.zeros(0)
    for e in case.edges:
        if e in _CLAIMS:
            assert _CLAIMS[e](case), e
        elif e.startswith("sat-"):
            assert case.act == e[4:] and (hidden > ec.SAT).any() and (hidden < -ec.SAT).any(), e
        elif e == "relu-margin":
            pass                                                 # (below: it holds for EVERY relu case, claimed or not)
        elif e == "softplus-log-range":
            for rows in (ec.A_ROWS[-1],) + ec.C_ROWS:            # every row count that sees 100 rows or more walks the whole ramp
                r = raw3[:rows]
                assert -80.5 <= r.min() <= -79.5 and 19.5 <= r.max() <= 20.5 and (r > 20.0 - 3.0).any(), (rows, r.min(), r.max())
            sg = np.logaddexp(0.0, raw3)
            assert 1e-36 < sg.min() < 1e-34
        else:
            assert e == "oracle-pin", e
    if case.act == "relu":
        assert "relu-margin" in case.edges and np.abs(hidden).min() > ec.RELU_MARGIN, np.abs(hidden).min()


def test_pairs_share_one_launch_with_a_ragged_first_encoder():
    for p in ec.PAIRS:
        (a, ra), (b, rb) = p["first"], p["second"]
        ca, cb = ec.BY_ID[a], ec.BY_ID[b]
        assert ca.dims != cb.dims and ca.act != cb.act and ra != rb
        assert ra % 256 != 0 and (ra + 255) // 256 == 2          # the second encoder starts at blk0 = 2
        assert ec.LDS[a][2] and ec.LDS[b][2]


@pytest.mark.parametrize("case", ec.CASES, ids=lambda c: c.id)
def test_recorded_float32_error_is_what_the_restatement_gives(case):
    now, rec = ec.measure_err32(case), ec.ERR32[case.id]
    assert set(now) == set(rec)
    for k in now:
        assert np.isfinite(now[k]) and now[k] > 0.0, (k, now[k])
        assert abs(now[k] - rec[k]) <= 1e-3 * rec[k], (k, now[k], rec[k])      # (recorded with four digits)


def test_recorded_lds_sizes_follow_the_drivers():
    for c in ec.CASES:
        w = sum(a * b + b for a, b in zip(c.dims[:-1], c.dims[1:]))
        need_c = (w + 4 + 2 * 256 * 65) * 4                      # csrc/precompute.hip, iwvi_model_precompute: weights + two activation buffers
        need_d = ((len(c.dims) - 1 + 5) * 4 * 65 + w) * 4        # csrc/backward.hip, enc_bwd_impl: (n + 5) row tiles of ER x ELD + the weights
        rc, rd, fits = ec.LDS[c.id]
        assert (rc, rd) == (need_c, need_d), c.id
        assert fits == (need_c <= 160 * 1024), c.id
        assert need_d <= 160 * 1024                              # site D takes every admitted encoder
        assert ec.expect(c.id, "C") == ("evaluate" if fits else "refuse")
        assert all(ec.expect(c.id, s) == "evaluate" for s in "ABD")
    assert (7676 + 4 + 2 * 256 * 65) * 4 == 160 * 1024           # the largest weight count site C takes
    assert {c.id for c in ec.CASES if not ec.LDS[c.id][2]} == set(ec.AB_PLAN) == {"over_3x64", "over_full"}


def test_the_layer_kernel_plans_the_encoders_beyond_site_c():
    for cid, (a_bytes, b_bytes) in ec.AB_PLAN.items():
        case = ec.BY_ID[cid]
        rc, plan = ec.lv_plan(case, ec.A_ROWS[-1], 1, ec.A_ROWS[-1])
        assert rc == 0 and plan[2] == a_bytes <= ec.LDS_LIMIT, (cid, rc, plan)
        rc, plan = ec.lv_plan(case, ec.B_POINTS * ec.B_SAMPLES, ec.B_SAMPLES, ec.B_POINTS)
        assert rc == 0 and plan[2] == b_bytes <= ec.LDS_LIMIT, (cid, rc, plan)


def test_layer_stream_restatement_shares_the_pinned_philox_core():
    """``philox_reference.layer_normal`` (the stream site C's sampling tail and the layer kernel draw from) is the counter layout of
    draw_normal4 over the Philox core and Box-Muller that tests/test_philox_reference_host.py pins.  Layer 0, quad 0, step 0 is the
    counter (t, 0, 0, 0): the stand-alone fill's block t, so the two restatements must give the same four numbers there."""
    seed = (7 << 32) | 12345
    for t in (0, 5, 2 ** 32 + 3):
        a = pr.layer_normal(seed, 0, 0, [t], 4)[0]
        b = pr.fill_normal(4, seed, t)
        assert np.array_equal(a, b), t
    full = pr.layer_normal(seed, 5, 0, np.arange(40), 8)
    assert np.array_equal(pr.layer_normal(seed, 5, 0, np.arange(40), 5), full[:, :5])      # a cut quad is the whole quad's head
    assert np.array_equal(pr.layer_normal(seed, 5, 0, np.arange(40), 3), full[:, :3])
    others = [pr.layer_normal(seed, 6, 0, np.arange(40), 8), pr.layer_normal(seed, 5, 1, np.arange(40), 8),
              pr.layer_normal(seed + 1, 5, 0, np.arange(40), 8), pr.layer_normal(seed, 5 + 2 ** 32, 0, np.arange(40), 8)]
    for o in others:                                             # step, layer, key and the step's high half all move the stream
        assert np.abs(o - full).max() > 0.5
    assert not np.array_equal(full[:, :4], full[:, 4:])          # the second quad is a block of its own
