"""``evaluation.evaluate_scores`` on tiny models: the draws of every batch are captured by wrapping the model's sampling method (and the PIT
values, which may be randomized, by wrapping ``evaluation.pit_values``), and every reported entry is recomputed from the captured tensors
with the float64 restatement (tests/scoring_reference.py) and compared within the kernels' own bounds (tests/test_gpu_sample_scores.py, tests/test_gpu_energy_score.py); a mean of <= 7 float64 values adds nothing.

Models: M = 16, 64 training points, one latent-variable layer and one GP layer -- Gaussian with one and with two target columns, Poisson --
and a ``cvae.CVAE`` without hidden layers.  7 test points, S = 64, batches of 4: two batches, the second ragged."""
import types

import numpy as np
import pytest
import torch

import scoring_reference as SR

pytestmark = pytest.mark.gpu

N_TEST, S, BATCH = 7, 64, 4
PROBS = (0.05, 0.25, 0.5, 0.75, 0.95)
BINS = 10
EPS = 2.0 ** -23


def _model(kind, dev):
    from dgps_with_iwvi_amd import likelihoods, synthetic
    if kind == "cvae":
        from dgps_with_iwvi_amd.build_models import build_cvae_model
        rng = np.random.RandomState(0)
        x = rng.uniform(-3.0, 3.0, (64 + N_TEST, 1)).astype(np.float32)
        y = (np.where(rng.rand(64 + N_TEST, 1) < 0.5, 1.0, -1.0) * np.sin(x) + 0.1 * rng.randn(64 + N_TEST, 1)).astype(np.float32)
        np.random.seed(5)                                                # the initial weights come from the host generator
        ARGS = types.SimpleNamespace(mode="CVAE", configuration="", minibatch_size=32, lr=5e-3, use_graph=False)
        return build_cvae_model(ARGS, x[:64], y[:64], device=dev), x[64:], y[64:]
    Dy = 2 if kind == "gaussian2" else 1
    spec = synthetic.make_spec(L=1, M=16, B=16, K=2, Dx=3, Dy=Dy, with_lv=True, seed=21, n_data=64 + N_TEST, distinct_y=True)
    lik = None
    Y = spec["Y"]
    if kind == "poisson":
        lik = likelihoods.Poisson(binsize=1.5)
        Y = np.floor(np.abs(Y) * 3.0)
        spec["Y"] = Y
    Xt, Yt = spec["X"][64:], np.asarray(Y[64:], dtype=np.float32)
    spec["X"], spec["Y"], spec["n_data"] = spec["X"][:64], spec["Y"][:64], 64
    return synthetic.build_model(spec, dev, likelihood=lik), Xt, Yt


def _capture(monkeypatch, owner, name):
    """Wrap ``owner.<name>`` so that every tensor it returns is kept."""
    kept, real = [], getattr(owner, name)

    def wrapped(*a, **k):
        out = real(*a, **k)
        kept.append(out.detach().clone())
        return out
    monkeypatch.setattr(owner, name, wrapped)
    return kept


@pytest.mark.parametrize("kind", ["gaussian1", "gaussian2", "poisson", "cvae"])
def test_every_entry_is_the_restatement_of_the_captured_draws(gpu_device, monkeypatch, kind):
    from dgps_with_iwvi_amd import evaluation
    model, Xt, Yt = _model(kind, gpu_device)
    Dt = Yt.shape[1]
    kept = _capture(monkeypatch, model, "predict_y_samples" if kind == "cvae" else "predict_y_draws")
    pits = _capture(monkeypatch, evaluation, "pit_values")
    res = evaluation.evaluate_scores(model, Xt, Yt, num_predict_samples=S, predict_batch_size=BATCH, quantiles=PROBS, pit_bins=BINS)
    assert [tuple(t.shape) for t in kept] == [(S, 4, Dt), (S, 3, Dt)]    # one sampling call per batch, the second batch ragged
    assert [tuple(t.shape) for t in pits] == [(N_TEST,)] * Dt            # one PIT per column, over all the test points
    draws = torch.cat(kept, 1).cpu().numpy()                              # [S, 7, Dt] float32
    keys = {"test_crps", "test_crps_fair", "test_pinball", "test_pit_hist", "test_calibration_error"}
    if Dt > 1:
        keys |= {"test_energy_score", "test_energy_score_fair"}
    assert set(res) == keys                                              # Dt = 1: no energy entry
    col = (lambda v, d: v) if Dt == 1 else (lambda v, d: v[d])
    if Dt > 1:
        assert all(isinstance(res[k], list) and len(res[k]) == Dt for k in ("test_crps", "test_crps_fair", "test_pinball", "test_pit_hist",
                                                                            "test_calibration_error"))
    for d in range(Dt):
        x, y = draws[:, :, d], Yt[:, d]
        ref = SR.crps(x, y)
        bound = (EPS * (ref["A"] + ref["G_over_S2"])).mean()
        assert abs(col(res["test_crps"], d) - ref["crps"].mean()) <= bound
        assert abs(col(res["test_crps_fair"], d) - ref["crps_fair"].mean()) <= bound
        pin, absd = SR.pinball(x, y, PROBS)
        got = np.asarray(col(res["test_pinball"], d))
        assert got.shape == (len(PROBS),) and np.all(np.abs(got - pin.mean(0)) <= EPS * absd.mean(0))
        below, equal = SR.counts(x, y)
        pit = pits[d].cpu().numpy()
        if kind == "poisson":                                            # randomized by default: inside the tie, each point
            assert np.all(pit >= below / (S + 1.0)) and np.all(pit <= (below + equal + 1.0) / (S + 1.0))
            assert equal.max() > 0                                       # (counts do tie with their draws: the case is exercised)
        else:                                                            # the mid-rank
            np.testing.assert_allclose(pit, SR.pit_midrank(below, equal, S), rtol=0, atol=1e-15)
        assert list(col(res["test_pit_hist"], d)) == SR.pit_hist(pit, BINS).tolist() and sum(col(res["test_pit_hist"], d)) == N_TEST
        assert col(res["test_calibration_error"], d) == pytest.approx(SR.calibration_error(pit), abs=1e-14)
    if Dt > 1:
        ref = SR.energy(draws, Yt)
        bound = ((Dt + 6) * 2.0 ** -24 * (ref["A"] + ref["B_over_S2"])).mean()
        assert abs(res["test_energy_score"] - ref["energy"].mean()) <= bound
        assert abs(res["test_energy_score_fair"] - ref["energy_fair"].mean()) <= bound
    assert all(np.all(np.isfinite(np.asarray(v, dtype=np.float64))) for v in res.values())


def test_the_pit_rule_follows_the_likelihood_unless_told(gpu_device, monkeypatch):
    from dgps_with_iwvi_amd import evaluation
    model, Xt, Yt = _model("poisson", gpu_device)
    kept = _capture(monkeypatch, model, "predict_y_draws")
    pits = _capture(monkeypatch, evaluation, "pit_values")
    evaluation.evaluate_scores(model, Xt, Yt, num_predict_samples=S, predict_batch_size=BATCH, randomized_pit=False)
    below, equal = SR.counts(torch.cat(kept, 1).cpu().numpy()[:, :, 0], Yt[:, 0])
    np.testing.assert_allclose(pits[0].cpu().numpy(), SR.pit_midrank(below, equal, S), rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        evaluation.evaluate_scores(model, Xt, Yt[:, :0], num_predict_samples=S)
    with pytest.raises(ValueError):
        evaluation.evaluate_scores(model, Xt, Yt, num_predict_samples=1)
    with pytest.raises(ValueError):
        evaluation.evaluate_scores(model, Xt, Yt, num_predict_samples=S, quantiles=[1.5])
