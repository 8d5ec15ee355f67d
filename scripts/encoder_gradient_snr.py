"""Signal-to-noise ratio of the encoder's gradient under the three estimators ("iwae" | "dreg" | "stl") as the number of importance
samples K grows: a configs[2]-shaped model (L=2, M=128, B=1024, one latent-variable layer) for K in {1, 5, 20, 50}, at its initial
parameters and after a fixed number of ``Trainer`` steps under each estimator.  Every figure is ``backward.snr_summary`` of
``backward.gradient_moments`` (Welford moments over fresh device noise, accumulated on the device): per encoder tensor
``norm_snr = ||mean|| / sqrt(sum var)``, and the same over all encoder tensors together ("encoder").

A recorded measurement, not a threshold: whatever it shows is what README.md reports.
``--bound B1 B2 ...`` (models.Bound.parse: iwae | miwae:<groups> | ciwae:<beta> | vr:<alpha>) measures the bound family instead
(profiles/bound_family_snr.json): the 'iwae' estimator throughout, each bound trained for ``--steps`` and measured at the state it trained,
and each measured at the state 'iwae' trained; a bound whose groups do not divide K is skipped for that K and said so.

Usage: python scripts/encoder_gradient_snr.py [--repeats 4096] [--steps 3000] [--out profiles/encoder_grad_snr.json] [--commit HASH]
       python scripts/encoder_gradient_snr.py --bound iwae miwae:4 miwae:5 ciwae:0.5 vr:0.5 --Ks 20 50 --out profiles/bound_family_snr.json"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dgps_with_iwvi_amd import backward, settings, synthetic   # noqa: E402
from dgps_with_iwvi_amd.training import Trainer   # noqa: E402

ESTIMATORS = ("iwae", "dreg", "stl")
SHAPE = dict(L=2, M=128, B=1024, with_lv=True)


def _commit():
    try:
        return subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL, text=True).strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown (no git history here)"


def measure(model, repeats, use_graph, estimators=ESTIMATORS):
    """{estimator: {tensor or "encoder": norm_snr, ...}} at the model's current parameters (under the model's bound)."""
    out = {}
    for est in estimators:
        mom = backward.gradient_moments(model, repeats, encoder_gradient=est, use_graph=use_graph)
        enc = {n: m for n, m in mom.items() if ".enc" in n}
        snr = backward.snr_summary(enc)
        mean = torch.cat([m["mean"].reshape(-1) for m in enc.values()])
        var = torch.cat([m["var"].reshape(-1) for m in enc.values()])
        row = {n: s["norm_snr"] for n, s in snr.items()}
        row["encoder"] = float(mean.norm() / var.sum().sqrt())
        row["encoder_median_elementwise"] = float((mean.abs() / var.sqrt()).median())
        out[est] = row
    return out


def _train(model, steps, use_graph):
    """``steps`` Trainer steps -> the last step's bound (raises FloatingPointError when the run leaves the finite numbers)."""
    tr = Trainer(model, use_graph=use_graph)
    elbo = None
    for _ in range(steps):
        elbo = tr.step()
    torch.cuda.synchronize()
    return float(elbo)


def bound_rows(spec, K, bounds, a, dev, use_graph):
    """The bound family at one K -> {"trained_<bound>": {"at_own_state": ..., "bound_at_last_step": ...}, "at_iwae_state": {bound: ...}}."""
    from dgps_with_iwvi_amd.models import Bound
    rows, usable = {}, []
    for text in bounds:
        if K % Bound.parse(text).groups:
            rows["trained_" + text] = dict(skipped="groups do not divide K = %d" % K)
        else:
            usable.append(text)
    iwae_state = None
    for text in usable:
        settings.set_seed(a.noise_seed)
        model = synthetic.build_model(spec, dev)
        model.bound = text
        try:
            last = _train(model, a.steps, use_graph)
        except FloatingPointError as e:
            rows["trained_" + text] = dict(diverged=str(e))
            continue
        rows["trained_" + text] = dict(at_own_state=measure(model, a.repeats, use_graph, ("iwae",))["iwae"], bound_at_last_step=last)
        if Bound.parse(text).is_default:
            iwae_state = model
    if iwae_state is not None:                                   # every bound's gradient at the parameters 'iwae' trained
        rows["at_iwae_state"] = {}
        for text in usable:
            iwae_state.bound = text
            rows["at_iwae_state"][text] = measure(iwae_state, a.repeats, use_graph, ("iwae",))["iwae"]
        iwae_state.bound = "iwae"
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--Ks", type=int, nargs="+", default=[1, 5, 20, 50])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--noise_seed", type=int, default=1)
    ap.add_argument("--eager", action="store_true", help="no graph replay (gradient_moments and the Trainer run eagerly)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encoder_grad_snr.json"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--bound", nargs="+", default=None, help="measure these bounds (the 'iwae' estimator) instead of the three estimators")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("encoder_gradient_snr.py measures on the device: no ROCm device here")
    dev = torch.device("cuda:0")
    use_graph = not a.eager
    res = dict(what="norm_snr = ||mean|| / sqrt(sum var) of the encoder's gradient over `repeats` noise draws; rows: state of the parameters "
                    "(init, or after `steps` Trainer steps under the named estimator) -> estimator measured -> tensor",
               floor="a gradient of zero mean still measures about 1 / sqrt(repeats) = %.4f: figures near it say 'no signal seen'" % (a.repeats ** -0.5),
               shape=dict(SHAPE, Ks=a.Ks), repeats=a.repeats, steps=a.steps, spec_seed=a.seed, noise_seed=a.noise_seed, graph=use_graph,
               commit=a.commit or _commit(), box=socket.gethostname(), device=torch.cuda.get_device_name(0), torch=torch.__version__,
               results={})
    t0 = time.time()
    if a.bound:
        res["what"] = ("norm_snr = ||mean|| / sqrt(sum var) of the encoder's gradient ('iwae' estimator) over `repeats` noise draws, per bound of "
                       "the family: at the state that bound trained for `steps` Trainer steps (with the last step's value of THAT bound: "
                       "different bounds, not comparable as numbers) and at the state 'iwae' trained; ONE seed")
        res["bounds"] = list(a.bound)
    for K in a.Ks:
        spec = synthetic.make_spec(K=K, seed=a.seed, **SHAPE)
        if a.bound:
            rows = bound_rows(spec, K, a.bound, a, dev, use_graph)
            res["results"]["K=%d" % K] = rows
            for state, row in rows.items():
                if state == "at_iwae_state":
                    print("K=%-3d at the iwae-trained state: " % K + "  ".join("%s %.4g" % (b, r["encoder"]) for b, r in row.items()), flush=True)
                elif "at_own_state" in row:
                    print("K=%-3d %-20s snr %.4g  (its bound %.2f)" % (K, state, row["at_own_state"]["encoder"], row["bound_at_last_step"]), flush=True)
                else:
                    print("K=%-3d %-20s %s" % (K, state, row), flush=True)
            continue
        rows = {}
        settings.set_seed(a.noise_seed)
        rows["init"] = measure(synthetic.build_model(spec, dev), a.repeats, use_graph)
        for est in ESTIMATORS:
            settings.set_seed(a.noise_seed)
            model = synthetic.build_model(spec, dev)
            model.encoder_gradient = est
            tr = Trainer(model, use_graph=use_graph)
            elbo = None
            try:
                for _ in range(a.steps):
                    elbo = tr.step()
            except FloatingPointError as e:                      # recorded, not hidden: the run under this estimator left the finite numbers
                rows["trained_" + est] = dict(diverged=str(e))
                continue
            torch.cuda.synchronize()
            rows["trained_" + est] = dict(measure(model, a.repeats, use_graph), bound_at_last_step=float(elbo))
        res["results"]["K=%d" % K] = rows
        for state, row in rows.items():
            if "diverged" in row:
                print("K=%-3d %-13s diverged: %s" % (K, state, row["diverged"]), flush=True)
                continue
            print("K=%-3d %-13s " % (K, state) + "  ".join("%s %.4g" % (e, row[e]["encoder"]) for e in ESTIMATORS)
                  + ("  (bound %.2f)" % row["bound_at_last_step"] if "bound_at_last_step" in row else ""), flush=True)
    res["seconds"] = time.time() - t0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
