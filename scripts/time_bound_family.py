"""Time of one value + gradient evaluation and of one training step (both as hipGraph replays, scripts/time_backward.py) under the members of
the bound family, and -- with ``--parent DIR``, a built checkout of the parent commit -- of the default bound on both trees, alternated in
one call: every figure is one fresh process of scripts/time_backward.py, the rounds interleave parent, this tree and the other bounds, and
the spread of a series is what the same tree gives from round to round.

A recorded measurement: the default route launches what it launched, so its two series should overlap; the other members give up the fused
heads (backward._saving_forward: two launches) and their cost over the default is reported, not bounded.
Usage: python scripts/time_bound_family.py [--parent DIR] [--rounds 3] [--iters 100] [--out profiles/bound_family_time.json]"""
import argparse
import json
import os
import socket
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = ("miwae:4", "miwae:5", "ciwae:0.5", "vr:0.5")


def one(tree, iters, config, bound=None, limit=300):
    """One process of ``tree``'s scripts/time_backward.py -> its JSON figures (None when it failed; the caller stops there)."""
    with tempfile.NamedTemporaryFile(suffix=".json", delete=False) as f:
        path = f.name
    cmd = [sys.executable, os.path.join(tree, "scripts", "time_backward.py"), "--config", str(config), "--iters", str(iters), "--json", path]
    if bound:
        cmd += ["--bound", bound]
    r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        print(r.stdout[-2000:], r.stderr[-2000:], flush=True)
        return None
    with open(path) as f:
        out = json.load(f)
    os.unlink(path)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (its scripts/time_backward.py is run from there)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bound_family_time.json"))
    a = ap.parse_args()
    keys = ("value_gradient_graph_ms", "step_graph_ms")
    series = {}
    if a.parent:
        a.parent = os.path.abspath(a.parent)
    order = ([("parent iwae", a.parent, None)] if a.parent else []) + [("iwae", ROOT, None)] + [(b, ROOT, b) for b in BOUNDS]
    for r in range(a.rounds):
        for name, tree, bound in order:
            got = one(tree, a.iters, a.config, bound)
            if got is None:
                raise SystemExit("%s failed in round %d: stopping" % (name, r))
            series.setdefault(name, []).append({k: got[k] for k in keys})
            print("round %d %-12s " % (r, name) + "  ".join("%s %.4f" % (k, got[k]) for k in keys), flush=True)
    res = dict(what="ms per value + gradient evaluation and per training step (NatGrad op + Adam op) at configs[%d], both as hipGraph replays, %d "
                    "replays per figure after warm-up, device synchronised around the timed loop; one fresh process per figure, %d rounds "
                    "interleaving the series" % (a.config, a.iters, a.rounds),
               box=socket.gethostname(), rounds=a.rounds, iters=a.iters, config=a.config, series=series, summary={})
    for name, rows in series.items():
        res["summary"][name] = {k: dict(min=min(x[k] for x in rows), max=max(x[k] for x in rows), median=sorted(x[k] for x in rows)[len(rows) // 2])
                                for k in keys}
    if a.parent:
        p, c = res["summary"]["parent iwae"], res["summary"]["iwae"]
        res["default_route_inside_the_spread"] = {k: bool(c[k]["min"] <= p[k]["max"] and p[k]["min"] <= c[k]["max"]) for k in keys}
    else:
        res["parent"] = "not measured"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
