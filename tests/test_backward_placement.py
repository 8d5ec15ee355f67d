"""Where the reverse sweep queues each layer's parameter branch (backward.branch_placement) and the one reader of the two route
switches (settings.backward_routes): host logic, no GPU.  The placement changes no bit of any gradient -- the bit-identity tests cannot
see it -- only the time of an evaluation, so this table is all that pins the policy."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stack(kinds, Ms):
    """Layers of CPU-built models, bottom to top: ``kinds`` 'LV' / 'GP', ``Ms`` the inducing points of each GP layer in turn."""
    from dgps_with_iwvi_amd import synthetic
    from dgps_with_iwvi_amd.layers import GPLayer, LatentVariableLayer
    lv, n_gp = kinds[0] == "LV", kinds.count("GP")
    built = {M: synthetic.build_model(synthetic.make_spec(L=n_gp, M=M, B=4, K=2, with_lv=lv, seed=0), torch.device("cpu")).layers
             for M in set(Ms)}
    Ms = ([None] if lv else []) + list(Ms)
    layers = [built[M if M is not None else Ms[1]][i] for i, M in enumerate(Ms)]
    assert [type(l) for l in layers] == [LatentVariableLayer if k == "LV" else GPLayer for k in kinds]
    assert [l.num_inducing for l in layers if isinstance(l, GPLayer)] == [M for M in Ms if M is not None]
    return layers


# layer kinds bottom to top, M of each GP layer, overlap, branch order -> (finished on the caller's stream, split in two); -1 = none
TABLE = [
    (("GP",), (16,), True, "default", (-1, -1)),
    (("GP",), (128,), True, "default", (-1, -1)),
    (("LV", "GP"), (16,), True, "default", (-1, 1)),
    (("LV", "GP"), (256,), True, "default", (-1, 1)),
    (("LV", "GP", "GP"), (128, 128), True, "default", (2, -1)),
    (("LV", "GP", "GP"), (128, 256), True, "default", (-1, 1)),
    (("GP", "GP", "GP"), (64, 64, 64), True, "default", (2, -1)),
    (("GP",) * 5, (128,) * 5, True, "default", (2, -1)),
    (("LV", "GP", "GP"), (128, 128), True, "old", (-1, 1)),
    (("LV", "GP", "GP"), (128, 128), False, "default", (-1, -1)),
]


@pytest.mark.parametrize("kinds,Ms,overlap,order,expected", TABLE)
def test_branch_placement_table(kinds, Ms, overlap, order, expected):
    from dgps_with_iwvi_amd import backward
    assert backward.branch_placement(_stack(kinds, Ms), overlap, order) == expected


def test_route_switches_are_read_when_called(monkeypatch):
    """Tests and scripts set the two variables between evaluations: the reader looks at the environment at every call, and anything but
    the two development values is the default route."""
    from dgps_with_iwvi_amd import settings
    monkeypatch.delenv("IWVI_BW_PREPARE", raising=False)
    monkeypatch.delenv("IWVI_BW_BRANCH_ORDER", raising=False)
    assert settings.backward_routes() == ("side", "default")
    monkeypatch.setenv("IWVI_BW_PREPARE", "inline")
    assert settings.backward_routes() == ("inline", "default")
    monkeypatch.setenv("IWVI_BW_BRANCH_ORDER", "old")
    assert settings.backward_routes() == ("inline", "old")
    monkeypatch.setenv("IWVI_BW_PREPARE", "side")
    monkeypatch.delenv("IWVI_BW_BRANCH_ORDER")
    assert settings.backward_routes() == ("side", "default")

