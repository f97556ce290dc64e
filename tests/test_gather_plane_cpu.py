"""``EngineConfig.gather_plane`` off the GPU: the validator, the default, the engines that accept the
field and behave as before (torch engine, torch ``ClientGroup``), the refusal of more than 8 ranks, and
the ``--gather-plane`` flag of the [C] entry point."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fedmi.fl.engine import GATHER_PLANES, EngineConfig, HipRoundEngine, TorchRoundEngine, gather_plane_id
from fedmi.fl.simulate import ClientGroup, SimRank
from fedmi.models.mlp import init_flat

from .reference_oracle import DATA_SEED, make_multiclass

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = [17, 24, 3]


def test_validator_and_default():
    assert EngineConfig().gather_plane == "host" and GATHER_PLANES == ("host", "xgmi")
    assert gather_plane_id(EngineConfig()) == 0
    assert gather_plane_id(EngineConfig(gather_plane="host")) == 0
    assert gather_plane_id(EngineConfig(gather_plane="xgmi")) == 1
    for bad in ("XGMI", "rccl", "", None, 1, True):
        with pytest.raises(ValueError, match="gather_plane"):
            gather_plane_id(EngineConfig(gather_plane=bad))
    assert EngineConfig(gather_plane="xgmi").to_dict()["gather_plane"] == "xgmi"


def _cfg(**kw):
    return EngineConfig(**{**dict(hidden=(24,), max_rounds=4, early_stop=False), **kw})


def test_torch_engine_ignores_the_plane():
    X, y = make_multiclass(240, 17, 3, DATA_SEED)
    flat = init_flat(DIMS, 1)
    runs = []
    for plane in GATHER_PLANES:
        e = TorchRoundEngine(X, y, 3, _cfg(aggregator="median", gather_plane=plane), None, flat)
        e.run(3)
        runs.append((e.global_flat(), e.history()))
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    for key in ("global", "loss", "per_rank"):
        np.testing.assert_array_equal(runs[0][1][key], runs[1][1][key])
    with pytest.raises(ValueError, match="gather_plane"):
        TorchRoundEngine(X, y, 3, _cfg(gather_plane="pcie"), None, flat)


@pytest.mark.parametrize("kw", [dict(aggregator="median"), dict(secagg=True, secagg_seed=3)], ids=["median", "secagg"])
def test_torch_group_ignores_the_plane(kw):
    X, y = make_multiclass(240, 17, 3, DATA_SEED)
    runs = []
    for plane in GATHER_PLANES:
        g = ClientGroup(X, y, 3, _cfg(gather_plane=plane, **kw), backend="torch", shard_mode="iid", seed=2)
        g.run(3)
        runs.append((g.global_flat(), g.history()))
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    for key in ("global", "loss", "per_rank"):
        np.testing.assert_array_equal(runs[0][1][key], runs[1][1][key])


def test_more_than_eight_ranks_are_refused():
    """Decided before anything touches a device: a SimRank of 9 on the xgmi plane."""
    X, y = make_multiclass(90, 17, 3, DATA_SEED)
    flat = init_flat(DIMS, 1)
    for kw in (dict(aggregator="median"), dict(aggregator="trimmed_mean"), dict(secagg=True, secagg_seed=3)):
        with pytest.raises(ValueError, match="gather_plane='xgmi' takes at most 8 ranks"):
            HipRoundEngine(X, y, 3, _cfg(gather_plane="xgmi", **kw), SimRank(9, 0, "cpu"), flat, n_total=9 * len(X),
                           client_sizes=[len(X)] * 9)
    # the torch engine of the same federation does not read the field
    TorchRoundEngine(X, y, 3, _cfg(gather_plane="xgmi", aggregator="median"), SimRank(9, 0, "cpu"), flat,
                     n_total=9 * len(X), client_sizes=[len(X)] * 9)


def test_entry_point_flag():
    sys.path.insert(0, ROOT)
    try:
        import FL_CustomMLPCLassifierImplementation_Multiple_Rounds as entry
    finally:
        sys.path.remove(ROOT)
    assert entry.parse_args([]).gather_plane == "host"
    assert entry.parse_args(["--gather-plane", "xgmi"]).gather_plane == "xgmi"
    assert entry._gather_fields(entry.parse_args(["--gather-plane", "xgmi"])) == {"gather_plane": "xgmi"}
    with pytest.raises(SystemExit):
        entry.parse_args(["--gather-plane", "pcie"])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "FL_CustomMLPCLassifierImplementation_Multiple_Rounds.py"),
                        "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--gather-plane {host,xgmi}" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
