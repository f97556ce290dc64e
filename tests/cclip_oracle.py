"""The float64 group oracle of the centered-clipping tests."""
import torch

from fedmi.fl.aggregate import cclip_torch

from . import geomed_oracle


def cclip_group_f64(monkeypatch, shards, n_classes, cfg, flat, rounds, tamper):
    """A full-participation ``aggregator="cclip"`` group's weights after ``rounds`` rounds in float64: the geomed group
    oracle from the common model ``flat``, its aggregation call replaced by ``cclip_torch`` around the round's input."""
    o = geomed_oracle.Float64GeomedGroupOracle(shards, n_classes, cfg, [flat] * len(shards), lambda r: range(len(shards)),
                                               tamper=tamper)
    centre = lambda: torch.as_tensor(flat if o.x is None else o.x, dtype=torch.float64)
    monkeypatch.setattr(geomed_oracle, "geomed_torch", lambda stack, act, T, nu: cclip_torch(
        stack, act, centre(), int(cfg.cclip_iters), float(cfg.cclip_tau)))
    o.run(rounds)
    return o.x
