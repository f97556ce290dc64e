"""Record-level DP-SGD on the CPU: the torch engine's ghost norms and clipped gradient against per-row
float64 autograd, the record-level accountant, and what the option is refused with."""
import numpy as np
import pytest
import torch

from fedmi.fl.engine import EngineConfig, TorchRoundEngine
from fedmi.models.mlp import init_flat
from fedmi.privacy.accountant import epsilon_rdp, epsilon_record_level
from fedmi.privacy.dpsgd import ghost_clipped_grad

from .dpsgd_oracle import DPSGD_SHAPES, clipped_sum, row_grads_f64
from .reference_oracle import DATA_SEED, INIT_SEED, make_multiclass, nerr


@pytest.mark.parametrize("dims", DPSGD_SHAPES, ids=lambda d: "-".join(map(str, d)))
def test_ghost_norms_and_clipped_sum_equal_per_row_autograd(dims):
    X, y = make_multiclass(37, dims[0], dims[-1], DATA_SEED)
    flat = init_flat(list(dims), INIT_SEED)
    G, ce = row_grads_f64(flat, dims, X, y)
    ref_norms = np.sqrt((G * G).sum(1))
    for C in (2 * ref_norms.max(), float(np.median(ref_norms)), 1e-3 * ref_norms.min()):
        norms, grad, loss = ghost_clipped_grad(torch.as_tensor(flat).double(), dims, torch.as_tensor(X).double(),
                                               torch.as_tensor(y), C)
        assert np.max(np.abs(norms.numpy() - ref_norms) / ref_norms) < 1e-12
        assert nerr(grad.numpy(), clipped_sum(G, C, len(X))) < 1e-12
        assert abs(float(loss) - ce.mean()) < 1e-12


def test_record_level_epsilon_composes_over_every_step():
    assert epsilon_record_level(1.1, 40, 3, 1e-5) == epsilon_rdp(1.1, 120, 1e-5)
    assert epsilon_record_level(0.0, 1, 1, 1e-5) == float("inf")
    with pytest.raises(ValueError):
        epsilon_record_level(1.0, 4, 0, 1e-5)


@pytest.mark.parametrize("kw, msg", [
    (dict(dpsgd_noise=0.5), "dpsgd_clip"), (dict(dpsgd_clip=-1.0), "dpsgd_clip"),
    (dict(dpsgd_clip=1.0, dpsgd_noise=float("nan")), "dpsgd_noise"), (dict(dpsgd_clip=1.0, dpsgd_seed=2 ** 64), "dpsgd_seed"),
    (dict(dpsgd_clip=1.0, dtype="bf16"), "bf16")])
def test_invalid_options_are_refused(kw, msg):
    X, y = make_multiclass(20, 14, 2, DATA_SEED)
    with pytest.raises(ValueError, match=msg):
        TorchRoundEngine(X, y, 2, EngineConfig(hidden=(4,), max_rounds=2, **kw), None, init_flat([14, 4, 2], 1))


def test_unsupported_front_ends_refuse_the_option():
    from fedmi.fl.sklearn_fed import refuse_dpsgd
    from fedmi.fl.wide import WideClient
    from fedmi.hpo.fed_sweep import FedTrial, FedTrialGroup
    X, y = make_multiclass(40, 14, 2, DATA_SEED)
    cfg = EngineConfig(max_rounds=2, dpsgd_clip=0.5)
    with pytest.raises(ValueError, match="dpsgd"):
        FedTrialGroup(X, y, 2, [FedTrial((4,), 0.01, 1)], None, cfg, backend="torch")
    with pytest.raises(ValueError, match="dpsgd"):
        WideClient(torch.as_tensor(X), torch.as_tensor(y), [14, 50, 200, 2], dpsgd_clip=0.5)
    with pytest.raises(ValueError, match="dpsgd"):
        refuse_dpsgd(cfg)
    from fedmi.fl.engine import HipRoundEngine
    with pytest.raises(ValueError, match="comm_buffers"):   # (refused before the native library is loaded)
        HipRoundEngine(X, y, 2, cfg, None, init_flat([14, 50, 200, 2], 1), comm_buffers=[torch.zeros(4), torch.zeros(4)])
    e = TorchRoundEngine(X, y, 2, EngineConfig(hidden=(4,), max_rounds=2, dpsgd_clip=0.5, dpsgd_seed=11), None,
                         init_flat([14, 4, 2], 1))
    e.run(1)
    assert e.row_grad_norms().shape == (40,) and e.portable_state()["dpsgd_seed"] == 11
    assert "dpsgd_seed" not in EngineConfig().to_dict()
