"""Contribution scores on the CPU: the coalition tables, the Shapley / leave-one-out math, the torch group, the refusals."""
import numpy as np
import pytest

from fedmi.fl.contribution import (coalition_images_model, coalition_masks, coalition_perms, leave_one_out,
                                   shapley_exact, shapley_permutations)
from fedmi.fl.engine import EngineConfig
from fedmi.fl.simulate import ClientGroup

from .reference_oracle import DATA_SEED, make_multiclass


def test_mask_tables():
    assert coalition_masks("loo", 3).tolist() == [7, 6, 5, 3]
    assert coalition_masks("shapley", 3).tolist() == list(range(8))
    tab, perms = coalition_masks("shapley", 9, 2, seed=5), coalition_perms(9, 2, 5)
    assert len(tab) == 19 and tab[0] == 0 and tab[9] == tab[18] == 511
    for p in range(2):   # nested prefixes, one client more each
        chain = [0, *[int(t) for t in tab[1 + 9 * p:10 + 9 * p]]]
        assert [b & ~a for a, b in zip(chain, chain[1:])] == [1 << int(i) for i in perms[p]]
    np.testing.assert_array_equal(tab, coalition_masks("shapley", 9, 2, seed=5))
    assert (tab != coalition_masks("shapley", 9, 2, seed=6)).any()
    for bad in (("shapley", 9, 0), ("shapley", 64, 64), ("shapley", 9, 456)):   # no permutations; 4097 coalitions
        with pytest.raises(ValueError, match="contribution"):
            coalition_masks(*bad)


def test_shapley_exact_on_a_hand_computed_game():
    # u(T) by mask over players {0, 1, 2}: the glove game with a bonus -- phi = (2/3 + 1, 1/6, 1/6) by hand:
    # u = 1 iff client 0 and one of {1, 2}; plus 1 whenever client 0 is in
    u = np.array([0, 1, 0, 2, 0, 2, 0, 2], np.float64)
    np.testing.assert_allclose(shapley_exact(u, [0, 1, 2]), [1 + 2 / 3, 1 / 6, 1 / 6], atol=1e-15)
    np.testing.assert_allclose(shapley_exact(u, 0b011), [1.5, 0.5, 0.0], atol=1e-15)   # client 2 unsampled: null, 0
    np.testing.assert_array_equal(leave_one_out(u[[7, 6, 5, 3]], [0, 1, 2]), [2, 0, 0])


@pytest.mark.parametrize("K,sampled", [(4, 0b1111), (4, 0b1011), (9, 0b111111111), (9, 0b101100110)])
def test_efficiency_null_players_and_twins_on_the_models_own_utilities(K, sampled):
    """Utilities from the build's host model: u(T) = -|model(T) - target|^2.  Client 1's buffer duplicates client 0's."""
    rng = np.random.default_rng(K)
    w = rng.uniform(0.1, 0.3, K).astype(np.float32)
    models = rng.standard_normal((K, 8)).astype(np.float32)
    models[1], w[1] = models[0], w[0]
    v, x, target = w[:, None] * models, np.zeros(8, np.float32), rng.standard_normal(8)
    masks, perms = coalition_masks("shapley", K, 3, 1), (coalition_perms(K, 3, 1) if K > 8 else None)
    img = coalition_images_model(v, w, x, np.ones(8, bool), masks, sampled)
    u = -((img.astype(np.float64) - target) ** 2).sum(1)
    phi = shapley_exact(u, sampled, K) if K <= 8 else shapley_permutations(u, perms, sampled)
    full = u[-1]   # (exact: index 2^K - 1; permutations: a chain's last prefix)
    assert abs(phi.sum() - (full - u[0])) <= 1e-12 * max(1.0, abs(full))   # efficiency
    assert all(phi[i] == 0.0 for i in range(K) if not (sampled >> i) & 1)   # unsampled: null player
    if K <= 8:
        assert abs(phi[0] - phi[1]) <= 1e-12   # identical buffers, equal exact scores


def _cfg(**kw):
    return EngineConfig(**{**dict(hidden=(24,), max_rounds=4, early_stop=False, graph_rounds=0), **kw})


def _data():
    X, y = make_multiclass(461, 17, 3, DATA_SEED)
    return X[:400], y[:400], (X[400:], y[400:])


def test_torch_group_ranks_the_sign_flip_attacker_last():
    X, y, ho = _data()
    g = ClientGroup(X, y, 4, _cfg(contribution="shapley", attack="sign_flip", attack_clients=(2,), attack_scale=3.0,
                                  contribution_every=2), backend="torch", shard_mode="iid", seed=2, heldout=ho)
    g.run(3)
    h = g.history()
    assert h["contribution"].shape == h["contribution_acc"].shape == (3, 4) and h["coalition_loss_sum"].shape == (3, 16)
    assert np.isnan(h["contribution"][1]).all() and (h["coalition_correct"][1] == -1).all()   # round 1 is not scored
    for r in (0, 2):
        assert np.argmin(h["contribution"][r]) == 2
        u = -(h["coalition_loss_sum"][r].astype(np.float64) / 61)
        assert abs(h["contribution"][r].sum() - (u[15] - u[0])) < 1e-12
    plain = ClientGroup(X, y, 4, _cfg(attack="sign_flip", attack_clients=(2,), attack_scale=3.0), backend="torch",
                        shard_mode="iid", seed=2, heldout=ho)
    plain.run(3)
    assert set(h) - set(plain.history()) == {"coalition_masks", "coalition_loss_sum", "coalition_correct", "contribution",
                                             "contribution_acc"}
    assert set(plain.history()) == set(ClientGroup(X, y, 4, _cfg(), backend="torch", heldout=ho).history())
    np.testing.assert_array_equal(g.global_flat(), plain.global_flat())


@pytest.mark.parametrize("kw,k,heldout,match", [
    ({}, 4, False, "held-out"), (dict(secagg=True, secagg_seed=1), 4, True, "secagg"),
    (dict(dp_clip=1.0), 4, True, "dp_clip"), (dict(compress="topk"), 4, True, "compress"),
    (dict(aggregator="median"), 4, True, "aggregator"), (dict(screen="multi_krum"), 5, True, "screen"),
    (dict(contribution_perms=0), 9, True, "contribution_perms"), ({}, 65, True, "64 clients"),
    (dict(contribution="banzhaf"), 4, True, "must be one of")])
def test_refusals_name_the_conflict(kw, k, heldout, match):
    X, y, ho = _data()
    with pytest.raises(ValueError, match=match):
        ClientGroup(X, y, k, _cfg(**{"contribution": "shapley", **kw}), backend="torch", heldout=ho if heldout else None)


def test_refusals_outside_the_group():
    import torch
    from fedmi.fl.engine import HipRoundEngine, TorchRoundEngine
    from fedmi.fl.simulate import SimRank
    from fedmi.fl.wide import WideClient
    from fedmi.hpo.fed_sweep import FedTrialGroup
    from fedmi.models.mlp import init_flat

    class TwoRanks:
        size, rank = 2, 0
    X, y, _ = _data()
    with pytest.raises(ValueError, match="use ClientGroup"):
        TorchRoundEngine(X, y, 3, _cfg(contribution="loo"), TwoRanks(), init_flat([17, 24, 3], 0), n_total=800)
    with pytest.raises(ValueError, match="comm_buffers.*contribution"):   # trial packing
        HipRoundEngine(X, y, 3, _cfg(contribution="loo"), SimRank(3, 0, "cpu"), init_flat([17, 24, 3], 0),
                       comm_buffers=(torch.zeros(8), torch.zeros(8)))
    with pytest.raises(ValueError, match="contribution"):
        WideClient(None, None, [17, 24, 3], contribution="loo")
    with pytest.raises(ValueError, match="contribution"):
        FedTrialGroup(X, y, 3, [], None, _cfg(contribution="loo"))
    ClientGroup(X, y, 1, _cfg(contribution="shapley"), backend="torch")   # one client: off, nothing refused
