"""Spectral screening (DnC) without a GPU: the names and ids, the refusal table, the reference rule in float32
against float64, bad clients, a torch group with ALIE colluders, and the checkpoint round trip.

``planted`` is the data builder of this file and of tests/test_dnc.py.  The margin the GPU tests rely on is
asserted here from the float64 oracle alone: in every iteration the smallest removed score is >= 10 x the
largest kept one (scores have max 1).  m colluders among n clients project (n - m) / n and -m / n after
centring, a score ratio of ((n - m) / m)^2, so m <= n / 5; three clients carry a NaN client instead.
"""
import numpy as np
import pytest
import torch

from fedmi.fl.aggregate import (SCREEN_NAMES, SCREENS, SPECTRAL_SCREENS, dnc_drop_count, dnc_scratch_floats,
                                dnc_select_ref, dnc_subset, mask_bits)
from fedmi.fl.engine import EngineConfig, TorchRoundEngine, screen_id
from fedmi.fl.simulate import ClientGroup, SimRank
from fedmi.models.mlp import dense_to_image, image_layout, init_flat, param_count

from .reference_oracle import DATA_SEED, make_multiclass

SMALL, INCOME = [17, 24, 3], [14, 50, 200, 2]
TAILS = 7


def planted(dims, K, seed):
    """``(a [K, Pimg + TAILS] fp32, real [Pimg], sampled [K] bools, f, colluders, nan_client)``: honest clients
    ``base + 0.1 noise``; K // 6 colluders moved 0.25 sqrt(P) along one unit direction; one client all NaN (always bad);
    K >= 16: two honest clients not sampled; NaN / 1e30 in the image padding of clients 0 / 1.  ``f`` counts the
    colluders and the NaN client, so ``q = f`` removes exactly them."""
    pimg, P, rng = image_layout(dims)[2], param_count(dims), np.random.default_rng(seed)
    dense = rng.standard_normal(P) + 0.1 * rng.standard_normal((K, P))
    unit = rng.standard_normal(P)
    unit /= np.linalg.norm(unit)
    bad = [int(k) for k in rng.choice(np.arange(2, K - 1), size=K // 6, replace=False)] if K >= 6 else []
    dense[bad] += 0.25 * np.sqrt(P) * unit     # 2.5 x the norm of a client's own noise
    a = rng.standard_normal((K, pimg + TAILS)).astype(np.float32)
    a[:, :pimg] = np.stack([dense_to_image(row.astype(np.float32), dims) for row in dense])
    real = dense_to_image(np.ones(P, np.float32), dims) != 0
    nan = K - 1
    a[nan, :pimg], a[0, :pimg][~real], a[1, :pimg][~real] = np.nan, np.nan, 1e30
    sampled = np.ones(K, bool)
    if K >= 16:
        sampled[[k for k in range(2, K - 1) if k not in bad][:2]] = False
    return a, real, sampled, len(bad) + 1, bad, nan


@pytest.mark.parametrize("sub", [1.0, 0.5])
@pytest.mark.parametrize("K", [3, 16, 17, 64])
@pytest.mark.parametrize("dims", [SMALL, INCOME], ids=["small", "income"])
def test_reference_fp32_equals_fp64_with_margin(dims, K, sub):
    a, real, sampled, f, bad, nan = planted(dims, K, 40 + K)
    pimg = real.shape[0]
    kept64, rec64 = dnc_select_ref(a[:, :pimg], sampled, real, f, 1.0, 3, sub, 9, 2, np.float64)
    kept32, rec32 = dnc_select_ref(a[:, :pimg], sampled, real, f, 1.0, 3, sub, 9, 2, np.float32)
    assert kept32 == kept64 == [bool(sampled[k]) and k not in bad and k != nan for k in range(K)]
    for t, (r64, r32) in enumerate(zip(rec64, rec32)):
        assert r64["bad"] == r32["bad"] == [k == nan for k in range(K)] and r64["kept"] == r32["kept"]
        s = r64["scores"]
        removed = [s[k] for k in range(K) if sampled[k] and not r64["kept"][k]]
        keep = [s[k] for k in range(K) if r64["kept"][k]]
        assert len(removed) == f and min(removed) >= 10.0 * max(keep), (t, min(removed), max(keep))
        sub_t = dnc_subset(real, sub, 9, 2, t)
        assert not (sub_t & ~real).any() and (sub_t.sum() == real.sum() if sub == 1.0 else
                                               abs(sub_t.sum() / real.sum() - 0.5) < 0.1)
    if sub < 1.0:   # every iteration and every round draws its own subset
        assert (dnc_subset(real, sub, 9, 2, 0) != dnc_subset(real, sub, 9, 2, 1)).any()
        assert (dnc_subset(real, sub, 9, 2, 0) != dnc_subset(real, sub, 9, 3, 0)).any()


def planted_bad():
    """``planted(SMALL, 9, 3)`` with three more bad clients: 4 scaled by 1e30 (over the 2**60 cut), 6 with one inf,
    3 at 1.1e18 everywhere -- under the cut, but 507 squares of 9e17 leave fp32: bad by its diagonal alone (the
    honest clients' centred values, -1.6e17, do not).  Returns ``(a, real, sampled, bad clients)``."""
    a, real, sampled, f, bad, nan = planted(SMALL, 9, 3)
    pimg = real.shape[0]
    a[4, :pimg] *= 1e30
    a[6, np.flatnonzero(real)[5]] = np.inf
    a[3, :pimg] = 1.1e18
    return a, real, sampled, (3, 4, 6, nan)


def test_nan_and_huge_clients_are_removed_as_bad():
    a, real, sampled, bad = planted_bad()
    pimg = real.shape[0]
    for dt in (np.float32, np.float64):
        kept, rec = dnc_select_ref(a[:, :pimg], sampled, real, 0, 1.0, 1, 1.0, 0, 0, dt)   # q = 0: only bad clients go
        assert rec[0]["bad"] == [k in bad for k in range(9)] and kept == [k not in bad for k in range(9)]
        assert np.isinf(rec[0]["scores"][list(bad)]).all()
        # nobody survives: the screen abstains
        assert dnc_select_ref(a[[8, 8], :pimg], [True, True], real, 0, 1.0, 1, 1.0, 0, 0, dt)[0] == [True, True]


def _cfg(**kw):
    return EngineConfig(**{**dict(hidden=(4,), max_rounds=3, screen="dnc"), **kw})


def test_names_ids_and_config_record():
    assert SCREENS == ("none", "multi_krum") and SPECTRAL_SCREENS == ("dnc",) and SCREEN_NAMES[2] == "dnc"
    assert [screen_id(EngineConfig(screen=s)) for s in SCREEN_NAMES] == [0, 1, 2]
    d = EngineConfig()
    assert (d.screen_iters, d.screen_subsample, d.screen_filter, d.screen_seed) == (1, 1.0, 1.0, 0)
    new = ("screen_iters", "screen_subsample", "screen_filter", "screen_seed")
    assert not any(k in d.to_dict() for k in new) and not any(k in EngineConfig(screen="multi_krum").to_dict() for k in new)
    assert all(k in _cfg().to_dict() for k in new)
    assert dnc_drop_count(3, 1.5) == 5 and dnc_scratch_floats(11352, 3, 64) == 3 * (89 * 4100 + 4288)


@pytest.mark.parametrize("kw, world, msg", [
    (dict(screen="spectral"), None, "screen must be one of"), (dict(screen_iters=0), None, "screen_iters"),
    (dict(screen_iters=9), None, "screen_iters"), (dict(screen_iters=1.0), None, "screen_iters"),
    (dict(screen_subsample=0.0), None, "screen_subsample"), (dict(screen_subsample=1.5), None, "screen_subsample"),
    (dict(screen_filter=0.0), None, "screen_filter"), (dict(screen_filter=float("inf")), None, "screen_filter"),
    (dict(screen_seed=-1), None, "screen_seed"), (dict(screen_seed=2 ** 64), None, "screen_seed"),
    (dict(screen_keep=3), None, "screen_keep"), (dict(secagg=True, secagg_seed=1), None, "secagg"),
    (dict(dp_clip=1.0), None, "differential privacy"), (dict(gather_plane="xgmi"), None, "one-shot select kernel"),
    (dict(), 65, "at most 64 clients"), (dict(screen_byzantine=7), 7, "screen_byzantine"),
    (dict(screen_byzantine=2, screen_iters=3, screen_filter=1.5), 9, "screen_byzantine"),   # 9 - 3 * 3 < 1
    (dict(screen_byzantine=2, participation=0.5), 4, "screen_byzantine")])                  # 2 of 4 sampled
def test_refusals(kw, world, msg):
    with pytest.raises(ValueError, match=msg):
        if world is None:
            screen_id(_cfg(**kw))
        else:
            X, y = make_multiclass(24, 5, 2, DATA_SEED)
            TorchRoundEngine(X, y, 2, _cfg(**kw), SimRank(world, 0, "cpu"), init_flat([5, 4, 2], 0),
                             n_total=world * len(X), client_sizes=[len(X)] * world)
    if world is None and "screen" not in kw and kw.keys() & {"screen_iters", "screen_subsample", "screen_filter", "screen_seed"}:
        with pytest.raises(ValueError, match=msg):   # validated with the screen off too
            screen_id(EngineConfig(**kw))


def _alie_group(backend, agg="mean", rounds=4, **kw):
    X, y = make_multiclass(270, 17, 3, DATA_SEED)
    torch.set_num_threads(1)
    cfg = EngineConfig(hidden=(24,), max_rounds=6, early_stop=False, graph_rounds=0, eps=1e-4, screen="dnc",
                       screen_byzantine=2, attack="alie", attack_clients=(2, 5), attack_z=1.0, aggregator=agg, **kw)
    g = ClientGroup(X, y, 9, cfg, backend=backend, shard_mode="iid", seed=2)
    g.run(rounds)
    return g


def test_torch_group_drops_the_alie_colluders_and_checkpoints(tmp_path):
    from fedmi.ckpt.checkpoint import load_checkpoint, resume, save_checkpoint
    g = _alie_group("torch", screen_iters=2, screen_subsample=0.5, screen_seed=11)
    lead = g.clients[0]
    kept = lead.history()["screen_kept"]
    assert lead.screen == 2 and lead.agg_scale == 1.0 and len(kept) == 4
    for w in kept:
        assert int(w) & mask_bits(k in (2, 5) for k in range(9)) == 0 and bin(int(w)).count("1") >= 9 - 2 * 2
    save_checkpoint(str(tmp_path), lead)
    meta = load_checkpoint(str(tmp_path))["meta"]
    cfg = meta["config"]
    assert (cfg["screen"], cfg["screen_iters"], cfg["screen_subsample"], cfg["screen_filter"], cfg["screen_seed"]) == \
        ("dnc", 2, 0.5, 1.0, 11)
    assert meta["history"]["screen_kept"] == [int(w) for w in kept]
    fresh = _alie_group("torch", rounds=0, screen_iters=2, screen_subsample=0.5, screen_seed=11).clients[0]
    assert resume(str(tmp_path), fresh) == 4
    np.testing.assert_array_equal(fresh.history()["screen_kept"], kept)
