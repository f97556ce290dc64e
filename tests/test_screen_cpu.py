"""Multi-Krum screening on the CPU: the host models of the distance kernel and of the selection rule
against an independent float64 numpy oracle, the rule's details by hand-written expectation, torch
client groups with colluding tamperers, three ranks over gloo, config validation and the [C] flags.

Oracle.  ``((a[:, None] - a[None]) ** 2).sum(-1)`` in float64 over the sampled clients, ``np.sort`` per
row, the sum of the ``K_r - f - 2`` smallest off-diagonal entries, ``argsort`` of the scores.  It shares
no code with ``pair_distances_model`` / ``screen_select``; it decides the same kept set wherever the
scores at the keep boundary are further apart than the fp32 error of the models, which the generated
cases guarantee by construction and the test asserts for every one of them (relative gap >= 1e-3).

Distance bound.  A term is ``fl(fl(a - b)^2)``: the subtraction's rounding enters squared, the
multiplication's once -- a factor within ``(1 + u)^3`` of the exact square, u = 2^-24.  The terms are
non-negative and every one passes through at most ``chain = 4 ceil(Pimg / 4 / 256) + 6 + 4`` additions
(a thread's float4s lane by lane, 6 levels of the wave's xor tree, 4 wave sums), each within
``(1 + u)``.  So ``|model - exact| <= ((1 + u)^(chain + 3) - 1) exact``, asserted as it stands against the
float64 distance of the same fp32 inputs (whose own error, ~ Pimg 2^-53, is far below).  The bound is
1.3e-6 of d for the 17-24-3 image and 5.3e-6 for the 14-50-200-2 image: under 1e-5, so not vacuous.
"""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fedmi.fl.aggregate import (AGGREGATORS, SCREENS, mask_bits, pair_distances_model, pair_distances_torch,
                                robust_aggregate_torch, screen_keep_count, screen_select)
from fedmi.fl.engine import EngineConfig, TorchRoundEngine, screen_id
from fedmi.fl.simulate import ClientGroup, SimRank
from fedmi.models.mlp import dense_to_image, image_layout, init_flat, param_count

from .reference_oracle import DATA_SEED, make_multiclass

U = 2.0 ** -24
KS = (3, 5, 7, 8, 9, 17, 64)
P = 1000   # floats of the synthetic "images" of the rule tests (every position real; one float4 per thread)


def dist_chain(pimg):
    """Longest sequential chain of additions of the distance kernel's reduction (module docstring)."""
    return 4 * math.ceil(pimg / 4 / 256) + 6 + 4


def oracle(stack, mask, f, m):
    """(kept mask, relative gap between the oracle scores on both sides of the keep boundary or None)."""
    S = np.flatnonzero(mask)
    kr = len(S)
    if kr < 2 * f + 3:
        return np.asarray(mask, bool).copy(), None
    a = np.asarray(stack, np.float64)[S]
    d = ((a[:, None] - a[None]) ** 2).sum(-1)
    nb = kr - f - 2
    scores = np.sort(d, axis=1)[:, 1:nb + 1].sum(axis=1)   # (column 0: the zero diagonal)
    want = kr - f if m is None else min(m, kr - f)
    order = np.argsort(scores, kind="stable")
    kept = np.zeros(len(mask), bool)
    kept[S[order[:want]]] = True
    gap = None
    if want < kr:
        lo, hi = scores[order[want - 1]], scores[order[want]]
        gap = (hi - lo) / hi
    return kept, gap


def planted(K, mask, seed, graded=False):
    """[K, P] fp32: honest clients ``base + 0.1 noise``; the first ``(K_r - 3) // 2`` sampled clients of a
    seeded shuffle are Byzantine, each at its own far distance ``base + 20 (q + 1) + noise``.  ``graded``:
    no Byzantine client, and honest client k's noise is scaled by ``1 + 0.2 k``, so the honest scores are
    spread and a keep boundary INSIDE the honest clients (``screen_keep`` below ``K_r - f``) has a gap too
    (beside far Byzantine clients that f does not cover, their distances would swamp every honest score)."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(P)
    a = base + 0.1 * rng.standard_normal((K, P)) * (1.0 + 0.2 * np.arange(K)[:, None] if graded else 1.0)
    S = rng.permutation(np.flatnonzero(mask))
    for q, k in enumerate(S[:0 if graded else max(0, (len(S) - 3) // 2)]):
        a[k] = base + 20.0 * (q + 1) + rng.standard_normal(P)
    return a.astype(np.float32)


def holes(K, seed):
    rng = np.random.default_rng(seed)
    m = np.ones(K, bool)
    m[rng.choice(K, size=max(1, K // 4), replace=False)] = False
    return m


@pytest.mark.parametrize("K", KS)
def test_host_models_against_the_float64_oracle(K):
    real = np.ones(P, bool)
    cases = gaps = 0
    for mask, graded in ((np.ones(K, bool), False), (holes(K, 40 + K), False), (np.ones(K, bool), True)):
        if graded and K > 9:
            continue
        kr = int(mask.sum())
        a = planted(K, mask, 1000 + 2 * K + int(mask.all()), graded)
        dm = pair_distances_model(a, mask, real)
        dt = pair_distances_torch(torch.as_tensor(a), mask)
        np.testing.assert_array_equal(dm, dm.T)
        assert (np.diag(dm) == 0).all() and (dm[~mask] == 0).all() and (dm[:, ~mask] == 0).all()
        for f in range(0, (kr - 3) // 2 + 1 if kr >= 3 else 1):
            for m in ((None, 1, 2, 3) if graded else (None,)):
                # (nb = 1 is left to the hand-written ties: two mutually nearest clients share one score
                # exactly, d being symmetric, so a keep boundary between them has no gap by design)
                if m is not None and (m > kr - f or kr - f - 2 < 2):
                    continue
                kept, gap = oracle(a, mask, f, m)
                tag = f"K={K} K_r={kr} f={f} m={m}"
                if gap is not None:
                    assert gap >= 1e-3, (tag, gap)   # every generated case: far above the ~4e-6 fp32 chain error
                    gaps += 1
                assert kept.sum() == screen_keep_count(kr, f, m), tag
                assert screen_select(dm, mask, f, m) == kept.tolist(), tag
                assert screen_select(dt, mask, f, m) == kept.tolist(), tag
                cases += 1
    assert cases >= 2 and (gaps > 0 or K == 3)


@pytest.mark.parametrize("dims", [[17, 24, 3], [14, 50, 200, 2]], ids=["small", "income"])
def test_distance_model_within_its_chain_bound(dims):
    pimg = image_layout(dims)[2]
    real = dense_to_image(np.ones(param_count(dims), np.float32), dims) != 0
    rng = np.random.default_rng(5)
    K = 6
    a = np.stack([dense_to_image(rng.standard_normal(param_count(dims)).astype(np.float32), dims) for _ in range(K)])
    a[0][~real] = np.nan          # padding never enters a distance
    a[3][~real] = 1e30
    mask = np.ones(K, bool)
    d = pair_distances_model(a, mask, real)
    exact = ((a[:, None, real].astype(np.float64) - a[None, :, real].astype(np.float64)) ** 2).sum(-1)
    rel = (1.0 + U) ** (dist_chain(pimg) + 3) - 1.0
    assert rel < 1e-5, rel        # not vacuous
    off = ~np.eye(K, dtype=bool)
    err = np.abs(d.astype(np.float64) - exact)
    print(f"{dims}: chain {dist_chain(pimg)}, bound {rel:.3g} of d, worst error {float((err[off] / exact[off]).max()):.3g} of d")
    assert (err[off] <= rel * exact[off]).all(), float((err[off] / exact[off]).max())
    assert (np.diag(d) == 0).all()
    # the model does not depend on how many clients stand beside a pair
    d2 = pair_distances_model(a[[1, 4]], [True, True], real)
    assert d2[0, 1].view(np.int32) == d[1, 4].view(np.int32)


def _stack(K, seed=3):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(P) + 0.1 * rng.standard_normal((K, P))).astype(np.float32)


def test_duplicates_tie_and_the_lower_index_wins():
    a = _stack(6)
    a[4] = a[1]                                   # exact duplicates: equal rows of d, equal scores
    mask = np.ones(6, bool)
    d = pair_distances_model(a, mask, np.ones(P, bool))
    assert d[1, 4] == 0 and (d[1][[0, 2, 3, 5]] == d[4][[0, 2, 3, 5]]).all()
    for f in (0, 1):
        full = screen_select(d, mask, f, None)
        for m in range(1, 6 - f + 1):
            kept = screen_select(d, mask, f, m)
            assert sum(kept) == m
            assert not (kept[4] and not kept[1]), (f, m, kept)      # 4 is never kept without 1
            assert all(full[k] or not kept[k] for k in range(6))    # nested in the m = K_r - f set
    # a hand-made matrix: clients 0, 1, 2 all at distance 1 from each other, 3 far away; f = 0, nb = 2
    d = np.array([[0, 1, 1, 9], [1, 0, 1, 9], [1, 1, 0, 9], [9, 9, 9, 0]], np.float32)
    assert screen_select(d, [True] * 4, 0, 1) == [True, False, False, False]
    assert screen_select(d, [True] * 4, 0, 2) == [True, True, False, False]
    assert screen_select(d, [True] * 4, 0, None) == [True] * 4
    # f = 0, nb = 2: scores 0 -> 2 + 2 = 4; 1 -> 1 + 2 = 3; 2 -> 2 + 5 = 7; 3 -> 1 + 2 = 3: the tie (1, 3) goes to 1
    d = np.array([[0, 2, 2, 2], [2, 0, 5, 1], [2, 5, 0, 7], [2, 1, 7, 0]], np.float32)
    assert screen_select(d, [True] * 4, 0, 1) == [False, True, False, False]
    assert screen_select(d, [True] * 4, 0, 2) == [False, True, False, True]
    got = [screen_select(d, [True] * 4, 0, m) for m in (1, 2, 3)]
    nb2 = lambda i: float(np.sort(d[i])[1:3].sum())    # f = 0: nb = 2
    order = sorted(range(4), key=lambda i: (nb2(i), i))
    assert got == [[i in order[:m] for i in range(4)] for m in (1, 2, 3)]


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf"), 1e30], ids=["nan", "inf", "-inf", "1e30"])
def test_non_finite_clients_score_inf_and_are_never_kept(bad):
    K = 7
    a = _stack(K)
    a[2] = bad
    if bad == 1e30:
        a[5, ::2] = 1e30                          # partly huge: its squares overflow all the same
    else:
        a[5, 17] = bad                            # one bad coordinate is enough
    mask = np.ones(K, bool)
    d = pair_distances_model(a, mask, np.ones(P, bool))
    assert (d[2, [0, 1, 3, 4, 5, 6]] == np.inf).all() and (d[5, [0, 1, 2, 3, 4, 6]] == np.inf).all()
    assert not np.isnan(d).any() and d[2, 2] == 0 and d[5, 5] == 0
    dt = pair_distances_torch(torch.as_tensor(a), mask)
    assert (dt[2, [0, 1, 3, 4, 5, 6]] == np.inf).all() and not np.isnan(dt).any()
    for dist in (d, dt):
        for f in (1, 2):
            for m in (None, 1, 3):
                kept = screen_select(dist, mask, f, m)
                assert not kept[2] and not kept[5] if f == 2 else not (kept[2] and kept[5]), (f, m, kept)
                if f == 2:
                    assert sum(kept) == (5 if m is None else m)
    # one bad client, f = 1: never kept, whatever m
    a[5] = a[4] + np.float32(0.01)
    d = pair_distances_model(a, mask, np.ones(P, bool))
    for m in (None, 1, 2, 6):
        kept = screen_select(d, mask, 1, m)
        assert not kept[2] and sum(kept) == (6 if m is None else m)
    # +inf == +inf ties: every score infinite (nb reaches the bad client for all): the lower indices are kept
    d = np.full((5, 5), np.inf, np.float32)
    np.fill_diagonal(d, 0)
    assert screen_select(d, [True] * 5, 1, 2) == [True, True, False, False, False]


def test_unsampled_rows_are_ignored_whatever_they_hold():
    K = 9
    a = _stack(K)
    mask = np.ones(K, bool)
    mask[[1, 6]] = False
    real = np.ones(P, bool)
    d = pair_distances_model(a, mask, real)
    ref = screen_select(d, mask, 2, None)
    assert not ref[1] and not ref[6] and sum(ref) == 5
    for junk in (np.nan, -1.0, 0.0, np.inf):
        dj = d.copy()
        dj[[1, 6], :] = junk
        dj[:, [1, 6]] = junk
        assert screen_select(dj, mask, 2, None) == ref
    b = a.copy()
    b[1], b[6] = np.nan, 1e30
    np.testing.assert_array_equal(pair_distances_model(b, mask, real), d)
    # equal to the rule on the sampled clients alone
    sub = np.flatnonzero(mask)
    alone = screen_select(pair_distances_model(a[sub], np.ones(len(sub), bool), real), np.ones(len(sub), bool), 2, None)
    assert [ref[k] for k in sub] == alone


def test_too_few_sampled_clients_keep_all():
    a = _stack(6)
    a[0] = np.nan
    for kr, f in ((1, 0), (2, 0), (4, 1), (6, 2)):       # K_r < 2 f + 3
        mask = np.arange(6) < kr
        d = pair_distances_model(a, mask, np.ones(P, bool))
        assert screen_select(d, mask, f, None) == mask.tolist()
        assert screen_select(d, mask, f, 1) == mask.tolist()
        assert screen_keep_count(kr, f, 1) == kr
    assert screen_keep_count(5, 1, None) == 4 and screen_keep_count(5, 1, 9) == 4 and screen_keep_count(5, 1, 2) == 2
    with pytest.raises(ValueError):
        screen_select(np.zeros((3, 3), np.float32), [True] * 3, -1, None)
    with pytest.raises(ValueError):
        screen_select(np.zeros((3, 3), np.float32), [True] * 3, 0, 0)
    with pytest.raises(ValueError):
        screen_select(np.zeros((3, 4), np.float32), [True] * 3, 0, None)


@pytest.mark.parametrize("agg", AGGREGATORS)
def test_keep_one_returns_the_argmin_clients_model(agg):
    K = 7
    a = _stack(K, seed=11)
    a[3] = a[3] + 30.0
    mask = np.ones(K, bool)
    mask[0] = False
    d = pair_distances_model(a, mask, np.ones(P, bool))
    kept = screen_select(d, mask, 1, 1)
    assert sum(kept) == 1
    S = np.flatnonzero(mask)
    d64 = ((a[S][:, None].astype(np.float64) - a[S][None].astype(np.float64)) ** 2).sum(-1)
    sc = np.sort(d64, axis=1)[:, 1:4].sum(axis=1)                     # nb = 6 - 1 - 2 = 3
    best = S[np.argmin(sc)]
    assert (np.sort(sc)[1] - np.sort(sc)[0]) / np.sort(sc)[1] >= 1e-3  # the float64 argmin is not a near tie
    assert kept[best]
    kind, beta = ("trimmed_mean", 0.0) if agg == "mean" else (agg, 0.2)   # what a screening engine runs
    out = robust_aggregate_torch(torch.as_tensor(a), kept, kind, beta).numpy()
    np.testing.assert_array_equal(out.view(np.int32), a[best].view(np.int32))


# ---- groups ----
ROUNDS = 6
DIMS = [17, 24, 3]
NP = param_count(DIMS)
BAD = (2, 5)


def _group(tamper=None, k=7, screened=True, f=2, rounds=ROUNDS, **kw):
    X, y = make_multiclass(140, 17, 3, DATA_SEED)
    scr = dict(screen="multi_krum", screen_byzantine=f) if screened else {}
    cfg = EngineConfig(**{**dict(hidden=(24,), max_rounds=ROUNDS + 2, early_stop=False, graph_rounds=0), **scr, **kw})
    torch.set_num_threads(1)
    g = ClientGroup(X, y, k, cfg, backend="torch", shard_mode="iid", seed=2, tamper=tamper)
    g.run(rounds)
    return g


def _collude(value, who=BAD):
    """The tamperers all publish client 0's model + 50 (``value`` None), or ``value`` everywhere."""
    def tamper(r, bufs):
        for k in who:
            bufs[k][:NP] = bufs[0][:NP] + 50.0 if value is None else value
    return tamper


def _kept_clients(h):
    return [[k for k in range(64) if (int(w) >> k) & 1] for w in h["screen_kept"]]


@pytest.mark.parametrize("agg", AGGREGATORS)
def test_torch_group_rejects_two_colluding_tamperers(agg):
    a = _group(_collude(None), aggregator=agg)
    h = a.history()
    assert h["rounds_run"] == ROUNDS and len(h["screen_kept"]) == ROUNDS and h["screen_kept"].dtype == np.uint64
    for kept in _kept_clients(h):
        assert len(kept) == 5 and not set(kept) & set(BAD), kept
    wa = a.global_flat()
    assert np.isfinite(wa).all()
    b = _group(_collude(float("nan")), aggregator=agg)
    np.testing.assert_array_equal(wa, b.global_flat())          # bitwise: what a rejected client sends is not read
    np.testing.assert_array_equal(h["screen_kept"], b.history()["screen_kept"])
    np.testing.assert_array_equal(h["global"], b.history()["global"])
    for c in a.clients[1:]:
        np.testing.assert_array_equal(c.global_flat(), wa)
        np.testing.assert_array_equal(c.history()["screen_kept"], h["screen_kept"])   # one history for the group
    lead = a.clients[0]
    assert lead.robust and lead.screen == SCREENS.index("multi_krum") and lead.agg_scale == 1.0
    if agg == "mean":
        assert lead.robust_beta == 0.0
        poisoned = _group(_collude(None), screened=False, aggregator="mean")
        assert "screen_kept" not in poisoned.history()
        assert np.abs(poisoned.global_flat() - wa).max() > 5.0   # 2 of 7 clients at +50 move the weighted mean by ~14


def test_torch_group_with_participation_rejects_the_tamperer_when_sampled():
    g = _group(_collude(None, who=(2,)), f=1, participation=0.72)       # 5 of 7 sampled: 2 f + 3
    lead = g.clients[0]
    sampled = [2 in lead.participants(r) for r in range(ROUNDS)]
    assert any(sampled) and not all(sampled)
    for r, kept in enumerate(_kept_clients(g.history())):
        part = set(int(k) for k in lead.participants(r))
        assert len(kept) == 4 and set(kept) <= part and 2 not in kept, (r, kept)
    assert np.isfinite(g.global_flat()).all()


def test_screen_none_is_bit_identical_to_the_default():
    out = []
    for kw in (dict(), dict(screen="none", screen_byzantine=3, screen_keep=2)):
        g = _group(screened=False, k=5, **kw)
        out.append((g.global_flat(), g.history()["global"], g.history()["loss"]))
        assert "screen_kept" not in g.history()
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)


# ---- three ranks over gloo ----
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_cfg():
    return EngineConfig(hidden=(24,), max_rounds=ROUNDS + 2, early_stop=False, graph_rounds=0, screen="multi_krum",
                        screen_byzantine=0, screen_keep=2)


def _gloo_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    try:
        from fedmi.data.sharding import shard_indices
        from fedmi.parallel.comm import Comm
        comm = Comm(backend="gloo", device="cpu")
        X, y = make_multiclass(140, 17, 3, DATA_SEED)
        idx = [shard_indices(len(X), r, world, mode="iid", seed=2, labels=y, alpha=0.5) for r in range(world)]
        e = TorchRoundEngine(X[idx[rank]], y[idx[rank]], 3, _rank_cfg(), comm, init_flat(DIMS, 2 * 1000003 + rank),
                             n_total=sum(len(i) for i in idx))
        e.run(ROUNDS)
        h = e.history()
        q.put((rank, (e.global_flat(), np.asarray(h["global"]), np.asarray(h["loss"]), np.asarray(h["screen_kept"])), None))
        comm.close()
    except Exception:  # noqa: BLE001 -- reported to the parent
        import traceback
        q.put((rank, None, traceback.format_exc()))


def test_three_ranks_over_gloo_equal_the_torch_group_bitwise():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 3, port, q)) for r in range(3)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=120) for _ in range(3)], key=lambda t: t[0])
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.terminate()
    for rank, _, err in res:
        assert err is None, f"rank {rank}:\n{err}"
    X, y = make_multiclass(140, 17, 3, DATA_SEED)
    torch.set_num_threads(1)
    g = ClientGroup(X, y, 3, _rank_cfg(), backend="torch", shard_mode="iid", seed=2)
    g.run(ROUNDS)
    h = g.history()
    assert all(bin(int(w)).count("1") == 2 for w in h["screen_kept"])
    ref = (g.global_flat(), h["global"], h["loss"], h["screen_kept"])
    for rank, out, _ in res:
        for a, b in zip(out, ref):
            np.testing.assert_array_equal(a, b, err_msg=f"rank {rank}")


# ---- config validation ----
def _scr(**kw):
    return EngineConfig(**{**dict(hidden=(4,), max_rounds=3, screen="multi_krum"), **kw})


def test_config_validation_and_refusals():
    assert SCREENS == ("none", "multi_krum")
    d = EngineConfig()
    assert (d.screen, d.screen_byzantine, d.screen_keep) == ("none", 0, None)
    assert [screen_id(EngineConfig(screen=s)) for s in SCREENS] == [0, 1]
    assert all(k in d.to_dict() for k in ("screen", "screen_byzantine", "screen_keep"))
    for bad, msg in ((dict(screen="krum"), "screen must be one of"), (dict(screen_byzantine=-1), "screen_byzantine"),
                     (dict(screen_byzantine=1.5), "screen_byzantine"), (dict(screen_keep=0), "screen_keep"),
                     (dict(secagg=True, secagg_seed=1), "secagg"), (dict(dp_clip=1.0), "differential privacy"),
                     (dict(gather_plane="xgmi"), "one-shot select kernel")):
        with pytest.raises(ValueError, match=msg):
            screen_id(_scr(**bad))
    # the fields are validated with the screen off too; what a screen refuses is not
    with pytest.raises(ValueError, match="screen_byzantine"):
        screen_id(EngineConfig(screen_byzantine=-1))
    assert screen_id(EngineConfig(dp_clip=1.0, gather_plane="xgmi", secagg=True)) == 0

    X, y = make_multiclass(24, 5, 2, DATA_SEED)
    flat = init_flat([5, 4, 2], 0)
    mk = lambda cfg, world=7, **kw: TorchRoundEngine(X, y, 2, cfg, SimRank(world, 0, "cpu") if world > 1 else None, flat,
                                                     n_total=world * len(X), client_sizes=[len(X)] * world, **kw)
    e = mk(_scr(screen_byzantine=2, screen_keep=5))
    assert e.screen == 1 and e.robust == AGGREGATORS.index("trimmed_mean") and e.robust_beta == 0.0 and e.agg_scale == 1.0
    e = mk(_scr(screen_byzantine=2, aggregator="median"))
    assert e.robust == AGGREGATORS.index("median")
    one = mk(_scr(screen_byzantine=5), world=1)          # one client: the screen is off, as a robust aggregator is
    assert one.screen == 0 and one.robust == 0 and "screen_kept" not in one.history()
    for kw in (dict(dp_clip=0.5, dp_seed=1), dict(gather_plane="xgmi")):   # ... so nothing is refused there either
        assert mk(_scr(**kw), world=1).screen == 0
    assert screen_id(_scr(dp_clip=0.5), world=1) == 0 and screen_id(_scr(), world=2) == 1
    for kw, world, msg in ((dict(secagg=True, secagg_seed=1), 7, "secagg"), (dict(dp_clip=0.5, dp_seed=1), 7, "differential privacy"),
                           (dict(gather_plane="xgmi"), 7, "gather_plane='xgmi'"), (dict(), 65, "at most 64 clients"),
                           (dict(screen_byzantine=-1), 7, "screen_byzantine"), (dict(screen_byzantine=3), 7, "2 f \\+ 3"),
                           (dict(screen_byzantine=1, participation=0.5), 7, "2 f \\+ 3"),   # 4 of 7 sampled < 5
                           (dict(screen_byzantine=2, screen_keep=6), 7, "screen_keep"),
                           (dict(screen_byzantine=1, screen_keep=5, participation=0.72), 7, "screen_keep"),   # 5 - 1 = 4
                           (dict(screen_keep=0), 7, "screen_keep")):
        with pytest.raises(ValueError, match=msg):
            mk(_scr(**kw), world=world)
    mk(_scr(screen_byzantine=1, screen_keep=4, participation=0.72))
    from fedmi.hpo.fed_sweep import FedTrial, FedTrialGroup
    with pytest.raises(ValueError, match="client-screening"):
        FedTrialGroup(X, y, 2, [FedTrial((4,), 0.01, 1)], None, _scr(), backend="torch")
    from fedmi.fl.wide import WideClient
    with pytest.raises(ValueError, match="client screening"):
        WideClient(torch.zeros(4, 14), torch.zeros(4, dtype=torch.long), [14, 8, 2], screen="multi_krum")
    from fedmi.fl.engine import HipRoundEngine
    views = [torch.zeros(8), torch.zeros(8)]
    with pytest.raises(ValueError, match="client screening"):   # before anything touches a device
        HipRoundEngine(X, y, 2, _scr(), SimRank(3, 0, "cpu"), flat, comm_buffers=views)
    with pytest.raises(ValueError, match="gather_plane='xgmi'"):
        HipRoundEngine(X, y, 2, _scr(gather_plane="xgmi"), SimRank(3, 0, "cpu"), flat)


def test_checkpoint_config_carries_the_screen_fields(tmp_path):
    from fedmi.ckpt.checkpoint import load_checkpoint, resume, save_checkpoint
    g = _group(_collude(None), rounds=3)
    lead = g.clients[0]
    save_checkpoint(str(tmp_path), lead)
    meta = load_checkpoint(str(tmp_path))["meta"]
    cfg = meta["config"]
    assert (cfg["screen"], cfg["screen_byzantine"], cfg["screen_keep"]) == ("multi_krum", 2, None)
    assert meta["history"]["screen_kept"] == [int(w) for w in lead.history()["screen_kept"]]
    fresh = _group(rounds=0).clients[0]
    assert resume(str(tmp_path), fresh) == 3
    np.testing.assert_array_equal(fresh.history()["screen_kept"], lead.history()["screen_kept"])


# ---- the [C] entry point ----
def test_entry_point_flags():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(root, "FL_CustomMLPCLassifierImplementation_Multiple_Rounds.py")
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    run = lambda *a: subprocess.run([sys.executable, script, "--device", "cpu", "--backend", "gloo", "--engine", "torch",
                                     "--quiet", *a], cwd=root, capture_output=True, text=True, timeout=300, env=env)
    r = run("--clients", "5", "--rounds", "3", "--screen", "multi_krum", "--screen-byzantine", "1", "--screen-keep", "3")
    assert r.returncode == 0 and "5 simulated clients (torch): 3 rounds" in r.stdout, r.stderr[-2000:]
    for args, msg in ((("--screen", "multi_krum", "--wide"), "--screen is not supported with --wide"),
                      (("--screen", "multi_krum", "--secagg"), "secagg"),
                      (("--screen", "multi_krum", "--dp-clip", "1.0"), "differential privacy"),
                      (("--screen", "multi_krum", "--aggregator", "median", "--gather-plane", "xgmi"), "one-shot select kernel"),
                      (("--screen", "multi_krum", "--screen-byzantine", "-1"), "screen_byzantine"),
                      (("--screen", "multi_krum", "--screen-keep", "0"), "screen_keep"),
                      (("--screen", "krum"), "invalid choice"),
                      (("--clients", "4", "--rounds", "2", "--screen", "multi_krum", "--screen-byzantine", "1"), "2 f + 3")):
        r = run(*args)
        assert r.returncode != 0 and msg in r.stderr, (args, r.stderr[-500:])
