"""Byzantine attack models without a GPU (fedmi/fl/attack.py): the configuration rules, the numpy model of the
kernels (``attack_model``) against a straightforward float64 evaluation of the rule, the bitwise properties
of the rule, the closed form of IPM under the mean, label flipping, and torch client groups against the same
groups driven through ``tamper``.

Operation counts of the bound in ``test_model_against_a_float64_evaluation`` (every fp32 operation of a chain
adds at most half an ulp, 2^-24, of its own result; the bound is the count times 2^-24 of the largest
intermediate magnitude of the coordinate, taken from the float64 evaluation).  ``h = |H_r|``; the weighted
mode adds one division per model that enters (``m_j = c_j / w_j``) and the final product ``w_k a_k``:

* ``sign_flip``: sub, mul, sub = 3; weighted 3 + 1 + 1 = 5.
* ``gauss``: the fp32 rounding of the float64 normal, mul, add = 3; weighted 5.
* ``ipm``: mu = h additions + 1 division; sub, mul, sub = h + 4; weighted h + 4 + h + 1 = 2 h + 5.
* ``alie``: mu = h + 1; var = per honest client sub, mul, add = 3 h, + 1 division; sqrt, mul, sub = 3:
  4 h + 5; weighted 4 h + 5 + h + 1 = 5 h + 6.  var is a sum of squares, so nothing cancels in it: the error of
  sqrt(var) is of the order of the errors of the d_j, each a few 2^-24 of |m_j| (magnitude about 1, the largest
  intermediate), however small var itself is; the honest values are drawn with a spread of 0.3 and var > 0.

Measured on the cases below (error / bound, worst coordinate, unweighted / weighted): sign_flip 0.45 / 0.11,
gauss 0.49 / 0.13, ipm 0.20 / 0.05, alie 0.07 / 0.02.

The closed form: ``ClientGroup(backend="torch")`` keeps its contribution rows in fp32, so the float64 group of
the closed-form test is the group's own arithmetic (``attack_torch``, then the sum in rank order) applied in
float64 to the rows a real torch group published; the fp32 group's aggregate is held to the same closed form
with a bound derived from its operation count.
"""
import functools

import numpy as np
import pytest
import torch

from fedmi.fl.attack import (ATTACKS, alie_z, attack_id, attack_model, attack_normals, attack_params, attack_torch)
from fedmi.fl.engine import EngineConfig, HipRoundEngine, TorchRoundEngine, attack_stage
from fedmi.fl.simulate import ClientGroup, SimRank
from fedmi.models.mlp import dense_to_image, image_layout, image_to_dense, init_flat, param_count
from fedmi.privacy.philox import ATTACK_STREAM, DP_STREAM, QSGD_STREAM, RANDK_STREAM

from .reference_oracle import DATA_SEED, make_multiclass

SMALL = [17, 24, 3]
TAILS = 7
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _real(dims):
    return dense_to_image(np.ones(param_count(list(dims)), np.float32), list(dims)) != 0


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- configuration ----
def test_defaults_and_fields():
    d = EngineConfig()
    assert ATTACKS == ("none", "sign_flip", "gauss", "alie", "ipm", "label_flip")
    assert (d.attack, tuple(d.attack_clients), d.attack_scale, d.attack_z, d.attack_seed) == ("none", (), 1.0, None, 0)
    assert attack_id(d) == 0 and attack_id(d, 7) == 0 and not attack_stage(d)
    on = EngineConfig(attack="alie", attack_clients=(1, 4))
    assert attack_id(on) == 3 and attack_id(on, 7) == 3 and attack_stage(on, 7)
    assert {"attack", "attack_clients", "attack_scale", "attack_z", "attack_seed"} <= set(on.to_dict())
    assert attack_id(EngineConfig(attack="label_flip", attack_clients=[0]), 2) == 5
    assert not attack_stage(EngineConfig(attack="label_flip", attack_clients=[0]), 2)
    assert len({ATTACK_STREAM, DP_STREAM, QSGD_STREAM, RANDK_STREAM, 0x47414353}) == 5


@pytest.mark.parametrize("kw, world, field", [
    (dict(attack="krum"), None, "attack must be"),
    (dict(attack=3), None, "attack must be"),
    (dict(attack="alie"), None, "attack_clients"),                                # empty while on
    (dict(attack="alie", attack_clients=(1, 1)), None, "attack_clients must be distinct"),
    (dict(attack="alie", attack_clients=(-1,)), None, "attack_clients"),
    (dict(attack="alie", attack_clients=(1.5,)), None, "attack_clients"),
    (dict(attack="alie", attack_clients="14"), None, "attack_clients"),
    (dict(attack="alie", attack_clients=(7,)), 7, r"attack_clients must lie in \[0, 7\)"),
    (dict(attack="ipm", attack_clients=(0, 1, 2)), 3, "attack_clients must leave at least one client honest"),
    (dict(attack="ipm", attack_clients=(0,), attack_scale=0.0), None, "attack_scale"),
    (dict(attack="ipm", attack_clients=(0,), attack_scale=-1.0), None, "attack_scale"),
    (dict(attack="ipm", attack_clients=(0,), attack_scale=float("nan")), None, "attack_scale"),
    (dict(attack="ipm", attack_clients=(0,), attack_scale=float("inf")), None, "attack_scale"),
    (dict(attack="ipm", attack_clients=(0,), attack_scale=1e-60), None, "attack_scale"),   # 0 in fp32
    (dict(attack="ipm", attack_clients=(0,), attack_scale=1e60), None, "attack_scale"),    # inf in fp32
    (dict(attack_scale="big"), None, "attack_scale"),                              # validated while off, too
    (dict(attack="alie", attack_clients=(0,), attack_z=float("nan")), None, "attack_z"),
    (dict(attack="alie", attack_clients=(0,), attack_z=float("inf")), None, "attack_z"),
    (dict(attack="gauss", attack_clients=(0,), attack_seed=-1), None, "attack_seed"),
    (dict(attack="gauss", attack_clients=(0,), attack_seed=2 ** 64), None, "attack_seed"),
    (dict(attack="gauss", attack_clients=(0,), attack_seed=1.0), None, "attack_seed"),
    (dict(attack="alie", attack_clients=(0,)), 2, "attack_z"),     # n = 2, f = 1: the ratio is 0
    (dict(attack="alie", attack_clients=(0, 1, 2, 3)), 7, "attack_z"),   # s = 0: the ratio is 1
])
def test_attack_id_refusals_name_the_field(kw, world, field):
    with pytest.raises(ValueError, match=field):
        attack_id(EngineConfig(**kw), world)


def test_default_z_is_the_papers_formula():
    from statistics import NormalDist
    assert alie_z(7, 2) == NormalDist().inv_cdf(0.6) and abs(alie_z(7, 2) - 0.2533) < 1e-4
    assert alie_z(8, 2) == NormalDist().inv_cdf((8 - 2 - 3) / (8 - 2))   # s = 8 // 2 + 1 - 2 = 3: Phi^-1(0.5) = 0
    par = attack_params(EngineConfig(attack="alie", attack_clients=(1, 4)), 7)
    assert par == {"kind": "alie", "clients": [1, 4], "scale": 1.0, "z": float(np.float32(NormalDist().inv_cdf(0.6)))}
    assert attack_params(EngineConfig(attack="alie", attack_clients=(1,), attack_z=1.5), 7)["z"] == 1.5
    for n, f in ((2, 1), (7, 4), (4, 3)):
        with pytest.raises(ValueError, match="attack_z"):
            alie_z(n, f)
    # an explicit z lifts the refusal; one client switches the attack off and refuses nothing
    assert attack_id(EngineConfig(attack="alie", attack_clients=(0,), attack_z=1.0), 2) == 3
    assert attack_id(EngineConfig(attack="alie", attack_clients=(5,)), 1) == 0


# ---- the model against a float64 evaluation of the rule ----
K = 5
ACTIVE = [True, True, False, True, True]    # client 2 is not sampled
SCALE, Z = 0.75, 0.25


def _case(dims, seed, weighted):
    """([K, Pimg + TAILS] contributions, x, real, weights or None): models 1 + 0.3 N(0, I) on the real parameters,
    sentinels in the padding and the tails; weighted: c_j = w_j m_j with the weights of unequal shards."""
    pimg = image_layout(dims)[2]
    real = _real(tuple(dims))
    rng = np.random.default_rng(seed)
    m = (1.0 + 0.3 * rng.standard_normal((K, pimg))).astype(np.float32)
    x = (1.0 + 0.3 * rng.standard_normal(pimg)).astype(np.float32)
    x[~real] = 0.0
    w = None
    if weighted:
        sizes = np.array([50, 70, 40, 30, 90], np.float64)
        w = (sizes / sizes[ACTIVE].sum()).astype(np.float32)
        w[2] = 0.0
        m = m * w[:, None]
    a = np.empty((K, pimg + TAILS), np.float32)
    a[:, :pimg] = m
    a[:, :pimg][:, ~real] = -77.0
    a[:, pimg:] = 5.0 + rng.standard_normal((K, TAILS)).astype(np.float32)
    return a, x, real, w


def _rule64(kind, a, x, real, w, bad, dims, seed=3, rnd=2):
    """{bad sampled client: (a_k in float64 [Pimg], largest intermediate magnitude [Pimg])}: the rule of
    fedmi/fl/attack.py written out in float64."""
    pimg = real.shape[0]
    c = a[:, :pimg].astype(np.float64)
    w64 = np.ones(K) if w is None else w.astype(np.float64)
    x64 = x.astype(np.float64)
    B = [k for k in range(K) if ACTIVE[k] and k in bad]
    H = [k for k in range(K) if ACTIVE[k] and k not in bad]
    mods = {j: c[j] / w64[j] for j in B + H}
    mag = np.zeros(pimg)

    def see(*vs):
        nonlocal mag
        for v in vs:
            mag = np.maximum(mag, np.abs(v))

    out = {}
    if kind in ("alie", "ipm"):
        s = np.zeros(pimg)
        for j in H:
            s = s + mods[j]
            see(mods[j], s)
        mu = s / len(H)
        if kind == "alie":
            v = np.zeros(pimg)
            for j in H:
                d = mods[j] - mu
                v = v + d * d
                see(d, v)
            v = v / (len(H) - 1) if len(H) >= 2 else v
            ak = mu - Z * np.sqrt(v)
            see(np.sqrt(v), Z * np.sqrt(v))
        else:
            ak = x64 - SCALE * (mu - x64)
            see(mu - x64, SCALE * (mu - x64), x64)
        for k in B:
            see(ak, w64[k] * ak)
            out[k] = w64[k] * ak
        return out, mag
    pos = dense_to_image(np.arange(1, param_count(dims) + 1), dims).astype(np.int64) - 1
    for k in B:
        if kind == "sign_flip":
            ak = x64 - SCALE * (mods[k] - x64)
            see(mods[k], mods[k] - x64, SCALE * (mods[k] - x64), x64, ak)
        else:
            n = np.zeros(pimg)
            n[pos >= 0] = attack_normals(param_count(dims), rnd, k, seed)[pos[pos >= 0]]
            ak = mods[k] + SCALE * n
            see(mods[k], n, SCALE * n, ak)
        see(w64[k] * ak)
        out[k] = w64[k] * ak
    return out, mag


def _ops(kind, h, weighted):
    return {"sign_flip": (3, 5), "gauss": (3, 5), "ipm": (h + 4, 2 * h + 5), "alie": (4 * h + 5, 5 * h + 6)}[kind][weighted]


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("kind", ["sign_flip", "gauss", "alie", "ipm"])
def test_model_against_a_float64_evaluation(kind, weighted):
    worst = 0.0
    for seed, bad in ((0, (1, 2)), (1, (1, 3)), (2, (0,))):
        a, x, real, w = _case(SMALL, seed, weighted)
        got = attack_model(a, x, ACTIVE, bad, kind, SCALE, Z, real, weights=w, seed=3, round=2, dims=SMALL)
        ref, mag = _rule64(kind, a, x, real, w, bad, SMALL)
        h = sum(1 for k in range(K) if ACTIVE[k] and k not in bad)
        assert ref and h >= 2
        pimg = real.shape[0]
        for k, r64 in ref.items():
            err = np.abs(got[k, :pimg].astype(np.float64) - r64)[real]
            bound = _ops(kind, h, weighted) * U * mag[real]
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (kind, weighted, seed, k, float((err / bound).max()))
            assert (err > 0).any()   # (an fp32 chain: not the float64 numbers themselves)
        if kind == "alie":
            d = np.stack([a[j, :pimg] / (1 if w is None else w[j]) for j in range(K) if ACTIVE[j] and j not in bad])
            assert (d.var(0, ddof=1)[real] > 0).all()
    print(f"{kind} {'weighted' if weighted else 'unweighted'}: worst error / bound {worst:.3g}")


# ---- bitwise properties of the rule ----
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("kind", ["sign_flip", "gauss", "alie", "ipm"])
def test_what_is_never_written(kind, weighted):
    a, x, real, w = _case(SMALL, 4, weighted)
    pimg = real.shape[0]
    run = lambda active, bad, **kw: attack_model(a, x, active, bad, kind, SCALE, Z, real, weights=w, seed=3, round=2,
                                                 dims=SMALL, **kw)
    got = run(ACTIVE, (1, 2, 3))
    assert got is not a and got.dtype == np.float32
    for k in (1, 3):                                                                  # bad and sampled: rewritten ...
        assert (_bits(got[k, :pimg][real]) != _bits(a[k, :pimg][real])).mean() > 0.9
        np.testing.assert_array_equal(_bits(got[k, :pimg][~real]), _bits(a[k, :pimg][~real]))   # ... never the padding
        np.testing.assert_array_equal(_bits(got[k, pimg:]), _bits(a[k, pimg:]))                   # ... nor the tails
    for k in (0, 4, 2):                                                               # honest rows; the unsampled bad row
        np.testing.assert_array_equal(_bits(got[k]), _bits(a[k]))
    # the no-ops: not live, B_r empty, and (colluding kinds) H_r empty
    np.testing.assert_array_equal(_bits(run(ACTIVE, (1, 3), live=False)), _bits(a))
    np.testing.assert_array_equal(_bits(run(ACTIVE, (2,))), _bits(a))
    np.testing.assert_array_equal(_bits(run([False] * K, (1, 3))), _bits(a))
    all_bad = run(ACTIVE, (0, 1, 3, 4))
    if kind in ("alie", "ipm"):
        np.testing.assert_array_equal(_bits(all_bad), _bits(a))
    else:
        assert (_bits(all_bad[0, :pimg][real]) != _bits(a[0, :pimg][real])).any()   # the own-buffer kinds need no honest client
    # flags and indices name the same clients
    np.testing.assert_array_equal(_bits(run(ACTIVE, [False, True, True, True, False])), _bits(got))
    np.testing.assert_array_equal(_bits(run([0, 1, 3, 4], (1, 2, 3))), _bits(got))


@pytest.mark.parametrize("kind", ["alie", "ipm"])
def test_colluding_clients_publish_one_vector(kind):
    a, x, real, _ = _case(SMALL, 5, False)
    pimg = real.shape[0]
    got = attack_model(a, x, ACTIVE, (1, 3), kind, SCALE, Z, real)
    np.testing.assert_array_equal(_bits(got[1, :pimg][real]), _bits(got[3, :pimg][real]))
    # weighted: the same model behind both contributions, each scaled by its own weight
    a, x, real, w = _case(SMALL, 5, True)
    got = attack_model(a, x, ACTIVE, (1, 3), kind, SCALE, Z, real, weights=w)
    H = [0, 4]
    mu = (a[0, :pimg] / w[0] + a[4, :pimg] / w[4]) / np.float32(len(H))
    if kind == "ipm":
        vec = x - np.float32(SCALE) * (mu - x)
    else:
        var = np.zeros(pimg, np.float32)
        for j in H:
            d = a[j, :pimg] / w[j] - mu
            var = var + d * d
        vec = mu - np.float32(Z) * np.sqrt(var / np.float32(1.0))
    for k in (1, 3):
        np.testing.assert_array_equal(_bits(got[k, :pimg][real]), _bits((w[k] * vec)[real]))


def test_one_honest_client_gives_zero_variance():
    a, x, real, _ = _case(SMALL, 6, False)
    pimg = real.shape[0]
    active = [True, True, False, True, False]
    got = attack_model(a, x, active, (1, 3), "alie", SCALE, 5.0, real)
    for k in (1, 3):   # mu = the one honest model, var = 0: a = mu - z * 0 = mu, whatever z
        np.testing.assert_array_equal(_bits(got[k, :pimg][real]), _bits(a[0, :pimg][real]))


def test_nan_in_an_honest_client_propagates():
    a, x, real, _ = _case(SMALL, 7, False)
    pimg = real.shape[0]
    hole = int(np.flatnonzero(real)[5])
    a[4, hole] = np.nan
    for kind in ("alie", "ipm"):
        got = attack_model(a, x, ACTIVE, (1,), kind, SCALE, Z, real)
        assert np.isnan(got[1, hole]) and np.isfinite(np.delete(got[1, :pimg][real], 5)).all()


def test_gauss_draws_differ_by_round_and_client():
    P = param_count(SMALL)
    n = attack_normals(P, 0, 1, 9)
    assert n.shape == (P,) and abs(n.mean()) < 0.15 and abs(n.std() - 1.0) < 0.1
    assert not np.array_equal(n, attack_normals(P, 1, 1, 9)) and not np.array_equal(n, attack_normals(P, 0, 3, 9))
    assert not np.array_equal(n, attack_normals(P, 0, 1, 10))
    from fedmi.privacy.philox import dp_normals
    assert not np.array_equal(n, dp_normals(P, 0, 1, 9))   # a stream of its own
    np.testing.assert_array_equal(n, attack_normals(P, 0, 1, 9))


def test_attack_torch_is_the_model_on_dense_rows():
    """fp32 rows: bit for bit the image model read back in dense order (deterministic kinds)."""
    P = param_count(SMALL)
    for weighted in (False, True):
        a, x, real, w = _case(SMALL, 8, weighted)
        pimg = real.shape[0]
        for kind in ("sign_flip", "alie", "ipm"):
            model = attack_model(a, x, ACTIVE, (1, 2, 3), kind, SCALE, Z, real, weights=w)
            rows = [torch.cat([torch.as_tensor(image_to_dense(r[:pimg], SMALL)), torch.as_tensor(r[pimg:])]) for r in a]
            attack_torch(rows, torch.as_tensor(image_to_dense(x, SMALL)), ACTIVE, (1, 2, 3), kind, SCALE, Z, P,
                         weights=None if w is None else [float(v) for v in w])
            for k in range(K):
                np.testing.assert_array_equal(_bits(rows[k][:P].numpy()), _bits(image_to_dense(model[k, :pimg], SMALL)))
                np.testing.assert_array_equal(_bits(rows[k][P:].numpy()), _bits(a[k, pimg:]))


# ---- torch groups ----
ROUNDS = 3
BAD = (1, 4)


def _cfg(**kw):
    return EngineConfig(**{**dict(hidden=(24,), max_rounds=ROUNDS + 2, early_stop=False, graph_rounds=0), **kw})


@functools.lru_cache(maxsize=None)
def _data():
    return make_multiclass(240, 17, 3, DATA_SEED)


def _group(k=7, tamper=None, common=False, **kw):
    X, y = _data()
    torch.set_num_threads(1)
    g = ClientGroup(X, y, k, _cfg(**kw), backend="torch", shard_mode="iid", seed=2, tamper=tamper)
    if common:   # the common initial model an attacked group starts from
        for c in g.clients:
            c.set_global_flat(init_flat(SMALL, 2 * 1000003))
    return g


def test_closed_form_of_ipm_under_the_mean():
    """Equal shards, f of K clients bad, one round: the mean of the contributions is
    x + ((K - f - f eps) / K) (mu_H - x)."""
    Kc, bad, eps = 4, (2,), 0.5
    seen = {}

    def grab(r, bufs):
        seen["rows"] = [b.clone() for b in bufs]

    g = _group(k=Kc, tamper=grab, attack="ipm", attack_clients=bad, attack_scale=eps)
    sizes = [c.n_local for c in g.clients]
    assert len(set(sizes)) == 1
    P = g.clients[0].P
    x = init_flat(SMALL, 2 * 1000003).astype(np.float64)
    np.testing.assert_array_equal(g.global_flat(), x.astype(np.float32))   # one common initial model
    assert g.run(1) == 1
    w = 1.0 / Kc
    rows64 = [r.double() for r in seen["rows"]]
    H = [k for k in range(Kc) if k not in bad]
    mu = sum(rows64[j][:P].numpy() / w for j in H) / len(H)
    form = x + ((Kc - len(bad) - len(bad) * eps) / Kc) * (mu - x)
    # the group's arithmetic in float64: the stage, then the sum in rank order
    attack_torch(rows64, torch.as_tensor(x), [True] * Kc, bad, "ipm", eps, 0.0, P, weights=[w] * Kc)
    tot = rows64[0][:P].clone()
    for r in rows64[1:]:
        tot += r[:P]
    scale = np.abs(np.stack([x, mu])).max()
    err64 = np.abs(tot.numpy() - form).max()
    print(f"ipm closed form: float64 evaluation {err64:.3g} (scale {scale:.3g})")
    assert err64 <= 16 * 2.0 ** -53 * scale
    # the fp32 group itself: h divisions + h additions + 1 division (mu), sub, mul, sub, the product by w, the
    # honest rows' own product by w (1) and K - 1 additions of the sum: 2 h + 5 + 1 + K - 1 = 15 operations
    err32 = np.abs(g.global_flat().astype(np.float64) - form).max()
    print(f"ipm closed form: fp32 group {err32:.3g}")
    assert err32 <= (2 * len(H) + 5 + Kc) * U * scale


def test_label_flip_poisons_the_bad_shards_only():
    clean = _group(k=4)
    g = _group(k=4, attack="label_flip", attack_clients=(1,))
    C = 3
    for k, (c, d) in enumerate(zip(g.clients, clean.clients)):
        np.testing.assert_array_equal(c.X.numpy(), d.X.numpy())
        want = (C - 1 - d.y.numpy()) if k == 1 else d.y.numpy()
        np.testing.assert_array_equal(c.y.numpy(), want)
        assert not c.attack_stage and c.attack == 5
    # label flipping is no stage: every client keeps its own initial model
    assert not np.array_equal(g.clients[0].global_flat(), g.clients[1].global_flat())
    assert g.run(ROUNDS) == ROUNDS and np.isfinite(g.global_flat()).all()
    clean.run(ROUNDS)
    assert not np.array_equal(g.global_flat(), clean.global_flat())


@pytest.mark.parametrize("kw", [dict(attack="sign_flip", attack_scale=2.0),
                                dict(attack="alie", aggregator="median"),
                                dict(attack="ipm", attack_scale=0.5, participation=0.7),
                                dict(attack="sign_flip", secagg=True, secagg_seed=5)],
                         ids=["sign_flip-mean", "alie-median", "ipm-mean-sampled", "sign_flip-secagg"])
def test_torch_group_equals_the_group_driven_through_tamper(kw):
    g = _group(attack_clients=BAD, **kw)
    assert g.clients[0].attack_stage
    for c in g.clients[1:]:
        np.testing.assert_array_equal(c.global_flat(), g.clients[0].global_flat())   # one common initial model
    plain = {k: v for k, v in kw.items() if not k.startswith("attack")}
    holder = {}

    def tamper(r, bufs):
        lead = holder["g"].clients[0]
        part = [int(k) for k in lead.participants(r)]
        if lead.robust:
            w = None
        elif lead.secagg:
            w = [float(np.float32(c.fedavg_weight(r))) for c in holder["g"].clients]
        elif float(lead.cfg.participation) < 1.0:
            w = [float(c.n_local) for c in holder["g"].clients]
        else:
            w = [float(c.n_local) / float(lead.n_total) for c in holder["g"].clients]
        par = attack_params(g.clients[0].cfg, 7)
        attack_torch(bufs, lead.global_params.detach().clone(), [k in part for k in range(7)], BAD, par["kind"],
                     par["scale"], par["z"], lead.P, weights=w, round=r)

    ref = holder["g"] = _group(tamper=tamper, common=True, **plain)
    assert not ref.clients[0].attack_stage
    assert g.run(ROUNDS) == ROUNDS and ref.run(ROUNDS) == ROUNDS
    np.testing.assert_array_equal(g.global_flat(), ref.global_flat())
    for key in ("global", "loss", "per_rank"):
        np.testing.assert_array_equal(g.history()[key], ref.history()[key])
    clean = _group(common=True, **plain)
    clean.run(ROUNDS)
    assert not np.array_equal(g.global_flat(), clean.global_flat())   # the attack did something


def test_attack_off_is_the_group_as_it_was():
    """attack="none" with the other fields set: weights and history of the group built without the fields."""
    a = _group(k=4)
    b = _group(k=4, attack="none", attack_scale=3.0, attack_z=1.0, attack_seed=5)
    a.run(ROUNDS), b.run(ROUNDS)
    np.testing.assert_array_equal(a.global_flat(), b.global_flat())
    assert set(a.history()) == set(b.history())
    assert "attack" not in EngineConfig().to_dict()   # a checkpoint's config record is what it was


# ---- refusals of the engines (no GPU: they precede every device call) ----
def test_engine_refusals():
    X, y = _data()
    flat = init_flat(SMALL, 0)

    class Rank:   # a rank of its own (not a ClientGroup's)
        def __init__(self, size):
            self.size, self.rank, self.device = size, 0, torch.device("cpu")

    mk = lambda comm, **kw: TorchRoundEngine(X, y, 3, _cfg(**kw), comm, flat, n_total=len(X) * comm.size,
                                             client_sizes=[len(X)] * comm.size)
    on = dict(attack="ipm", attack_clients=(1,))
    with pytest.raises(ValueError, match="attack='ipm'.*plain mean"):
        mk(Rank(3), **on)
    with pytest.raises(ValueError, match="attack='ipm'.*secagg"):
        mk(Rank(3), secagg=True, secagg_seed=1, **on)
    assert mk(Rank(3), aggregator="median", **on).attack_stage                       # the host gather of a robust rule
    assert mk(Rank(3), screen="multi_krum", **{**on, "attack_clients": (1,)}, screen_byzantine=0).attack_stage
    assert mk(SimRank(3, 0, "cpu"), **on).attack_stage                               # a group's client: every rule
    assert not mk(Rank(3), attack="label_flip", attack_clients=(1,)).attack_stage    # label_flip: every plane
    with pytest.raises(ValueError, match="attack='ipm' takes at most 64 clients"):
        mk(SimRank(65, 0, "cpu"), **on)
    with pytest.raises(ValueError, match=r"attack_clients must lie in \[0, 3\)"):
        mk(SimRank(3, 0, "cpu"), attack="ipm", attack_clients=(3,))
    one = TorchRoundEngine(X, y, 3, _cfg(attack="ipm", attack_clients=(5,)), None, flat)   # one client: off
    assert one.attack == 0 and not one.attack_stage
    with pytest.raises(ValueError, match="comm_buffers.*attack='ipm'"):
        HipRoundEngine(X, y, 3, _cfg(**on), SimRank(3, 0, "cpu"), flat, comm_buffers=(torch.zeros(8), torch.zeros(8)))
    with pytest.raises(ValueError, match="attack='ipm'.*gather_plane='xgmi'"):
        HipRoundEngine(X, y, 3, _cfg(aggregator="median", gather_plane="xgmi", **on), Rank(3), flat)
    from fedmi.hpo.fed_sweep import FedTrialGroup
    with pytest.raises(ValueError, match="fed_sweep.*attack='ipm'"):
        FedTrialGroup(X, y, 3, [], None, _cfg(**on))
    with pytest.raises(ValueError, match="fed_sweep.*attack='label_flip'"):   # nothing there flips labels
        FedTrialGroup(X, y, 3, [], None, _cfg(attack="label_flip", attack_clients=(1,)))
    from fedmi.fl.wide import WideClient
    with pytest.raises(ValueError, match="WideClient.*attack='alie'"):
        WideClient(torch.zeros(4, 4), torch.zeros(4), [4, 8, 2], attack="alie")
    with pytest.raises(ValueError, match="WideClient.*attack='label_flip'"):
        WideClient(torch.zeros(4, 4), torch.zeros(4), [4, 8, 2], attack="label_flip")
