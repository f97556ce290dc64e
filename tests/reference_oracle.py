"""Literal re-implementation of the reference [C] client math for tests (the reference
script itself imports mpi4py, which is not installable here).  Mirrors
FL_CustomMLPCLassifierImplementation_Multiple_Rounds.py:12-25 (MLPModel), :63-73
(train_one_epoch), :75-91 (evaluate_local), :101-120 (federated_averaging arithmetic)."""
import numpy as np
import torch
import torch.nn as nn
import torch.optim as optim


class RefMLP(nn.Module):
    def __init__(self, input_size, hidden_sizes, output_size):
        super().__init__()
        layers, in_size = [], input_size
        for h in hidden_sizes:
            layers += [nn.Linear(in_size, h), nn.ReLU()]
            in_size = h
        layers.append(nn.Linear(in_size, output_size))
        self.model = nn.Sequential(*layers)

    def forward(self, x):
        return self.model(x)


class RefClient:
    def __init__(self, X, y, hidden, n_classes, flat_init, lr=0.004):
        from fedmi.models.mlp import flat_to_dict
        self.X = torch.tensor(X, dtype=torch.float32)
        self.y = torch.tensor(y, dtype=torch.long)
        self.model = RefMLP(X.shape[1], hidden, n_classes)
        dims = [X.shape[1], *hidden, n_classes]
        sd = {k: torch.tensor(v) for k, v in flat_to_dict(flat_init, dims).items()}
        self.model.load_state_dict(sd)
        self.criterion = nn.CrossEntropyLoss()
        self.optimizer = optim.Adam(self.model.parameters(), lr=lr)
        self.scheduler = optim.lr_scheduler.StepLR(self.optimizer, step_size=30, gamma=0.5)

    def train_one_epoch(self):
        self.model.train()
        self.optimizer.zero_grad()
        loss = self.criterion(self.model(self.X), self.y)
        loss.backward()
        self.optimizer.step()
        self.scheduler.step()

    def predictions(self):
        self.model.eval()
        with torch.no_grad():
            _, p = torch.max(self.model(self.X), 1)
        return p.numpy()

    def get_weights(self):
        return {n: p.clone().detach().cpu().numpy() for n, p in self.model.named_parameters()}

    def set_weights(self, w):
        with torch.no_grad():
            for n, p in self.model.named_parameters():
                p.copy_(torch.tensor(w[n], dtype=torch.float32))


# Shapes of the fused round kernels off the income shape, shared by tests/test_hip_engine_shapes.py
# (HIP vs oracle) and tests/test_oracle_noise.py (the oracle's own noise): (rows, F, C, hidden).
SHAPE_CASES = [
    (300, 14, 3, (50, 200)),     # smallest general-CE case
    (300, 14, 5, (33, 17, 9)),   # swizzled rows keep their logits in columns 4..7
    (400, 14, 16, (40,)),        # FL_MAX_CLASSES, full tile
    (300, 1, 2, (16,)),          # F = 1
    (300, 17, 3, (16, 16)),      # second 16-chunk of features
    (300, 33, 2, (65,)),         # second 16-chunk, odd hidden tile
    (5, 14, 2, (50, 200)),       # n_rows < R, one partial workgroup
    (33, 14, 3, (7,)),           # R + 1 rows at R = 32
    (32, 14, 2, (7,)),           # exactly one full workgroup at R = 32, two at 16
]
# Optimizer settings off the defaults: (id, rows, F, C, hidden, EngineConfig overrides)
OPT_CASES = [
    ("weight_decay", 300, 14, 2, (50, 200), dict(weight_decay=1e-2)),
    ("steplr", 300, 14, 2, (50, 200), dict(step_size=2, gamma=0.3)),
    ("betas_eps_lr", 300, 14, 2, (50, 200), dict(betas=(0.5, 0.9), eps=1e-3, lr=0.02)),
    ("all", 300, 17, 5, (33, 17), dict(weight_decay=1e-2, step_size=2, gamma=0.3, betas=(0.8, 0.99), eps=1e-6,
                                       local_steps=2, prox_mu=0.3)),
]
# bf16 train-kernel gradient: (rows, F, C, hidden, R, slab)
BF16_GRAD_CASES = [
    (300, 14, 3, (50, 200), 32, "fp16"),
    (300, 14, 5, (33, 17, 9), 16, "fp32"),
    (400, 14, 16, (40,), 32, "fp16"),
    (300, 1, 2, (16,), 16, "fp16"),
    (300, 33, 2, (65,), 32, "fp32"),
    (300, 40, 4, (40, 96), 32, "fp16"),
    (5, 14, 2, (50, 200), 64, "fp16"),   # (this model's split-bf16 layout may exceed LDS at R = 64)
    (5, 14, 2, (7,), 64, "fp16"),        # n_rows < R on a model that fits at R = 64
    (33, 14, 3, (7,), 32, "fp32"),
]
# bf16 engine vs fp32 oracle over 60 rounds: (C, EngineConfig overrides).  3000 rows, the size the
# tracking bounds were set at: on 600 rows the fp32 oracle's own final accuracy moves by 0.013 to
# 0.02 between init seeds (tests/test_oracle_noise.py)
BF16_TRACK_CASES = [(3, {}), (2, dict(weight_decay=1e-2))]
BF16_TRACK_ROWS = 3000
DATA_SEED = 3
INIT_SEED = 1


def nerr(a, b):
    """max|a - b| / max|b|: the normalised error of test_round_matches_torch."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def make_multiclass(n, F, C, seed):
    """Gaussian features with labels from a noisy random linear teacher: C roughly balanced
    classes at any feature width (make_income_like is 14 features / 2 classes only)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, F)).astype(np.float32)
    T = rng.standard_normal((F, C)) / np.sqrt(F)
    y = np.argmax(X.astype(np.float64) @ T + 0.5 * rng.standard_normal((n, C)), 1)
    return X, y.astype(np.int64)


def _dense_layers(flat, dims, dtype=torch.float64):
    """[(W [out, in], b [out])] of a dense flat parameter buffer, as ``dtype`` tensors."""
    from fedmi.models.mlp import flat_to_dict
    d = flat_to_dict(flat, dims)
    return [(torch.tensor(d[f"model.{2 * l}.weight"], dtype=dtype), torch.tensor(d[f"model.{2 * l}.bias"], dtype=dtype))
            for l in range(len(dims) - 1)]


def float64_logits(flat, dims, X):
    """Logits of the MLP with dense parameters ``flat`` on rows ``X``, every operation in float64."""
    a = torch.as_tensor(np.asarray(X, np.float32)).to(torch.float64)
    layers = _dense_layers(flat, dims)
    for l, (W, b) in enumerate(layers):
        a = a @ W.T + b
        if l + 1 < len(layers):
            a = torch.relu(a)
    return a.numpy()


class Float64RoundOracle:
    """One client's round of ``TorchRoundEngine`` (full-batch CE, ``local_steps`` steps with the
    FedProx term, ``torch.optim.Adam``, ``StepLR`` stepped once per round; FedAvg of one client is
    the identity) with every tensor in float64, from the same dense ``init_flat``.  The yardstick
    for the fp32 oracle's own rounding noise."""

    def __init__(self, X, y, n_classes, cfg, init_flat):
        self.cfg = cfg
        self.dims = [int(X.shape[1]), *[int(h) for h in cfg.hidden], int(n_classes)]
        self.X = torch.as_tensor(np.asarray(X, np.float32)).to(torch.float64)
        self.y = torch.as_tensor(np.asarray(y), dtype=torch.long)
        self.params = []
        for W, b in _dense_layers(init_flat, self.dims):
            self.params += [W.requires_grad_(), b.requires_grad_()]
        self.optimizer = optim.Adam(self.params, lr=cfg.lr, betas=tuple(cfg.betas), eps=cfg.eps,
                                    weight_decay=cfg.weight_decay)
        self.scheduler = optim.lr_scheduler.StepLR(self.optimizer, step_size=cfg.step_size, gamma=cfg.gamma)
        self.loss = []

    def _forward(self):
        a = self.X
        for l in range(0, len(self.params), 2):
            a = a @ self.params[l].T + self.params[l + 1]
            if l + 2 < len(self.params):
                a = torch.relu(a)
        return a

    def run(self, n_rounds):
        cfg = self.cfg
        for _ in range(n_rounds):
            anchor = [p.detach().clone() for p in self.params]
            for _ in range(cfg.local_steps):
                self.optimizer.zero_grad()
                loss = nn.functional.cross_entropy(self._forward(), self.y)
                loss.backward()
                if cfg.prox_mu:
                    with torch.no_grad():
                        for p, a in zip(self.params, anchor):
                            p.grad.add_(cfg.prox_mu * (p.detach() - a))
                self.optimizer.step()
            self.scheduler.step()
            self.loss.append(float(loss.detach()))

    def _cat(self, ts):
        return torch.cat([t.detach().reshape(-1) for t in ts]).numpy()

    def weights(self):
        return self._cat(self.params)

    def exp_avg(self):
        return self._cat([self.optimizer.state[p]["exp_avg"] for p in self.params])

    def exp_avg_sq(self):
        return self._cat([self.optimizer.state[p]["exp_avg_sq"] for p in self.params])

    def result(self):
        """(dense weights, exp_avg, exp_avg_sq, per-round loss), float64."""
        return self.weights(), self.exp_avg(), self.exp_avg_sq(), np.asarray(self.loss, np.float64)


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float64)


def _bf16_forward(flat, X, dims, plain=False, pre_out=None):
    """Forward pass of the bf16 kernels (fl_kernels_bf16.hip) in float64: every layer multiplies the
    bf16 parts of its input and weights, x_hi = bf16(x), x_lo = bf16(x - x_hi) -- split-bf16
    hi.hi + (lo.hi + hi.lo), or with ``plain`` hi.hi alone (FLConfig::plain_fwd) -- and adds the
    fp32 bias; hidden outputs are rounded to fp32 after ReLU and split again.  Returns (Ws, the hi
    part of every layer's input, the logits).  ``pre_out``: a list that receives every hidden layer's
    pre-activations (tests/train_stage_oracle.py: the model's ReLU margin)."""
    from fedmi.models.mlp import flat_to_dict
    d = flat_to_dict(flat, dims)
    L = len(dims) - 1
    Ws = [torch.as_tensor(d[f"model.{2 * l}.weight"], dtype=torch.float64) for l in range(L)]
    bs = [torch.as_tensor(d[f"model.{2 * l}.bias"], dtype=torch.float64) for l in range(L)]
    a = torch.as_tensor(X, dtype=torch.float32).to(torch.float64)
    his = []
    for l in range(L):
        ah, wh = _bf(a), _bf(Ws[l])
        if plain:
            z = ah @ wh.T + bs[l]
        else:
            al, wl = _bf(a - ah), _bf(Ws[l] - wh)
            z = ah @ wh.T + (al @ wh.T + ah @ wl.T) + bs[l]
        his.append(ah)
        if pre_out is not None and l + 1 < L:
            pre_out.append(z)
        a = torch.relu(z).to(torch.float32).to(torch.float64)
    return Ws, his, z


def _split_bf16_reference_grad(flat, X, y, dims, scaled_delta=False, plain=False, n_div=None):
    """Host model of the bf16 train kernel's arithmetic (fl_kernels_bf16.hip), in float64:
    split-bf16 forward (hi.hi + lo.hi + hi.lo, hidden outputs split into hi/lo after ReLU; with
    ``plain`` the hi.hi forward of several clients' training pass), softmax-CE deltas rounded to
    bf16, backward on the hi parts with bf16 deltas.  ``n_div``: the mean's divisor (default: the
    rows given) -- one workgroup's rows with the whole shard's n give that workgroup's slab row
    (tests/train_stage_oracle.py), and n_div = 1 without ``scaled_delta`` the fp16 slab's unscaled sums."""
    L = len(dims) - 1
    Ws, his, z = _bf16_forward(flat, X, dims, plain)
    yt = torch.as_tensor(y, dtype=torch.long)
    n = len(y)
    p = torch.softmax(z, 1)
    dz = p.clone()
    dz[torch.arange(n), yt] -= 1.0
    # fp16 slab: the kernels back-propagate the unscaled delta (Adam applies the 1/n); fp32
    # slab: the delta of the mean loss
    div = float(n if n_div is None else n_div)
    sc = 1.0 if scaled_delta else div
    dz = _bf(dz / div) if scaled_delta else _bf(dz)
    gW, gb = [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        gW[l] = dz.T @ his[l] / sc
        gb[l] = dz.sum(0) / sc
        if l:
            dz = _bf((dz @ _bf(Ws[l])) * (his[l] > 0))
    return torch.cat([torch.cat([gW[l].reshape(-1), gb[l]]) for l in range(L)]).numpy()


def fedavg(weights, sizes):
    """C:110-116 root arithmetic."""
    total = sum(sizes)
    return {k: sum(weights[i][k] * sizes[i] / total for i in range(len(weights))) for k in weights[0]}
