"""Spectral screening (DnC) on the GPU: the fl_dnc kernels against the float64 oracle (fedmi/fl/aggregate.py
dnc_select_ref) on the planted inputs of tests/test_dnc_cpu.py, whose 10 x score margin is asserted there from
the oracle alone, so the kept and bad words must be EQUAL to the oracle's.

Gram bound.  With u = 2^-24 and gamma_m = m u / (1 - m u), entry (i, j) is held to

    |G - G64| <= gamma_m sum_p |c_i| |c_j| + gamma_{K_r + 1} sum_p [(|c_i| + e) |c_j| + |c_i| (|c_j| + e)],
    m = n + chunks + 3,      e[p] = mean_k |v_k[p]|

The first term is the fp32 dot-product bound: n = |R_t| products added in the MFMA's fma chain, 3 cross-wave
additions, `chunks` additions of the select kernel's fold.  The second is the centring's operations, carried
at their own small count: mu is K_r - 1 additions and a division of values of magnitude |v|, off by at most
gamma_{K_r} e[p], and c = v - mu adds one rounding, so |c^ - c| <= gamma_{K_r + 1} (|c| + e) in either factor
(first order).  For models centred at 0 the whole is gamma_{m + 2 K_r + 2} sum |c_i| |c_j|; the planted ones are
not (base 1, spread 0.1), and mu's rounding scales with the base.  Derived, not fitted; the worst measured
error / bound is printed and recorded in docs/ARCHITECTURE.md.
"""
import numpy as np
import pytest
import torch

from fedmi.fl.aggregate import (DNC_SLOT, dnc_chunks, dnc_partial_floats, dnc_scratch_floats, dnc_select_ref,
                                dnc_subset, dnc_threshold, mask_bits)
from fedmi.models.mlp import image_layout

from .reference_oracle import nerr
from .test_dnc_cpu import INCOME, SMALL, _alie_group, planted, planted_bad
from .test_screen import SENTINEL, _rtab, _state, _tab

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = 9


class _Dnc:
    """The two launches over K device rows with caller-owned scratch, as _AggLaunch issues them."""

    def __init__(self, dims, rows, rtab, rounds, f, iters, sub):
        from fedmi.ops import native
        self.m, self.dims, self.K, self.rows = native(), dims, len(rows), rows
        self.args = (f, f, iters)                      # screen_filter 1: q = f
        self.sub, self.rtab, self.rounds, self.iters = sub, rtab, rounds, iters
        self.tab = _tab(rows)
        self.pimg = image_layout(dims)[2]
        assert self.m.dnc_scratch_floats(dims, iters, self.K) == dnc_scratch_floats(self.pimg, iters, self.K)
        self.scratch = torch.full((dnc_scratch_floats(self.pimg, iters, self.K),), -7.0, device=DEV)
        self.keep = torch.full((1,), SENTINEL, dtype=torch.int64, device=DEV)
        self.hist = torch.full((rounds,), SENTINEL, dtype=torch.int64, device=DEV)

    def run(self, state, stream=None):
        s = torch.cuda.current_stream().cuda_stream if stream is None else stream
        self.m.dnc_gram(self.dims, self.tab.data_ptr(), self.K, *self.args, dnc_threshold(self.sub), SEED,
                        self.scratch.data_ptr(), state.data_ptr(), self.rtab.data_ptr(), self.rounds, s)
        self.m.dnc_select(self.dims, self.K, *self.args, self.scratch.data_ptr(), self.keep.data_ptr(),
                          self.hist.data_ptr(), state.data_ptr(), self.rtab.data_ptr(), self.rounds, s)
        if stream is None:
            torch.cuda.synchronize()

    def kept(self):
        return int(self.keep.cpu().numpy().view(np.uint64)[0])

    def record(self, t):
        """Iteration t's record: (scores [K], gram [K, K], kept word, bad word)."""
        base = self.iters * dnc_chunks(self.pimg, self.K) * dnc_partial_floats(self.K) + t * DNC_SLOT
        slot = self.scratch[base:base + DNC_SLOT].cpu().numpy()
        w = slot[128:132].view(np.uint32).astype(np.uint64)
        g = slot[192:].reshape(64, 64)[:self.K, :self.K]
        return slot[:self.K], g, int(w[0] | (w[1] << np.uint64(32))), int(w[2] | (w[3] << np.uint64(32)))


def _rows(a, gathered):
    if gathered:   # rows of one gathered stack, Pimg + tails apart: dword-aligned only (TAILS is odd)
        flat = torch.as_tensor(a.reshape(-1)).to(DEV)
        return [flat[k * a.shape[1]:(k + 1) * a.shape[1]] for k in range(a.shape[0])]
    return [torch.as_tensor(row).to(DEV) for row in a]


@pytest.mark.parametrize("sub", [1.0, 0.5])
@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("K", [3, 16, 17, 64])
@pytest.mark.parametrize("dims", [SMALL, INCOME], ids=["small", "income"])
def test_kernels_against_the_float64_oracle(dims, K, iters, sub):
    a, real, sampled, f, bad, nan = planted(dims, K, 40 + K)
    pimg, r = real.shape[0], 2
    assert pimg % (256 if K <= 32 else 128) != 0          # the last chunk is ragged
    rtab = _rtab([np.ones(K, bool), np.ones(K, bool), sampled])
    kept64, rec64 = dnc_select_ref(a[:, :pimg], sampled, real, f, 1.0, iters, sub, SEED, r, np.float64)
    worst = 0.0
    for gathered in (False, True):
        dn = _Dnc(dims, _rows(a, gathered), rtab, 3, f, iters, sub)
        dn.run(_state(1, r))
        assert dn.kept() == mask_bits(kept64) and dn.kept() & ~mask_bits(sampled) == 0
        hist = dn.hist.cpu().numpy().view(np.uint64)
        assert int(hist[r]) == dn.kept() and int(hist[0]) == int(hist[1]) == SENTINEL
        S = np.flatnonzero(sampled & (np.arange(K) != nan))
        absv = np.abs(a[S, :pimg].astype(np.float64))
        for t in range(iters):
            scores, g, kw, bw = dn.record(t)
            assert kw == mask_bits(rec64[t]["kept"]) and bw == mask_bits(rec64[t]["bad"]) == 1 << nan
            assert np.isinf(scores[nan]) and (scores[~sampled] == 0).all()
            sub_t = dnc_subset(real, sub, SEED, r, t)
            c = np.where(sub_t, np.abs(a[S, :pimg] - a[S, :pimg].astype(np.float64).mean(0)), 0.0)   # |c| over R_t
            ce = c @ np.where(sub_t, c + absv.mean(0), 0.0).T                                       # sum |c_i| (|c_j| + e)
            gamma = lambda m: m * 2.0 ** -24 / (1 - m * 2.0 ** -24)
            bound = gamma(int(sub_t.sum()) + dnc_chunks(pimg, K) + 3) * (c @ c.T) + gamma(len(S) + 1) * (ce + ce.T)
            err = np.abs(g[np.ix_(S, S)].astype(np.float64) - rec64[t]["gram"][np.ix_(S, S)])
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (t, float((err / bound).max()))
            np.testing.assert_array_equal(g, g.T)
    print(f"dnc {dims} K={K} iters={iters} sub={sub}: worst Gram error / bound {worst:.3g}")


def test_huge_values_an_overflowing_diagonal_and_the_abstaining_screen():
    a, real, sampled, bad = planted_bad()
    dn = _Dnc(SMALL, _rows(a, False), _rtab([sampled]), 1, 0, 1, 1.0)      # q = 0: only bad clients go
    dn.run(_state(1, 0))
    scores, g, kw, bw = dn.record(0)
    assert bw == mask_bits(k in bad for k in range(9)) and dn.kept() == kw == mask_bits(k not in bad for k in range(9))
    assert np.isinf(g[3, 3]) and np.isfinite(g[0, 0]) and np.isinf(scores[list(bad)]).all()
    dn = _Dnc(SMALL, _rows(a[[8, 8]], False), _rtab([np.ones(2, bool)]), 1, 0, 1, 1.0)   # two NaN clients: nobody survives
    dn.run(_state(1, 0))
    assert dn.record(0)[2:] == (0, 0b11) and dn.kept() == 0b11


def test_a_state_that_is_not_live_writes_nothing():
    a, real, sampled, f, bad, nan = planted(SMALL, 17, 5)
    rtab = _rtab([sampled])
    for state in (_state(0, 0), _state(1, 1), _state(1, -1)):
        dn = _Dnc(SMALL, _rows(a, False), rtab, 1, f, 2, 0.5)
        dn.run(state)
        assert (dn.scratch.cpu().numpy() == -7.0).all() and dn.kept() == SENTINEL
        assert (dn.hist.cpu().numpy() == SENTINEL).all()


def test_captured_graph_replays_each_rounds_own_subset_and_word():
    K = 17
    a, real, sampled, f, bad, nan = planted(SMALL, K, 77)
    honest = [k for k in range(K) if k not in bad and k != nan]
    masks = [np.ones(K, bool), sampled, np.arange(K) != honest[-1]]   # (the planted clients are always sampled)
    rtab = _rtab(masks)
    rows = _rows(a, False)
    eager = []
    for r in range(3):
        dn = _Dnc(SMALL, rows, rtab, 3, f, 2, 0.5)
        dn.run(_state(1, r))
        eager.append((dn.kept(), dn.record(1)[1].copy()))
        assert dn.kept() == mask_bits(dnc_select_ref(a[:, :real.shape[0]], masks[r], real, f, 1.0, 2, 0.5, SEED, r)[0])
    assert len({k for k, _ in eager}) == 3 and not np.array_equal(eager[0][1], eager[2][1])
    dn = _Dnc(SMALL, rows, rtab, 3, f, 2, 0.5)
    state = _state(1, 0)
    torch.cuda.synchronize()
    stream, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=stream):
        dn.run(state, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for r in (0, 1, 2, 1):
        state.copy_(_state(1, r))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert dn.kept() == eager[r][0], r
        np.testing.assert_array_equal(dn.record(1)[1], eager[r][1])
    assert [int(h) for h in dn.hist.cpu().numpy().view(np.uint64)] == [k for k, _ in eager]


@pytest.mark.parametrize("agg", ["median", "mean"])
def test_hip_group_against_the_torch_group(agg):
    kw = dict(screen_iters=2, screen_subsample=0.5, screen_seed=11)
    hip, ref = _alie_group("hip", agg, **kw), _alie_group("torch", agg, **kw)
    h, ht = hip.history(), ref.history()
    np.testing.assert_array_equal(h["screen_kept"], ht["screen_kept"])
    assert all(int(w) & 0b100100 == 0 and int(w) for w in h["screen_kept"])
    assert hip.clients[0].layout["screen"] == "dnc" and hip.clients[0].layout["aggregator"] == agg
    err = nerr(hip.global_flat(), ref.global_flat())
    print(f"dnc group {agg}: HIP vs torch {err:.3g}")
    assert np.isfinite(hip.global_flat()).all() and err < 2e-5, err
