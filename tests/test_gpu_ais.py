"""Annealed importance sampling for log Z on the MI355X (plm_ais / plm.log_partition, DESIGN_NEXT_ROWS.md section 9.8):
every launch plan against the numpy twin (tests/ais_twin.py) draw for draw and, where the states agree, bit for bit in
the log weights and the tracked energy; the tracked energy against float64 energies; independence of the chain count and
of how the steps are cut into launches; exact log Z of enumerable models; a fitted model."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ais_twin as at  # noqa: E402
import sampler_plan_cases as cases  # noqa: E402
from test_gpu_sampler import _explained, _random_model  # noqa: E402
from evcouplings_amd import plm  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.abspath(__file__))
CAP = 0.01                                # of the chains may differ from the twin at all
FIELDS = ("states", "log_w", "e_j")


def _same(a, b, what):
    for k in FIELDS:
        assert np.array_equal(a[k], b[k]), (what, k, np.argwhere(a[k] != b[k])[:5])


def _ran(L, q, Cn, **want):
    p = plm.sample_plan(L, q, Cn)
    assert {k: p[k] for k in want} == want, (L, q, Cn, p)
    return p


@pytest.mark.parametrize("tile", cases.TILES)
def test_every_plan_follows_the_twin(tile):
    """k_ais<1 .. 8, tile> and k_ais_direct<2 .. 32>: L = 37, two workgroups with 37 live lanes in the second, three steps
    of a schedule that ends above 1.  The states after every step come from calls with the prefixes of the schedule."""
    L = cases.WIDTH_L
    betas = np.array([0.0, 0.4, 0.7, 1.3], np.float32)
    K = len(betas) - 1
    differ = chains = 0
    for q in cases.WIDTH_QS:
        Cn = tile + 37
        name = "tile %d q=%d" % (tile, q)
        h, J = _random_model(np.random.default_rng(7100 + q + tile), L, q)
        seed = 5151 + q
        twin = at.ais(h, J, q, Cn, betas=betas, seed=seed, trace=True)["steps"]
        with cases.forced(tile=tile):
            _ran(L, q, Cn, direct=False, tile=tile, jc=cases.WIDTH_JC[tile][q], nv=(q + 3) // 4, n_workgroups=2)
            start = plm.sample(h, J, q, Cn, burn_in=0, seed=seed, energies=False)[0][0]
            tiled = [plm.log_partition(h, J, q, n_chains=Cn, betas=betas[:k + 1], seed=seed) for k in range(1, K + 1)]
        with cases.forced(form="direct"):
            assert Cn % _ran(L, q, Cn, direct=True)["tile"] != 0           # a partial last workgroup
            direct = [plm.log_partition(h, J, q, n_chains=Cn, betas=betas[:k + 1], seed=seed) for k in range(1, K + 1)]
        for k in range(K):
            _same(tiled[k], direct[k], "%s, %d steps: tiled against direct" % (name, k + 1))
            assert tiled[k]["log_z"] == direct[k]["log_z"] and tiled[k]["steps_done"] == k + 1
            assert tiled[k]["status"] == "converged"
            assert ("entropy" in tiled[k]) == (float(betas[k + 1]) == 1.0)
        gpu = np.stack([start] + [r["states"] for r in tiled]).astype(np.int64)
        _explained(name, gpu, twin["states"], twin["margin"], twin["maxarg"], L, q, cap=1.0)
        agree = (gpu == twin["states"]).all(axis=(0, 2))
        differ += int((~agree).sum())
        chains += Cn
        for k in range(K):
            for f in ("log_w", "e_j"):
                g, t = tiled[k][f][agree], twin[f][k + 1][agree]
                assert np.array_equal(g, t), (name, k + 1, f, np.abs(g - t).max())
        # the summary is the definition's, from the returned log weights
        lz, se, ess = at.summary(tiled[-1]["log_w"], at.log_z0(h))
        assert abs(tiled[-1]["log_z0"] - at.log_z0(h)) <= 1e-13 * abs(at.log_z0(h))
        assert abs(tiled[-1]["log_z"] - lz) <= 1e-12 * abs(lz) and abs(tiled[-1]["ess"] - ess) <= 1e-9 * ess
        assert abs(tiled[-1]["log_z_se"] - se) <= 1e-9 * se
    print("tile %d: %d of %d chains differ from the twin" % (tile, differ, chains))
    assert differ <= CAP * chains, (differ, chains)


@pytest.mark.parametrize("q", sorted(cases.CHUNK_QS))
def test_chunk_geometry(q):
    """Tile 64, every chunk length the planner accepts, at lengths below, at and above it: each run equals the direct form
    bit for bit.  One site has no couplings: nothing to track."""
    Cn, K = cases.CHUNK_C, 2
    for L in cases.CHUNK_LS:
        h, J = _random_model(np.random.default_rng(8100 + 100 * q + L), L, q)
        seed = 77 + L
        with cases.forced(form="direct"):
            _ran(L, q, Cn, direct=True)
            direct = plm.log_partition(h, J, q, n_chains=Cn, n_temps=K, seed=seed)
        if L == 1:
            assert not direct["e_j"].any() and not direct["log_w"].any()
            assert direct["log_z"] == direct["log_z0"] and direct["ess"] == Cn
            assert abs(direct["log_z0"] - at.log_z0(h)) <= 1e-13 * abs(at.log_z0(h))
        else:
            assert direct["log_w"].std() > 0
        for jc in cases.CHUNK_QS[q]:
            with cases.forced(tile=64, jc=jc):
                _ran(L, q, Cn, direct=False, tile=64, jc=jc, n_workgroups=2)
                tiled = plm.log_partition(h, J, q, n_chains=Cn, n_temps=K, seed=seed)
            _same(tiled, direct, "q=%d L=%d jc=%d" % (q, L, jc))
            assert tiled["log_z"] == direct["log_z"]


@pytest.mark.parametrize("L,q,K,j_scale", [(37, 21, 16, 0.15), (49, 3, 8, 0.5)])
def test_tracked_energy_against_float64(L, q, K, j_scale):
    """e_j of every chain against the float64 coupling energy of its final state.  The tracked value is E0 (L sums of L - 1
    float32 terms, halved) plus K n L differences of two such sums; a sum of L - 1 terms carries at most (L - 2) 2^-24
    times the sum of the |terms|, so the worst case is (2 K n + 1/2)(L - 2) 2^-24 sum_i sum_{j != i} max |J_ij|."""
    Cn, n = 1024 + 37, 1
    h, J = _random_model(np.random.default_rng(300 + L), L, q, j_scale=j_scale)
    r = plm.log_partition(h, J, q, n_chains=Cn, n_temps=K, sweeps_per_temp=n, seed=L)
    ref = plm.hamiltonians(r["states"], q, h, J)[:, 1]
    bound = (2 * K * n + 0.5) * (L - 2) * 2.0 ** -24 * 2.0 * np.abs(J).max(axis=(1, 2)).sum()
    err = np.abs(r["e_j"] - ref).max()
    print("L=%d q=%d K=%d: max |e_j - H_J| = %.3g (bound %.3g), max|J| = %.3g" % (L, q, K, err, bound, np.abs(J).max()))
    assert err <= bound, (err, bound)


def test_independent_of_launches_and_chain_count_and_cancellation():
    L, q, K = 23, 21, 7
    h, J = _random_model(np.random.default_rng(41), L, q)
    kw = dict(n_temps=K, sweeps_per_temp=2, seed=17)
    whole = plm.log_partition(h, J, q, n_chains=300, steps_per_launch=K, **kw)
    for spl in (1, 3, 0):
        cut = plm.log_partition(h, J, q, n_chains=300, steps_per_launch=spl, **kw)
        _same(cut, whole, "steps_per_launch=%d" % spl)
        assert cut["log_z"] == whole["log_z"] and cut["steps_done"] == K
    small = plm.log_partition(h, J, q, n_chains=64 + 37, **kw)
    for k in FIELDS:
        assert np.array_equal(small[k], whole[k][:101]), k
    other = plm.log_partition(h, J, q, n_chains=300, n_temps=K, sweeps_per_temp=2, seed=18)
    assert (other["log_w"] != whole["log_w"]).mean() > 0.9
    # a callback is called between launches only, and cancels
    seen = []
    done = plm.log_partition(h, J, q, n_chains=300, steps_per_launch=3, callback=lambda d, t: seen.append((d, t)), **kw)
    assert seen == [(3, K), (6, K)] and done["status"] == "converged"
    _same(done, whole, "with a callback")
    stop = plm.log_partition(h, J, q, n_chains=300, steps_per_launch=3, callback=lambda d, t: True, **kw)
    assert stop["status"] == "interrupted" and stop["steps_done"] == 3
    assert np.isnan(stop["log_z"]) and "entropy" not in stop
    prefix = plm.log_partition(h, J, q, n_chains=300, betas=at.linear_schedule(K)[:4], sweeps_per_temp=2, seed=17)
    _same(stop, prefix, "the state reached at cancellation")
    with pytest.raises(ZeroDivisionError):
        plm.log_partition(h, J, q, n_chains=300, steps_per_launch=3, callback=lambda d, t: 1 // 0, **kw)


@pytest.mark.parametrize("L,q,j_scale,model_seed", at.ENUMERABLE)
def test_against_enumeration(L, q, j_scale, model_seed):
    h, J = at.enumerable_model(L, q, j_scale, model_seed)
    exact = at.exact_log_z(h, J, q)
    for seed in at.ENUMERABLE_SEEDS:
        twin = at.ais(h, J, q, at.ENUMERABLE_C, at.ENUMERABLE_K, seed=seed)
        r = plm.log_partition(h, J, q, n_chains=at.ENUMERABLE_C, n_temps=at.ENUMERABLE_K, seed=seed)
        print("L=%d q=%d seed %d: log Z %.5f (twin %.5f, exact %.5f), twin's se %.5f, ess %.0f" % (
            L, q, seed, r["log_z"], twin["log_z"], exact, twin["log_z_se"], r["ess"]))
        assert abs(r["log_z"] - exact) <= 5 * twin["log_z_se"], (seed, r["log_z"], exact, twin["log_z_se"])
        lz, se, ess = at.summary(r["log_w"], at.log_z0(h))
        assert abs(r["ess"] - ess) <= 1e-9 * ess and abs(r["log_z_se"] - se) <= 1e-9 * se
        w = np.exp(r["log_w"] - r["log_w"].max())
        assert abs(r["ess"] - w.sum() ** 2 / (w * w).sum()) <= 1e-9 * ess
        assert abs(r["log_z_se"] - w.std(ddof=1) / (np.sqrt(len(w)) * w.mean())) <= 1e-9 * se
        assert np.isfinite(r["entropy"]) and r["entropy"] < L * np.log(q)


def test_a_fitted_model():
    """tests/golden/hip_fit_L24.npz: two schedules agree within their own standard errors, and the entropy is that of a
    distribution over q^L sequences."""
    d = np.load(os.path.join(ROOT, "golden", "hip_fit_L24.npz"))
    h, J = d["hi"], d["jij"]
    L, q = h.shape
    a = plm.log_partition(h, J, q, n_chains=1024, n_temps=128, seed=1)
    b = plm.log_partition(h, J, q, n_chains=1024, n_temps=32, seed=2)
    print("hip_fit_L24: K=128 log Z %.4f +- %.4f (ess %.0f), K=32 %.4f +- %.4f (ess %.0f), log Z0 %.4f, entropy %.3f" % (
        a["log_z"], a["log_z_se"], a["ess"], b["log_z"], b["log_z_se"], b["ess"], a["log_z0"], a["entropy"]))
    assert abs(a["log_z"] - b["log_z"]) <= 4 * np.hypot(a["log_z_se"], b["log_z_se"])
    assert a["log_z"] > a["log_z0"]
    for r in (a, b):
        assert np.isfinite(r["entropy"]) and r["entropy"] < L * np.log(q)
