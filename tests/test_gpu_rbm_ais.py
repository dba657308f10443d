"""Annealed importance sampling for the restricted Boltzmann machine on the GPU (plm_rbm_ais / plm.rbm_log_partition,
DESIGN_NEXT_ROWS.md section 9.25) against the numpy twin tests/rbm_ais_twin.py.  The shapes, seeds and schedules are those
of tests/rbm_ais_cases.py, whose conditions test_rbm_ais_host.py checks on the CPU.

Observed on one MI355X: no chain of the eight draw-for-draw cases differs from the twin; |log w - twin| is at most 0.017 of
its bound ((5, 3, 3), n = 1) and 0.0032 of it against the host's value from the score's inputs; the z-scores against
exact enumeration are +0.33, +0.29, -1.30 at (5, 3, 3) and +0.50, -0.83, -0.98 at (13, 21, 7); the fitted model gives
48.13825 +- 0.00826 (K = 32) and 48.13865 +- 0.00407 (K = 128) against 48.13465; the whole file in 3 s."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import rbm_ais_cases as cases
import rbm_ais_twin as at
import rbm_cases
import rbm_twin as tw
from evcouplings_amd import alignment_io, plm, rbm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bytes(r):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in ("log_w", "states", "hidden"))


# ---- 1. draw for draw -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,q,M,Cn,n,seed", cases.FOLLOW_CASES)
def test_follows_the_twin(L, q, M, Cn, n, seed):
    """The schedule (0, 0.4, 0.7, 1.3) read step by step through its prefixes.  A chain may differ from the twin only from
    a near tie on (rbm_ais_twin.first_difference_explained), 1 % of the chains at most; log w of every chain whose draws
    agree lies within 2^-49 K M (1 + max |x|) of the twin's."""
    g, c, W = cases.model(L, q, M)
    twin = cases.follow_twin(L, q, M, Cn, n, seed)
    steps = twin["steps"]
    agrees = np.ones(Cn, bool)
    unexplained, worst = [], 0.0
    for K in range(1, len(cases.BETAS)):
        r = plm.rbm_log_partition(g, c, W, q, n_chains=Cn, sweeps_per_temp=n, betas=cases.BETAS[:K + 1], seed=seed,
                                  hidden=True)
        assert r["status"] == "converged" and r["steps_done"] == K and set(np.unique(r["hidden"])) <= {0, 1}
        differs = (r["states"] != steps["states"][K]).any(axis=1) | (r["hidden"] != steps["hidden"][K]).any(axis=1)
        for ch in np.nonzero(differs & agrees)[0]:
            step = {key: steps[key][K - 1][:, ch] for key in ("hm", "hx", "vm", "va")}
            step.update(states=steps["states"][K][ch], hidden=steps["hidden"][K][ch])
            start_tie = K == 1 and (twin["start_margin"][ch] <= tw.delta_visible(0, q, twin["start_maxu"][ch])).any()
            if not (start_tie or at.first_difference_explained(step, r["states"][ch], r["hidden"][ch], q)):
                unexplained.append((int(ch), K))
        agrees &= ~differs
        bound = at.log_w_bound(K, M, twin["max_x"])
        err = np.abs(r["log_w"] - steps["log_w"][K])[agrees]
        if err.size:
            worst = max(worst, float(err.max() / bound))
        assert (err <= bound).all(), (K, float(err.max()), bound)
    print("L=%d q=%d M=%d C=%d n=%d: %d chains differ from the twin, %d unexplained; max |log w - twin| / bound = %.3g"
          % (L, q, M, Cn, n, (~agrees).sum(), len(unexplained), worst))
    assert not unexplained, unexplained[:5]
    assert (~agrees).sum() <= 0.01 * Cn


# ---- 2. the bytes do not depend on the plan ---------------------------------------------------------------------------

@pytest.mark.parametrize("L,q,M", cases.PLAN_SHAPES)
def test_same_bytes_under_every_plan(L, q, M, monkeypatch):
    g, c, W = cases.model(L, q, M)
    K, n, Cn = cases.PLAN_K, cases.PLAN_N, cases.PLAN_C
    kw = dict(n_temps=K, sweeps_per_temp=n, seed=cases.PLAN_SEED, hidden=True)
    base = plm.rbm_log_partition(g, c, W, q, n_chains=Cn, **kw)
    assert base["status"] == "converged" and base["steps_done"] == K and np.isfinite(base["log_z"])
    # PLM_RBM_WAVES is read at every call
    for waves in ("1", "2", "4", "8"):
        monkeypatch.setenv("PLM_RBM_WAVES", waves)
        again = plm.rbm_log_partition(g, c, W, q, n_chains=Cn, **kw)
        assert _bytes(again) == _bytes(base), waves
        assert (again["log_z"], again["log_z_se"], again["ess"]) == (base["log_z"], base["log_z_se"], base["ess"])
    monkeypatch.delenv("PLM_RBM_WAVES")
    head = plm.rbm_log_partition(g, c, W, q, n_chains=cases.PLAN_C_HEAD, **kw)
    for key in ("log_w", "states", "hidden"):
        assert head[key].tobytes() == base[key][:cases.PLAN_C_HEAD].tobytes(), key
    for spl in cases.PLAN_LAUNCHES:
        assert _bytes(plm.rbm_log_partition(g, c, W, q, n_chains=Cn, steps_per_launch=spl, **kw)) == _bytes(base), spl
    seen = []
    on = plm.rbm_log_partition(g, c, W, q, n_chains=Cn, steps_per_launch=2, callback=lambda d, t: seen.append((d, t)), **kw)
    assert seen == [(2, K), (4, K), (6, K)] and _bytes(on) == _bytes(base) and on["log_z"] == base["log_z"]
    cut = plm.rbm_log_partition(g, c, W, q, n_chains=Cn, steps_per_launch=1, callback=lambda d, t: d == 3, **kw)
    assert cut["status"] == "interrupted" and cut["steps_done"] == 3
    assert np.isnan([cut["log_z"], cut["log_z_se"], cut["ess"]]).all() and cut["log_z0"] == base["log_z0"]
    assert "entropy" not in cut and "mean_score" not in cut
    prefix = plm.rbm_log_partition(g, c, W, q, n_chains=Cn, sweeps_per_temp=n, betas=at.linear_schedule(K)[:4],
                                   seed=cases.PLAN_SEED, hidden=True)
    assert _bytes(cut) == _bytes(prefix)

    def fails(done, total):
        raise KeyError("from the callback")

    with pytest.raises(KeyError, match="from the callback"):
        plm.rbm_log_partition(g, c, W, q, n_chains=Cn, steps_per_launch=1, callback=fails, **kw)


# ---- 3. the inputs are those of the score -----------------------------------------------------------------------------

@pytest.mark.parametrize("L,q,M", cases.PLAN_SHAPES)
def test_inputs_are_the_scores_inputs(L, q, M):
    """W = 0 on all but one unit: log w from the host, out of the inputs plm.rbm_score returns for the states each step
    began with (the start states, then those of the one-step prefix)."""
    g, c, W = cases.model(L, q, M)
    W = W.copy()
    W[np.arange(M) != M - 2] = 0.0
    Cn, seed = 300, 31
    v0 = plm.rbm_sample(g, c, W, q, Cn, burn_in=0, seed=seed)[0]
    one = plm.rbm_log_partition(g, c, W, q, n_chains=Cn, betas=cases.BETAS[:2], seed=seed)
    two = plm.rbm_log_partition(g, c, W, q, n_chains=Cn, betas=cases.BETAS[:3], seed=seed)
    I0 = plm.rbm_score(v0, q, g, c, W, inputs=True)[1]
    I1 = plm.rbm_score(one["states"], q, g, c, W, inputs=True)[1]
    lw1 = at.weight_step(I0, cases.BETAS[1], cases.BETAS[0])
    lw2 = lw1 + at.weight_step(I1, cases.BETAS[2], cases.BETAS[1])
    max_x = float(cases.BETAS[2]) * max(np.abs(I0).max(), np.abs(I1).max())
    e1, e2 = np.abs(one["log_w"] - lw1).max(), np.abs(two["log_w"] - lw2).max()
    print("L=%d q=%d M=%d: |log w - host| / bound = %.3g (one step), %.3g (two)"
          % (L, q, M, e1 / at.log_w_bound(1, M, max_x), e2 / at.log_w_bound(2, M, max_x)))
    assert e1 <= at.log_w_bound(1, M, max_x) and e2 <= at.log_w_bound(2, M, max_x)
    assert np.ptp(lw2) > 0.0


# ---- 4. exact values --------------------------------------------------------------------------------------------------

def _ns(g, c, W):
    return SimpleNamespace(g=g, c=c, W=W, L=g.shape[0], q=g.shape[1], M=c.size)


@pytest.mark.parametrize("L,q,M,sd_w", cases.ENUMERABLE)
def test_against_enumeration(L, q, M, sd_w):
    g, c, W = cases.enumerable_model(L, q, M, sd_w)
    exact = rbm.log_partition_exact(_ns(g, c, W))
    for seed in cases.ENUMERABLE_SEEDS:
        twin = cases.enumerable_twin(L, q, M, sd_w, seed)
        r = plm.rbm_log_partition(g, c, W, q, n_chains=cases.ENUMERABLE_C, n_temps=cases.ENUMERABLE_K, seed=seed)
        print("L=%d q=%d M=%d seed %d: log Z %.5f (twin %.5f), exact %.5f, se %.5f, z %+.2f, ess %.0f"
              % (L, q, M, seed, r["log_z"], twin["log_z"], exact, r["log_z_se"], (r["log_z"] - exact) / r["log_z_se"], r["ess"]))
        assert abs(r["log_z"] - exact) <= 5 * twin["log_z_se"]
        lz, se, ess = at.summary(r["log_w"], r["log_z0"])
        assert abs(r["log_z"] - lz) <= 1e-9 and abs(r["log_z_se"] - se) <= 1e-9 and abs(r["ess"] - ess) <= 1e-9
        assert abs(r["log_z0"] - at.log_z0(g, M)) <= 1e-12              # L + 1 float64 terms of order one to ten
        assert np.isfinite(r["entropy"]) and r["entropy"] == r["log_z"] - r["mean_score"]


def _sp(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def test_closed_forms():
    # W = 0: every chain carries the same log w, the closed form up to the rounding of K M terms
    L, q, M, Cn = 6, 5, 11, 300
    g, c, _ = tw.random_model(L, q, M, seed=3)
    W = np.zeros((M, L, q), np.float32)
    for betas, last, K in ((None, 1.0, 4), (np.array([0.0, 0.3, 0.3, 2.5], np.float32), 2.5, 3)):
        r = plm.rbm_log_partition(g, c, W, q, n_chains=Cn, n_temps=4, sweeps_per_temp=2, betas=betas, seed=1)
        want = float((_sp(np.float64(np.float32(last)) * c.astype(np.float64)) - np.log(2.0)).sum())
        max_x = last * float(np.abs(c).max())
        assert (r["log_w"] == r["log_w"][0]).all()
        assert abs(r["log_w"][0] - want) <= at.log_w_bound(K, M, max_x)
        assert r["ess"] == Cn and r["log_z_se"] == 0.0
        assert abs(r["log_z"] - (at.log_z0(g, M) + want)) < 1e-12
    # K = 1 is plain importance sampling from the start states
    L, q, M, sd_w = cases.ENUMERABLE[0]
    g, c, W = cases.enumerable_model(L, q, M, sd_w)
    for b1 in (1.0, 0.25):
        r = plm.rbm_log_partition(g, c, W, q, n_chains=2000, betas=[0.0, b1], seed=9)
        x0 = plm.rbm_sample(g, c, W, q, 2000, burn_in=0, seed=9)[0]
        I = tw.inputs(x0, c, W)
        lw = _sp(np.float64(np.float32(b1)) * I).sum(axis=1) - M * np.log(2.0)
        assert np.abs(r["log_w"] - lw).max() <= at.log_w_bound(1, M, b1 * float(np.abs(I).max()))
        assert abs(r["log_z"] - (at.log_z0(g, M) + np.log(np.mean(np.exp(lw))))) < 1e-12
    # one site, two states, one unit: by hand
    g = np.array([[0.3, -0.2]], np.float32)
    c = np.array([0.4], np.float32)
    W = np.array([[[1.5, -0.7]]], np.float32)
    g64, c64, W64 = g.astype(np.float64), c.astype(np.float64), W.astype(np.float64)
    exact = np.log(sum(np.exp(g64[0, a]) * (1.0 + np.exp(c64[0] + W64[0, 0, a])) for a in (0, 1)))
    r = plm.rbm_log_partition(g, c, W, 2, n_chains=4096, betas=[0.0, 1.0], seed=4)
    start = plm.rbm_sample(g, c, W, 2, 4096, burn_in=0, seed=4)[0][:, 0]
    by_hand = np.log1p(np.exp(c64[0] + W64[0, 0, start])) - np.log(2.0)
    assert np.abs(r["log_w"] - by_hand).max() <= at.log_w_bound(1, 1, 1.9)
    assert abs(r["log_z"] - exact) <= 4 * r["log_z_se"]
    r = plm.rbm_log_partition(g, c, W, 2, n_chains=4096, n_temps=16, seed=4)
    assert abs(r["log_z"] - exact) <= 4 * r["log_z_se"]
    # large biases stay finite
    g, _, W = tw.random_model(5, 3, 4, seed=8)
    c = np.array([50.0, -50.0, 50.0, -50.0], np.float32)
    r = plm.rbm_log_partition(g, c, W, 3, n_chains=64, n_temps=8, seed=2)
    assert np.isfinite(r["log_w"]).all() and np.isfinite([r["log_z"], r["log_z_se"], r["ess"]]).all()
    assert abs(r["log_z"] - rbm.log_partition_exact(_ns(g, c, W))) <= 4 * r["log_z_se"] + 1e-9


# ---- 5. a fitted model ------------------------------------------------------------------------------------------------

def _fitted():
    L, q, M = cases.FIT["shape"]
    msa, w, (g, c, W) = rbm_cases.fit_data(L, q, M, cases.FIT["N"], cases.FIT["seed"])
    r = plm.rbm_fit(msa, w, q, g, c, W, cases.FIT["chains"], cases.FIT["epochs"], lr=cases.FIT["lr"], seed=cases.FIT["seed"])
    m = _ns(r["g"], r["c"], r["W"])
    m.alphabet = alignment_io.ALPHABET_PROTEIN[:q]
    return m, msa, w


def test_a_fitted_model():
    m, msa, w = _fitted()
    exact = rbm.log_partition_exact(m)
    k1, k2 = cases.FIT["K"]
    a = rbm.log_partition(m, n_chains=cases.FIT["C"], n_temps=k1, seed=1)
    b = rbm.log_partition(m, n_chains=cases.FIT["C"], n_temps=k2, seed=1)
    for K, r in ((k1, a), (k2, b)):
        print("K = %d: log Z %.5f +- %.5f (exact %.5f, z %+.2f), ess %.0f, entropy %.4f"
              % (K, r["log_z"], r["log_z_se"], exact, (r["log_z"] - exact) / r["log_z_se"], r["ess"], r["entropy"]))
        assert abs(r["log_z"] - exact) <= 5 * r["log_z_se"]
        assert np.isfinite(r["entropy"]) and r["entropy"] < m.L * np.log(m.q)
    assert abs(a["log_z"] - b["log_z"]) <= 4 * np.sqrt(a["log_z_se"] ** 2 + b["log_z_se"] ** 2)
    assert b["log_z_se"] < a["log_z_se"]
    sc = rbm.scores(m, msa)
    w64 = w.astype(np.float64)
    ll = rbm.mean_log_likelihood(m, msa, w, n_chains=cases.FIT["C"], n_temps=k2, seed=1)
    assert abs(ll - ((w64 * sc).sum() / w64.sum() - b["log_z"])) < 1e-9
    twin_ll = (w64 * (tw.score(msa, m.g, m.c, m.W) - exact)).sum() / w64.sum()
    assert abs(rbm.mean_log_likelihood(m, msa, w, log_z=exact) - twin_ll) < 1e-9


# ---- 6. the Python layer and the command line -------------------------------------------------------------------------

def test_python_layer_and_cli(tmp_path):
    L, q, M = 13, 21, 7
    g, c, W = cases.model(L, q, M)
    alphabet = alignment_io.ALPHABET_PROTEIN[:q]
    m = SimpleNamespace(g=g, c=c, W=W, alphabet=alphabet, L=L, q=q, M=M, index_list=np.arange(1, L + 1, dtype=np.int32),
                        target_seq=alphabet[1] * L, lambda_g=0.0, lambda_w=1e-3, n_eff=1.0, theta=0.8)
    rows = np.random.default_rng(6).integers(1, q, (20, L)).astype(np.int8)
    res = plm.rbm_log_partition(g, c, W, q, n_chains=512, n_temps=64, seed=7)
    lp, d = rbm.log_probabilities(m, rows, n_chains=512, n_temps=64, seed=7)
    assert d["log_z"] == res["log_z"] and np.array_equal(lp, rbm.scores(m, rows) - res["log_z"])
    assert np.array_equal(rbm.log_probabilities(m, rows, 1.25)[0], rbm.scores(m, rows) - 1.25)
    assert abs(res["log_z"] - rbm.log_partition_exact(m)) <= 5 * res["log_z_se"]
    model, a2m, csv = str(tmp_path / "m.npz"), str(tmp_path / "s.a2m"), str(tmp_path / "s.csv")
    rbm.save(model, m)
    with open(a2m, "w") as f:
        for s, row in enumerate(rows):
            f.write(">seq%d\n%s\n" % (s, "".join(alphabet[k] for k in row)))
    run = lambda *a: subprocess.run([sys.executable, "-m", "evcouplings_amd.rbm"] + [str(v) for v in a], cwd=ROOT,
                                    capture_output=True, text=True, timeout=300)
    r = run("logz", model, "-n", 512, "-k", 64, "--seed", 7)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "log Z = %.6f +- %.6f (ESS = %.1f of 512 chains" % (res["log_z"], res["log_z_se"], res["ess"]) in r.stdout
    assert "log Z_0 = %.6f, entropy = %.6f" % (res["log_z0"], res["entropy"]) in r.stdout
    r = run("score", model, "--sequences", a2m, "-o", csv, "--log-z", "ais")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = open(csv).read().split()
    assert lines[0] == "id,score,log_prob" and len(lines) == 21
    got = np.array([[float(v) for v in line.split(",")[1:]] for line in lines[1:]])
    sc = rbm.scores(m, rows)
    assert np.array_equal(got[:, 0], sc) and np.array_equal(got[:, 1], sc - rbm.log_partition(m)["log_z"])
