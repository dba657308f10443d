"""Annealed importance sampling for the restricted Boltzmann machine (plm_rbm_ais, DESIGN_NEXT_ROWS.md section 9.25) without
a GPU: the numpy twin (tests/rbm_ais_twin.py) against rbm.log_partition_exact and in its closed-form cases, the conditions
the device tests rest on (rbm_ais_cases.py), the binding and the validation that comes before the device check, and the
wrappers and the command line with plm.rbm_log_partition replaced by the twin.

The Philox twin's z-scores (log_z - exact) / log_z_se at K = 16, C = 4096, seeds 0, 1, 2: +0.33, +0.29, -1.30 at
(5, 3, 3) with se 0.0056-0.0058 and ess 3605-3623; +0.50, -0.83, -0.99 at (13, 21, 7) with se 0.0196-0.0207 and ess
1483-1595."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import rbm_ais_cases as cases
import rbm_ais_twin as at
import rbm_twin as tw
import sampler_twin as st
from evcouplings_amd import _lib, plm, rbm

EINVAL, EUNSUPPORTED = -1, -4


def _ns(g, c, W):
    return SimpleNamespace(g=g, c=c, W=W, L=g.shape[0], q=g.shape[1], M=c.size)


# ---- the twin against exact values ------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,q,M,sd_w", cases.ENUMERABLE)
def test_twin_against_enumeration(L, q, M, sd_w):
    """Linear schedule, K = 16, n = 1, C = 4096: within four of its own standard errors of the exact log Z, three seeds."""
    g, c, W = cases.enumerable_model(L, q, M, sd_w)
    exact = rbm.log_partition_exact(_ns(g, c, W))
    for seed in cases.ENUMERABLE_SEEDS:
        r = cases.enumerable_twin(L, q, M, sd_w, seed)
        z = (r["log_z"] - exact) / r["log_z_se"]
        print("L=%d q=%d M=%d seed %d: log Z %.5f, exact %.5f, se %.5f, z %+.2f, ess %.0f"
              % (L, q, M, seed, r["log_z"], exact, r["log_z_se"], z, r["ess"]))
        assert abs(r["log_z"] - exact) <= 4 * r["log_z_se"], (seed, r["log_z"], exact, r["log_z_se"])
        assert 0 < r["log_z_se"] < 0.05 and 0.25 * cases.ENUMERABLE_C < r["ess"] <= cases.ENUMERABLE_C


def _sp(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def test_without_weights_the_estimate_is_exact():
    """W = 0: every chain has log w = sum_mu sp(beta_K c_mu) - log 2 up to the rounding of K M terms, ess = C, and log Z
    is the closed form; also with a schedule that ends elsewhere than at 1."""
    L, q, M, Cn = 6, 5, 11, 300
    g, c, _ = tw.random_model(L, q, M, seed=3)
    W = np.zeros((M, L, q), np.float32)
    for betas, last in ((None, 1.0), (np.array([0.0, 0.3, 0.3, 2.5], np.float32), 2.5)):
        r = at.ais(g, c, W, Cn, 4, sweeps_per_temp=2, betas=betas, seed=1)
        K = 4 if betas is None else 3
        want = float((_sp(np.float64(np.float32(last)) * c.astype(np.float64)) - np.log(2.0)).sum())
        assert (r["log_w"] == r["log_w"][0]).all()
        assert abs(r["log_w"][0] - want) <= at.log_w_bound(K, M, r["max_x"])
        assert r["ess"] == Cn and r["log_z_se"] == 0.0
        assert abs(r["log_z"] - (at.log_z0(g, M) + want)) < 1e-12
        scaled = _ns(g, (np.float32(last) * c).astype(np.float32), W)
        assert abs(r["log_z"] - rbm.log_partition_exact(scaled)) < 1e-5      # (float32)(beta c) is not beta c


def test_one_step_is_plain_importance_sampling():
    """K = 1: v ~ the independent-site model of g, log w = sum_mu sp(beta_1 I_mu(v)) - M log 2"""
    L, q, M, sd_w = cases.ENUMERABLE[0]
    g, c, W = cases.enumerable_model(L, q, M, sd_w)
    Cn = 2000
    for b1 in (1.0, 0.25):
        r = at.ais(g, c, W, Cn, betas=[0.0, b1], seed=9)
        x0 = tw.start_states(g, Cn, 9)
        lw = _sp(np.float64(np.float32(b1)) * tw.inputs(x0, c, W)).sum(axis=1) - M * np.log(2.0)
        assert np.abs(r["log_w"] - lw).max() < 1e-12
        plain = at.log_z0(g, M) + np.log(np.mean(np.exp(lw)))
        assert abs(r["log_z"] - plain) < 1e-12
        scaled = _ns(g, (np.float32(b1) * c).astype(np.float32), (np.float32(b1) * W).astype(np.float32))
        assert abs(r["log_z"] - rbm.log_partition_exact(scaled)) <= 4 * r["log_z_se"] + 1e-5


def test_one_site_two_states_one_unit_by_hand():
    g = np.array([[0.3, -0.2]], np.float32)
    c = np.array([0.4], np.float32)
    W = np.array([[[1.5, -0.7]]], np.float32)
    g64, c64, W64 = g.astype(np.float64), c.astype(np.float64), W.astype(np.float64)
    exact = np.log(sum(np.exp(g64[0, a]) * (1.0 + np.exp(c64[0] + W64[0, 0, a])) for a in (0, 1)))
    assert abs(rbm.log_partition_exact(_ns(g, c, W)) - exact) < 1e-14
    r = at.ais(g, c, W, 4096, betas=[0.0, 1.0], seed=4, trace=True)
    start = r["steps"]["states"][0][:, 0]
    by_hand = np.log1p(np.exp(c64[0] + W64[0, 0, start])) - np.log(2.0)
    assert np.abs(r["log_w"] - by_hand).max() < 4e-15
    assert abs(r["log_z"] - exact) <= 4 * r["log_z_se"]
    r = at.ais(g, c, W, 4096, 16, seed=4)
    assert abs(r["log_z"] - exact) <= 4 * r["log_z_se"]


def test_large_biases_stay_finite():
    L, q, M = 5, 3, 4
    g, _, W = tw.random_model(L, q, M, seed=8)
    c = np.array([50.0, -50.0, 50.0, -50.0], np.float32)
    r = at.ais(g, c, W, 64, 8, seed=2)
    assert np.isfinite(r["log_w"]).all() and np.isfinite([r["log_z"], r["log_z_se"], r["ess"]]).all()
    assert abs(r["log_z"] - rbm.log_partition_exact(_ns(g, c, W))) <= 4 * r["log_z_se"] + 1e-9


def test_twin_does_not_depend_on_the_chain_count_and_prefixes_are_schedules():
    g, c, W = cases.model(5, 3, 3)
    full = at.ais(g, c, W, 64, betas=cases.BETAS, seed=2, trace=True)
    part = at.ais(g, c, W, 16, betas=cases.BETAS[:3], seed=2)
    assert np.array_equal(part["log_w"], full["steps"]["log_w"][2][:16])
    assert np.array_equal(part["states"], full["steps"]["states"][2][:16])
    assert np.array_equal(part["hidden"], full["steps"]["hidden"][2][:16])


# ---- the conditions of the device tests -------------------------------------------------------------------------------

@pytest.mark.parametrize("L,q,M,Cn,n,seed", cases.FOLLOW_CASES)
def test_follow_cases_have_few_near_ties(L, q, M, Cn, n, seed):
    """The float32-arg twin and a float64-arg twin differ in at most 0.5 % of the chains: the 1 % cap of the device test
    is then a condition the device can meet."""
    a = cases.follow_twin(L, q, M, Cn, n, seed)["steps"]
    b = cases.follow_twin(L, q, M, Cn, n, seed, True)["steps"]
    differ = ((a["states"] != b["states"]).any(axis=(0, 2)) | (a["hidden"] != b["hidden"]).any(axis=(0, 2)))
    print("L=%d q=%d M=%d C=%d n=%d: %d chains differ" % (L, q, M, Cn, n, differ.sum()))
    assert differ.sum() <= 0.005 * Cn
    same = ~differ
    K = len(cases.BETAS) - 1
    bound = at.log_w_bound(K, M, cases.follow_twin(L, q, M, Cn, n, seed)["max_x"])
    assert np.abs(a["log_w"][:, same] - b["log_w"][:, same]).max() <= bound


# ---- binding and validation -------------------------------------------------------------------------------------------

def test_binding_is_declared_and_matches_the_header_layout():
    assert "plm_rbm_ais" in {name for name, _, _ in _lib.SYMBOLS}
    assert hasattr(_lib.load(), "plm_rbm_ais")
    r = _lib.PlmRbmAisResult
    assert (r.log_z.offset, r.log_z0.offset, r.log_z_se.offset, r.ess.offset, r.log_w.offset, r.states.offset,
            r.hidden.offset, r.steps_done.offset, r.status.offset, C.sizeof(r)) == (0, 8, 16, 24, 32, 40, 48, 56, 60, 64)
    assert _lib.load().plm_version() == 2


def _code(L=4, q=3, M=2, **kw):
    g, c, W = np.zeros((L, q), np.float32), np.zeros(M, np.float32), np.zeros((M, L, q), np.float32)
    with pytest.raises(_lib.PlmError) as err:
        plm.rbm_log_partition(g, c, W, q, **kw)
    return err.value.code


def test_validation_comes_before_the_device():
    """Every PLM_EINVAL / PLM_EUNSUPPORTED, on a machine with or without a GPU."""
    assert _code(n_chains=0) == EINVAL
    assert _code(n_temps=0) == EINVAL
    assert _code(sweeps_per_temp=0) == EINVAL
    assert _code(steps_per_launch=-1) == EINVAL
    assert _code(n_temps=65536, sweeps_per_temp=65536) == EINVAL            # K n = 2^32
    assert _code(n_temps=65537, sweeps_per_temp=65535) == EINVAL            # K n = 2^32 - 1
    assert _code(betas=[0.0, 0.5, 0.4]) == EINVAL                           # decreases
    assert _code(betas=[0.1, 0.5, 1.0]) == EINVAL                           # starts above 0
    assert _code(betas=[0.0, float("nan"), 1.0]) == EINVAL
    assert _code(betas=[float("nan"), 0.5, 1.0]) == EINVAL
    assert _code(betas=[0.0, 0.5, float("inf")]) == EINVAL
    assert _code(betas=[-0.5, 0.0, 1.0]) == EINVAL
    assert _code(q=33) == EUNSUPPORTED
    assert _code(q=1) == EUNSUPPORTED
    # the tile with the chunk sums of the weight: 64 M bytes of them per 8 M of hidden bits
    assert _code(L=1, q=2, M=4096, n_chains=8, n_temps=2) == EUNSUPPORTED
    # 639 words of states and hidden bits fit the LDS (plm_rbm_sample takes the shape), the 512 bytes behind them do not
    assert 639 * 256 <= 163840 < 639 * 256 + 512
    assert _code(L=2552, q=2, M=1, n_chains=8, n_temps=2) == EUNSUPPORTED
    lib = _lib.load()
    x = np.zeros(plm.rbm_n_params(4, 3, 2), np.float32)
    xp = x.ctypes.data_as(C.c_void_p)
    opts, res = _lib.PlmAisOpts(8, 2, 1, 0, None, 0), _lib.PlmRbmAisResult()
    assert lib.plm_rbm_ais(4, 3, 2, xp, None, 0, None, _lib.AIS_CB(), None, C.byref(res)) == EINVAL
    assert lib.plm_rbm_ais(4, 3, 2, xp, C.byref(opts), 0, None, _lib.AIS_CB(), None, None) == EINVAL
    assert lib.plm_rbm_ais(4, 3, 2, None, C.byref(opts), 0, None, _lib.AIS_CB(), None, C.byref(res)) == EINVAL
    assert lib.plm_rbm_ais(0, 3, 2, xp, C.byref(opts), 0, None, _lib.AIS_CB(), None, C.byref(res)) == EINVAL
    assert lib.plm_rbm_ais(4, 3, 0, xp, C.byref(opts), 0, None, _lib.AIS_CB(), None, C.byref(res)) == EINVAL
    assert lib.plm_rbm_ais(4, 3, 1 << 28, xp, C.byref(opts), 0, None, _lib.AIS_CB(), None, C.byref(res)) == EINVAL
    big = _lib.PlmAisOpts(1 << 29, 2, 1, 0, None, 0)
    assert lib.plm_rbm_ais(4, 3, 2, xp, C.byref(big), 0, None, _lib.AIS_CB(), None, C.byref(res)) == EINVAL     # C L = 2^31
    assert lib.plm_rbm_ais(1, 3, 4, xp, C.byref(big), 0, None, _lib.AIS_CB(), None, C.byref(res)) == EINVAL     # C M = 2^31
    assert lib.plm_rbm_ais(1, 2, 64 * 65535 + 1, xp, C.byref(opts), 0, None, _lib.AIS_CB(), None,
                           C.byref(res)) == EUNSUPPORTED
    g, c, W = cases.model(4, 3, 2)
    with pytest.raises(ValueError):
        plm.rbm_log_partition(g, c, W[:, :3], 3)
    with pytest.raises(ValueError):
        plm.rbm_log_partition(g, c, W, 3, betas=[0.0])


def test_a_valid_call_fails_loudly_without_a_gpu():
    if _lib.load().plm_device_count() <= 0:                # no CPU path
        g, c, W = cases.model(4, 3, 2)
        with pytest.raises(_lib.PlmError) as err:
            plm.rbm_log_partition(g, c, W, 3, n_chains=8, n_temps=2)
        assert err.value.code == -3


# ---- the wrappers and the command line, on the twin -------------------------------------------------------------------

def _twin_score(seqs, q, g, c, W, inputs=False, device=0):
    s = tw.score(np.asarray(seqs, np.int64), g, c, W)
    return (s, tw.inputs(np.asarray(seqs, np.int64), c, W)) if inputs else s


def _file_model():
    L, q, M = 5, 3, 3
    g, c, W = cases.model(L, q, M)
    return SimpleNamespace(g=g, c=c, W=W, alphabet="-AC", L=L, q=q, M=M, index_list=np.arange(1, L + 1, dtype=np.int32),
                           target_seq="AC-CA", lambda_g=0.0, lambda_w=1e-3, n_eff=10.0, theta=0.8)


def test_wrappers_on_the_twin(monkeypatch):
    calls = []

    def fake(g, c, W, q, **kw):
        calls.append(kw)
        return at.log_partition(g, c, W, q, **kw)

    monkeypatch.setattr(plm, "rbm_log_partition", fake)
    monkeypatch.setattr(plm, "rbm_score", _twin_score)
    m = _file_model()
    exact = rbm.log_partition_exact(m)
    res = rbm.log_partition(m, n_chains=512, n_temps=8, seed=3)
    assert calls == [dict(n_chains=512, n_temps=8, seed=3)]
    assert abs(res["log_z"] - exact) <= 4 * res["log_z_se"]
    assert "hidden" not in res and np.isfinite(res["entropy"]) and res["entropy"] < m.L * np.log(m.q)
    assert res["entropy"] == res["log_z"] - res["mean_score"]
    assert rbm.log_partition(m, n_chains=8, n_temps=2, hidden=True)["hidden"].shape == (8, m.M)
    assert "entropy" not in rbm.log_partition(m, n_chains=8, betas=[0.0, 0.5])
    # log P over all states sums to one with the exact log Z
    vs = st.all_states(m.L, m.q)
    lp, d = rbm.log_probabilities(m, vs, exact)
    assert d == dict(log_z=exact) and abs(np.exp(lp).sum() - 1.0) < 1e-12
    lp2, d2 = rbm.log_probabilities(m, vs, n_chains=512, n_temps=8, seed=3)
    assert d2["log_z"] == res["log_z"] and np.array_equal(lp2, tw.score(vs, m.g, m.c, m.W) - res["log_z"])
    w = np.linspace(0.0, 1.0, len(vs))
    assert abs(rbm.mean_log_likelihood(m, vs, w, exact) - tw.mean_log_likelihood(vs, w, m.g, m.c, m.W)) < 1e-12
    assert abs(rbm.mean_log_likelihood(m, vs, log_z=exact) - lp.mean()) < 1e-12
    assert rbm.mean_log_likelihood(m, vs[:9], n_chains=512, n_temps=8, seed=3) == pytest.approx(lp2[:9].mean(), abs=1e-12)


def test_command_line_on_the_twin(monkeypatch, tmp_path, capsys):
    calls = []

    def fake(g, c, W, q, **kw):
        calls.append(kw)
        return at.log_partition(g, c, W, q, **dict(kw, n_chains=min(kw.get("n_chains", 4096), 64),
                                                   n_temps=min(kw.get("n_temps", 1000), 4)))

    monkeypatch.setattr(plm, "rbm_log_partition", fake)
    monkeypatch.setattr(plm, "rbm_score", _twin_score)
    m = _file_model()
    path = rbm.save(str(tmp_path / "m.npz"), m)
    assert rbm.main(["logz", path, "-n", "64", "-k", "4", "--sweeps", "2", "--seed", "5"]) == 0
    assert calls == [dict(n_chains=64, n_temps=4, sweeps_per_temp=2, seed=5)]
    ref = at.log_partition(m.g, m.c, m.W, m.q, n_chains=64, n_temps=4, sweeps_per_temp=2, seed=5)
    text = capsys.readouterr().out
    assert "log Z = %.6f +- %.6f (ESS = %.1f of 64 chains" % (ref["log_z"], ref["log_z_se"], ref["ess"]) in text
    assert "log Z_0 = %.6f, entropy = %.6f" % (ref["log_z0"], ref["entropy"]) in text
    a2m, out = str(tmp_path / "s.a2m"), str(tmp_path / "s.csv")
    seqs = ["AC-CA", "CCCCC", "--A-A"]
    with open(a2m, "w") as f:
        for k, s in enumerate(seqs):
            f.write(">s%d some words\n%s\n" % (k, s))
    x = np.array([["-AC".index(ch) for ch in s] for s in seqs])
    sc = tw.score(x, m.g, m.c, m.W)
    # without the option the file is what it was
    assert rbm.main(["score", path, "--sequences", a2m, "-o", out]) == 0
    plain = open(out).read().split()
    assert plain == ["id,score"] + ["s%d,%.17g" % (k, v) for k, v in enumerate(sc)]
    assert rbm.main(["score", path, "--sequences", a2m, "-o", out, "--log-z", "1.5"]) == 0
    assert open(out).read().split() == ["id,score,log_prob"] + ["s%d,%.17g,%.17g" % (k, v, v - 1.5) for k, v in enumerate(sc)]
    calls.clear()
    assert rbm.main(["score", path, "--sequences", a2m, "-o", out, "--log-z", "ais"]) == 0
    assert calls == [{}]
    lz = at.log_partition(m.g, m.c, m.W, m.q, n_chains=64, n_temps=4)["log_z"]
    rows = open(out).read().split()
    assert rows[0] == "id,score,log_prob" and [r.split(",")[1] for r in rows[1:]] == [r.split(",")[1] for r in plain[1:]]
    assert np.array_equal(np.array([float(r.split(",")[2]) for r in rows[1:]]), sc - lz)
