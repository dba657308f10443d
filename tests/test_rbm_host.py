"""The restricted Boltzmann machine without a device (DESIGN_NEXT_ROWS.md section 9.22): the float64 twin against brute
force (score, invariance of P(v) under its transition matrix, log Z), the Python layer (start point, exact log Z, model
file), the argument checks of the three entry points, which come before the device is looked at, and the conditions the
device tests of test_gpu_rbm.py rest on: for every case of rbm_cases.py the float32-mode twin follows the float64 twin in
all but 0.5 % of the chains, the fits compared byte for byte have no near tie, the twin's own histogram passes the
chi-square test, and the twin learns the planted model."""
from types import SimpleNamespace

import numpy as np
import pytest
from scipy import stats

import rbm_cases as cases
import rbm_twin as tw
import sampler_twin as st
from evcouplings_amd import _lib, plm, rbm

EINVAL, EUNSUPPORTED = -1, -4


# ---- the twin against brute force -------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,q,M", [(5, 3, 3), (3, 4, 5), (1, 2, 1)])
def test_twin_score_is_the_log_of_the_sum_over_hidden_states(L, q, M):
    g, c, W = cases.model(L, q, M)
    E = tw.joint_log_weights(g, c, W)                       # [V][H]
    brute = np.log(np.exp(E - E.max()).sum(axis=1)) + E.max()
    s, A = tw.score(st.all_states(L, q), g, c, W, with_scale=True)
    assert np.abs(s - brute).max() <= 1e-13 * max(1.0, np.abs(brute).max())
    assert (A >= np.abs(s) - 1e-12).all()


def test_twin_transition_matrix_leaves_p_invariant():
    g, c, W = cases.model(5, 3, 3)
    T = tw.transition_matrix(g, c, W)
    np.testing.assert_allclose(T.sum(axis=1), 1.0, rtol=0, atol=1e-13)
    p = tw.enumerate_p(g, c, W)
    assert abs(p.sum() - 1.0) < 1e-13
    assert np.abs(p @ T - p).max() < 1e-15


@pytest.mark.parametrize("L,q,M", [(5, 3, 3), (3, 4, 5), (1, 2, 1)])
def test_log_partition_exact_against_the_full_enumeration(L, q, M):
    g, c, W = cases.model(L, q, M)
    m = SimpleNamespace(g=g, c=c, W=W)
    assert abs(rbm.log_partition_exact(m) - tw.log_z(g, c, W)) < 1e-12
    # sum_v exp(score(v)) = Z as well
    s = tw.score(st.all_states(L, q), g, c, W)
    assert abs(np.log(np.exp(s - s.max()).sum()) + s.max() - tw.log_z(g, c, W)) < 1e-12


def test_log_partition_exact_refuses_large_models():
    with pytest.raises(ValueError, match="24"):
        rbm.log_partition_exact(SimpleNamespace(g=np.zeros((2, 3)), c=np.zeros(25), W=np.zeros((25, 2, 3))))


def test_twin_sample_cut_by_first_step_and_first_chain():
    L, q, M = 5, 3, 3
    g, c, W = cases.model(L, q, M)
    whole = tw.sample(g, c, W, q, 7, burn_in=2, n_snapshots=3, thin=2, seed=5)
    a = tw.sample(g, c, W, q, 7, burn_in=2, n_snapshots=2, thin=2, seed=5)
    b = tw.sample(g, c, W, q, 7, burn_in=2, n_snapshots=1, seed=5, start=a[-1], first_step=4)
    assert np.array_equal(whole[:2], a) and np.array_equal(whole[2], b[0])
    tail = tw.sample(g, c, W, q, 4, burn_in=2, n_snapshots=3, thin=2, seed=5, first_chain=3)
    assert np.array_equal(whole[:, 3:], tail)


# ---- the Python layer -------------------------------------------------------------------------------------------------

def test_start_point_is_the_independent_site_model():
    rng = np.random.default_rng(3)
    msa = rng.integers(0, 4, (40, 6))
    w = rng.uniform(0.2, 1.0, 40)
    g, c, W = rbm.start_point(msa, w, 4, 5, init_seed=9)
    assert g.dtype == c.dtype == W.dtype == np.float32 and W.shape == (5, 6, 4) and not c.any()
    np.testing.assert_allclose(g.sum(axis=1), 0.0, atol=1e-5)
    f = np.stack([(w[:, None] * (msa == a)).sum(axis=0) for a in range(4)], axis=1)
    f = (f + rbm.PSEUDO_COUNT / 4) / (w.sum() + rbm.PSEUDO_COUNT)
    p = np.exp(g.astype(np.float64))
    np.testing.assert_allclose(p / p.sum(axis=1, keepdims=True), f, rtol=1e-5)
    assert 0.005 < W.std() < 0.02
    assert np.array_equal(W, rbm.start_point(msa, w, 4, 5, init_seed=9)[2])
    assert not np.array_equal(W, rbm.start_point(msa, w, 4, 5, init_seed=10)[2])
    ref = np.random.Generator(np.random.PCG64(9)).normal(0.0, 0.01, (5, 6, 4)).astype(np.float32)
    assert np.array_equal(W, ref)


def _model(L=6, q=4, M=3):
    g, c, W = cases.model(L, q, M)
    return SimpleNamespace(g=g, c=c, W=W, alphabet="-ACD", L=L, q=q, M=M, index_list=np.arange(10, 10 + L, dtype=np.int32),
                           target_seq="ACD-AC", lambda_g=1e-4, lambda_w=1e-2, n_eff=12.5, theta=0.8)


def test_save_load_round_trip_and_refusal(tmp_path):
    m = _model()
    path = rbm.save(str(tmp_path / "m.npz"), m)
    r = rbm.load(path)
    for k in rbm.FIELDS:
        a, b = getattr(m, k), getattr(r, k)
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, k
    assert r.g.dtype == r.c.dtype == r.W.dtype == np.float32 and (r.L, r.q, r.M) == (6, 4, 3)
    other = str(tmp_path / "other.npz")
    np.savez(other, **{k: getattr(m, k) for k in rbm.FIELDS})
    with pytest.raises(ValueError, match="kind"):
        rbm.load(other)
    np.savez(other, kind="ar", **{k: getattr(m, k) for k in rbm.FIELDS})
    with pytest.raises(ValueError, match="kind"):
        rbm.load(other)


# ---- the library's argument checks ------------------------------------------------------------------------------------

def _code(fn, *a, **kw):
    with pytest.raises(_lib.PlmError) as e:
        fn(*a, **kw)
    return e.value.code


L0, Q0, M0, N0 = 4, 3, 2, 6
G0, C0, WT0 = cases.model(L0, Q0, M0)
X0 = np.random.default_rng(2).integers(0, Q0, (N0, L0)).astype(np.int8)
WGT0 = np.ones(N0, np.float32)


def _wide(q):
    return np.zeros((L0, q), np.float32), np.zeros(M0, np.float32), np.zeros((M0, L0, q), np.float32)


def test_score_arguments():
    for v in (Q0, -1):
        bad = X0.copy()
        bad[3, 2] = v
        assert _code(plm.rbm_score, bad, Q0, G0, C0, WT0) == EINVAL
    assert _code(plm.rbm_score, X0[:0], Q0, G0, C0, WT0) == EINVAL
    assert _code(plm.rbm_score, X0, 33, *_wide(33)) == EUNSUPPORTED
    assert _code(plm.rbm_score, X0, 1, *_wide(1)) == EUNSUPPORTED
    lib = _lib.load()
    x = np.zeros(plm.rbm_n_params(L0, Q0, M0), np.float32)
    out = np.zeros(N0)
    p = lambda a: a.ctypes.data
    assert lib.plm_rbm_score(None, N0, L0, Q0, M0, p(x), 0, None, p(out), None) == EINVAL
    assert lib.plm_rbm_score(p(X0), N0, L0, Q0, M0, None, 0, None, p(out), None) == EINVAL
    assert lib.plm_rbm_score(p(X0), N0, L0, Q0, M0, p(x), 0, None, None, None) == EINVAL
    assert lib.plm_rbm_score(p(X0), N0, 0, Q0, M0, p(x), 0, None, p(out), None) == EINVAL
    assert lib.plm_rbm_score(p(X0), N0, L0, Q0, 0, p(x), 0, None, p(out), None) == EINVAL
    # M L q at or above 2^31: refused before anything is read
    assert lib.plm_rbm_score(p(X0), N0, L0, Q0, 1 << 28, p(x), 0, None, p(out), None) == EINVAL


def test_sample_arguments():
    smp = lambda **kw: plm.rbm_sample(G0, C0, WT0, Q0, kw.pop("n", 8), **kw)
    assert _code(smp, n=0) == EINVAL
    assert _code(smp, n_snapshots=0) == EINVAL
    assert _code(smp, burn_in=-1) == EINVAL
    assert _code(smp, thin=0) == EINVAL
    assert _code(smp, allowed=np.zeros(Q0, bool)) == EINVAL
    bad = np.zeros((8, L0), np.int8)
    bad[2, 1] = Q0
    assert _code(smp, start=bad) == EINVAL
    allowed = np.array([False, True, True])
    assert _code(smp, start=np.zeros((8, L0), np.int8), allowed=allowed) == EINVAL          # state 0 is not allowed
    assert _code(smp, first_step=0xFFFFFFF0, burn_in=100) == EINVAL
    assert _code(smp, first_chain=0xFFFFFFFF, n=2) == EINVAL
    assert _code(plm.rbm_sample, *_wide(33), 33, 8) == EUNSUPPORTED
    lib = _lib.load()
    x = np.zeros(plm.rbm_n_params(L0, Q0, M0), np.float32)
    out = np.zeros((1, 8, L0), np.int8)
    assert lib.plm_rbm_sample(L0, Q0, M0, x.ctypes.data, None, 0, None, out.ctypes.data, None) == EINVAL


def test_fit_arguments():
    fit = lambda **kw: plm.rbm_fit(kw.pop("x", X0), kw.pop("w", WGT0), kw.pop("q", Q0), G0, C0, WT0, kw.pop("C", 8),
                                   kw.pop("E", 2), **kw)
    assert _code(fit, C=0) == EINVAL
    assert _code(fit, E=0) == EINVAL
    assert _code(fit, steps_per_epoch=0) == EINVAL
    assert _code(fit, first_epoch=-1) == EINVAL
    assert _code(fit, lr_decay_after=-1) == EINVAL
    for name in ("lr", "lambda_g", "lambda_w"):
        for v in (-0.5, np.nan, np.inf):
            assert _code(fit, **{name: v}) == EINVAL
    for k, v in ((1, -0.5), (2, np.nan), (0, np.inf)):
        w = WGT0.copy()
        w[k] = v
        assert _code(fit, w=w) == EINVAL
    assert _code(fit, w=0 * WGT0) == EINVAL
    bad = X0.copy()
    bad[5, 3] = 9
    assert _code(fit, x=bad) == EINVAL
    bad_start = np.full((8, L0), Q0, np.int8)
    assert _code(fit, start=bad_start) == EINVAL
    assert _code(fit, first_epoch=2 ** 31 - 3, E=2, steps_per_epoch=3) == EINVAL            # (e0 + E) k >= 2^32 - 1
    assert _code(plm.rbm_fit, X0, WGT0, 33, *_wide(33), 8, 2) == EUNSUPPORTED
    lib = _lib.load()
    x = np.zeros(plm.rbm_n_params(L0, Q0, M0), np.float32)
    opts = _lib.PlmRbmFitOpts(8, 2, 2, 0, 0, 0.1, 0.0, 0.0, 0, None)
    res = _lib.PlmRbmFitResult()
    import ctypes as C
    args = lambda msa, w, xs, o, r: (msa, w, N0, L0, Q0, M0, xs, o, 0, None, _lib.RBM_EPOCH_CB(), None, r)
    p = lambda a: a.ctypes.data
    assert lib.plm_rbm_fit(*args(p(X0), p(WGT0), None, C.byref(opts), C.byref(res))) == EINVAL      # x_start is required
    assert lib.plm_rbm_fit(*args(None, p(WGT0), p(x), C.byref(opts), C.byref(res))) == EINVAL
    assert lib.plm_rbm_fit(*args(p(X0), None, p(x), C.byref(opts), C.byref(res))) == EINVAL
    assert lib.plm_rbm_fit(*args(p(X0), p(WGT0), p(x), None, C.byref(res))) == EINVAL
    assert lib.plm_rbm_fit(*args(p(X0), p(WGT0), p(x), C.byref(opts), None)) == EINVAL


def test_valid_calls_need_a_device():
    """Without a gfx950 device a valid call raises PlmError (no fall-back); with one it answers."""
    calls = [lambda: plm.rbm_score(X0, Q0, G0, C0, WT0), lambda: plm.rbm_sample(G0, C0, WT0, Q0, 8),
             lambda: plm.rbm_fit(X0, WGT0, Q0, G0, C0, WT0, 8, 2)]
    if _lib.load().plm_device_count() > 0:
        assert plm.rbm_score(X0, Q0, G0, C0, WT0).shape == (N0,)
        return
    for call in calls:
        assert _code(call) == -3


# ---- the conditions the device tests rest on --------------------------------------------------------------------------

@pytest.mark.parametrize("L,q,M,C,variant,seed,steps", cases.DRAW_CASES)
def test_float32_mode_follows_the_float64_twin(L, q, M, C, variant, seed, steps):
    """The 1 % cap of the near-tie rule is a condition: rounding the sums as the contract does changes at most 0.5 % of the
    chains of every (shape, seed) the device tests use."""
    g, c, W = cases.model(L, q, M)
    kw = cases.draw_options(L, q, C, variant, seed)
    with np.errstate(over="ignore"):
        s32, h32, _ = tw.run(g, c, W, C, steps, seed=seed, f32=True, **kw)
    s64, h64, rec = tw.run(g, c, W, C, steps, seed=seed, **kw)
    differ = ((s32 != s64).any(axis=(0, 2)) | (h32 != h64).any(axis=(0, 2))).sum()
    print("L=%d q=%d M=%d C=%d %s: %d chains differ between the float32 and the float64 twin" % (L, q, M, C, variant, differ))
    assert differ <= 0.005 * C
    # and where they differ, the near-tie rule explains it
    tw.explained("float32 twin", s32, h32, s64, h64, rec, q, cap=0.005)


def test_float32_mode_at_the_chi_square_and_learning_shapes():
    L, q, M = cases.CHI_SHAPE
    g, c, W = cases.model(L, q, M)
    C = 2000
    s32, h32, _ = tw.run(g, c, W, C, cases.CHI_STEPS, seed=cases.CHI_SEED, f32=True)
    s64, h64, _ = tw.run(g, c, W, C, cases.CHI_STEPS, seed=cases.CHI_SEED)
    assert ((s32 != s64).any(axis=(0, 2)) | (h32 != h64).any(axis=(0, 2))).sum() <= 0.005 * C


@pytest.mark.parametrize("L,q,M,N,C,E,k,seed", cases.FIT_CASES)
def test_fit_cases_have_no_near_tie(L, q, M, N, C, E, k, seed):
    msa, w, (g, c, W) = cases.fit_data(L, q, M, N, seed)
    r = tw.fit(msa, w, q, g, c, W, C, E, steps_per_epoch=k, seed=seed, **cases.FIT_OPTS)
    print("L=%d q=%d M=%d N=%d C=%d: smallest margin / delta = %.3g" % (L, q, M, N, C, r["worst"]))
    assert r["worst"] > 1.0
    assert r["epochs_done"] == E and r["trace"].shape == (E, 5)
    for part in r["data"] + r["model"]:
        assert (part >= 0.0).all() and (part <= 1.0 + 1e-15).all()
    np.testing.assert_allclose(r["data"][0].sum(axis=1), 1.0, atol=1e-14)


def test_twin_fit_resumes_and_stops():
    L, q, M, N, C, _, k, seed = cases.FIT_CASES[6]
    msa, w, (g, c, W) = cases.fit_data(L, q, M, N, seed)
    whole = tw.fit(msa, w, q, g, c, W, C, 4, steps_per_epoch=k, seed=seed, lr_decay_after=2, **cases.FIT_OPTS)
    a = tw.fit(msa, w, q, g, c, W, C, 2, steps_per_epoch=k, seed=seed, lr_decay_after=2, **cases.FIT_OPTS)
    b = tw.fit(msa, w, q, a["g"], a["c"], a["W"], C, 2, steps_per_epoch=k, seed=seed, lr_decay_after=2, start=a["chains"],
               first_epoch=2, **cases.FIT_OPTS)
    assert np.array_equal(whole["x"], b["x"]) and np.array_equal(whole["chains"], b["chains"])
    assert np.array_equal(whole["trace"], np.concatenate([a["trace"], b["trace"]]))
    assert whole["trace"][3, 3] == cases.FIT_OPTS["lr"] * 2 / 4
    s = tw.fit(msa, w, q, g, c, W, C, 4, steps_per_epoch=k, seed=seed, stop_at=1, **cases.FIT_OPTS)
    one = tw.fit(msa, w, q, g, c, W, C, 1, steps_per_epoch=k, seed=seed, **cases.FIT_OPTS)
    assert s["status"] == "interrupted" and s["epochs_done"] == 1 and len(s["trace"]) == 2 and np.array_equal(s["x"], one["x"])


def test_twin_histogram_after_a_few_steps():
    """The chi-square test of test_gpu_rbm.py, passed by the twin's own chains first."""
    L, q, M = cases.CHI_SHAPE
    g, c, W = cases.model(L, q, M)
    states, _, _ = tw.run(g, c, W, cases.CHI_CHAINS, cases.CHI_STEPS, seed=cases.CHI_SEED)
    mu = st.start_distribution(g.astype(np.float64)) @ np.linalg.matrix_power(tw.transition_matrix(g, c, W), cases.CHI_STEPS)
    counts = np.bincount(st.state_index(states[-1], q), minlength=q ** L)
    chi, dof = st.chi2_counts(counts, mu, cases.CHI_CHAINS)
    bound = stats.chi2.isf(1e-6, dof)
    print("twin: chi2 = %.1f on %d degrees of freedom (bound %.1f)" % (chi, dof, bound))
    assert chi < bound
    # the test has power: the start distribution itself fails it
    assert st.chi2_counts(counts, st.start_distribution(g.astype(np.float64)), cases.CHI_CHAINS)[0] > bound


def test_twin_learns_the_planted_model():
    """The rehearsal of test_gpu_rbm's learning test: lr and the epoch count are chosen so that the twin passes with room."""
    L, q, M = cases.LEARN["shape"]
    data, _ = cases.planted_data()
    w = np.ones(len(data), np.float32)
    g0, c0, W0 = rbm.start_point(data, w, q, M)
    r = tw.fit(data, w, q, g0, c0, W0, cases.LEARN["C"], cases.LEARN["epochs"], steps_per_epoch=cases.LEARN["steps"],
               lr=cases.LEARN["lr"], seed=cases.LEARN["seed"])
    ll0 = tw.mean_log_likelihood(data, w, g0, c0, W0)
    ll1 = tw.mean_log_likelihood(data, w, r["g"], r["c"], r["W"])
    print("mean log-likelihood: %.4f at the start, %.4f after %d epochs" % (ll0, ll1, r["epochs_done"]))
    assert ll1 > ll0 + 0.04
