"""The autoregressive Potts model without a device (DESIGN_NEXT_ROWS.md section 9.19): the float64 twin against itself
(normalisation by enumeration, gradient against central differences, repack round trip), the Python layer (site order,
model file), and the argument checks of the four entry points, which come before the device is looked at."""
import numpy as np
import pytest

import ar_twin as tw
import sampler_twin as st
from evcouplings_amd import _lib, ar_model, plm

EINVAL, EUNSUPPORTED = -1, -4


@pytest.mark.parametrize("L,q", [(5, 3), (3, 4)])
def test_twin_probabilities_sum_to_one(L, q):
    h, J = tw.random_model(L, q)
    xs = st.all_states(L, q)
    lp = tw.logp(xs, h, J)
    assert abs(np.exp(lp).sum() - 1.0) < 1e-13
    np.testing.assert_allclose(tw.enumerate_p(h, J), np.exp(lp), rtol=1e-12, atol=0)
    allowed = np.ones(q, bool)
    allowed[0] = False
    p = tw.enumerate_p(h, J, beta=0.5, allowed=allowed)
    assert abs(p.sum() - 1.0) < 1e-13 and p[(xs == 0).any(axis=1)].sum() == 0.0


def test_twin_gradient_against_central_differences():
    L, q, n = 4, 3, 50
    rng = np.random.default_rng(5)
    h, J = tw.random_model(L, q)
    x = rng.integers(0, q, (n, L))
    w = rng.uniform(0.2, 1.0, n)
    lh, lj = 0.02, 0.03
    F, nll, gh, gJ = tw.objective(x, w, h, J, lh, lj)
    g = tw.pack(gh, gJ)
    p0 = tw.pack(h, J)
    eps = 1e-6
    for k in range(p0.size):
        e = np.zeros_like(p0)
        e[k] = eps
        fp = tw.objective(x, w, *tw.unpack(p0 + e, L, q), lh, lj, gradient=False)[0]
        fm = tw.objective(x, w, *tw.unpack(p0 - e, L, q), lh, lj, gradient=False)[0]
        # central differences of a smooth function: error ~ eps^2 |F'''| + rounding 1e-16 |F| / eps
        assert abs((fp - fm) / (2 * eps) - g[k]) < 1e-8, k
    assert nll > 0 and F > nll


def test_twin_first_site_and_block_orientation():
    """h_0 alone is the first site's conditional; entry [a][b] of block (j, i) couples state a of the earlier site"""
    L, q = 3, 4
    h, J = tw.random_model(L, q)
    x = np.array([[1, 2, 3]])
    site = tw.site_logp(x, h, J)[0]
    h64, J64 = h.astype(np.float64), J.astype(np.float64)
    lse = lambda u: np.log(np.exp(u - u.max()).sum()) + u.max()
    assert abs(site[0] - (h64[0, 1] - lse(h64[0]))) < 1e-14
    u1 = h64[1] + J64[tw.pair_index(0, 1, L)][1, :]
    assert abs(site[1] - (u1[2] - lse(u1))) < 1e-14
    u2 = h64[2] + J64[tw.pair_index(0, 2, L)][1, :] + J64[tw.pair_index(1, 2, L)][2, :]
    assert abs(site[2] - (u2[3] - lse(u2))) < 1e-14


@pytest.mark.parametrize("L,q", [(1, 7), (2, 3), (6, 5), (9, 21)])
def test_repack_round_trip(L, q):
    _, J = tw.random_model(L, q)
    T = tw.repack(J, L, q)
    assert T.shape == (L * (L - 1) // 2, q, (q + 3) // 4 * 4)
    assert np.array_equal(tw.unrepack(T, L, q), J)
    assert not T[:, :, q:].any()
    if L > 2:      # table i holds the blocks (0, i) .. (i - 1, i) in that order
        assert np.array_equal(T[3 * 2 // 2 + 1, :, :q], J[tw.pair_index(1, 3, L)]) if L > 3 else True
        assert np.array_equal(T[2 * 1 // 2 + 0, :, :q], J[tw.pair_index(0, 2, L)])


def test_entropic_order():
    fi = np.array([[0.25, 0.25, 0.25, 0.25], [1.0, 0.0, 0.0, 0.0], [0.5, 0.5, 0.0, 0.0], [0.0, 2.0, 0.0, 0.0],
                   [0.5, 0.0, 0.5, 0.0]])
    assert ar_model.entropic_order(fi).tolist() == [1, 3, 2, 4, 0]
    H = ar_model.site_entropies(fi)
    np.testing.assert_allclose(H, [np.log(4), 0, np.log(2), 0, np.log(2)], atol=1e-15)
    msa = np.array([[0, 1, 2], [0, 1, 0], [0, 2, 1], [0, 1, 1]])
    f = ar_model.weighted_frequencies(msa, np.ones(4), 3)
    np.testing.assert_allclose(f.sum(axis=1), 1.0)
    assert ar_model.entropic_order(f).tolist() == [0, 1, 2]
    with pytest.raises(ValueError):
        ar_model._resolve_order([0, 0, 1], msa, np.ones(4), 3)


def _model(L=6, q=4):
    from types import SimpleNamespace
    h, J = tw.random_model(L, q)
    return SimpleNamespace(hi=h, jij=J, order=np.random.default_rng(1).permutation(L), alphabet="-ACD", L=L, q=q,
                           index_list=np.arange(10, 10 + L, dtype=np.int32), target_seq="ACD-AC", lambda_h=1e-4,
                           lambda_j=1e-2, n_eff=12.5, theta=0.8)


def test_save_load_round_trip_and_refusal(tmp_path):
    m = _model()
    path = ar_model.save(str(tmp_path / "m.npz"), m)
    r = ar_model.load(path)
    for k in ar_model.FIELDS:
        a, b = getattr(m, k), getattr(r, k)
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, k
    assert r.hi.dtype == np.float32 and r.jij.dtype == np.float32 and (r.L, r.q) == (6, 4)
    other = str(tmp_path / "potts.npz")
    np.savez(other, **{k: getattr(m, k) for k in ar_model.FIELDS})
    with pytest.raises(ValueError, match="kind"):
        ar_model.load(other)
    np.savez(other, kind="potts", **{k: getattr(m, k) for k in ar_model.FIELDS})
    with pytest.raises(ValueError, match="kind"):
        ar_model.load(other)


# ---- the library's argument checks ------------------------------------------------------------------------------------

def _code(fn, *a, **kw):
    with pytest.raises(_lib.PlmError) as e:
        fn(*a, **kw)
    return e.value.code


L0, Q0, N0 = 4, 3, 6
H0, J0 = tw.random_model(L0, Q0)
X0 = np.random.default_rng(2).integers(0, Q0, (N0, L0)).astype(np.int8)
W0 = np.ones(N0, np.float32)


def _wide(q):
    return np.zeros((L0, q), np.float32), np.zeros((L0 * (L0 - 1) // 2, q, q), np.float32)


def test_logprob_arguments():
    bad = X0.copy()
    bad[3, 2] = Q0
    assert _code(plm.ar_logprob, bad, Q0, H0, J0) == EINVAL
    bad[3, 2] = -1
    assert _code(plm.ar_logprob, bad, Q0, H0, J0) == EINVAL
    assert _code(plm.ar_logprob, X0, 33, *_wide(33)) == EUNSUPPORTED
    assert _code(plm.ar_logprob, X0, 1, *_wide(1)) == EUNSUPPORTED


def test_sample_arguments():
    assert _code(plm.ar_sample, H0, J0, Q0, 0) == EINVAL
    for beta in (0.0, -1.0, np.inf, np.nan):
        assert _code(plm.ar_sample, H0, J0, Q0, 8, beta=beta) == EINVAL
    assert _code(plm.ar_sample, H0, J0, Q0, 8, allowed=np.zeros(Q0, bool)) == EINVAL
    assert _code(plm.ar_sample, *_wide(33), 33, 8) == EUNSUPPORTED


def test_eval_arguments():
    for k, v in ((1, -0.5), (2, np.nan), (0, np.inf)):
        w = W0.copy()
        w[k] = v
        assert _code(plm.ar_evaluate, X0, w, Q0, 0.01, 0.01, H0, J0) == EINVAL
    assert _code(plm.ar_evaluate, X0, 0 * W0, Q0, 0.01, 0.01, H0, J0) == EINVAL
    assert _code(plm.ar_evaluate, X0, W0, Q0, -0.01, 0.01, H0, J0) == EINVAL
    assert _code(plm.ar_evaluate, X0, W0, Q0, 0.01, -0.01, H0, J0) == EINVAL
    bad = X0.copy()
    bad[0, 0] = Q0
    assert _code(plm.ar_evaluate, bad, W0, Q0, 0.01, 0.01, H0, J0) == EINVAL
    assert _code(plm.ar_evaluate, X0, W0, 33, 0.01, 0.01, *_wide(33)) == EUNSUPPORTED


def test_fit_arguments():
    fit = lambda **kw: plm.ar_fit(X0, kw.pop("w", W0), kw.pop("q", Q0), kw.pop("lh", 0.01), kw.pop("lj", 0.01), **kw)
    assert _code(fit, lbfgs_m=0) == EINVAL
    assert _code(fit, lbfgs_m=21) == EINVAL
    assert _code(fit, epsilon=0.0) == EINVAL
    assert _code(fit, epsilon=np.nan) == EINVAL
    assert _code(fit, max_iter=-1) == EINVAL
    assert _code(fit, lh=-1.0) == EINVAL
    assert _code(fit, w=0 * W0) == EINVAL
    assert _code(fit, w=-W0) == EINVAL
    assert _code(fit, q=33) == EUNSUPPORTED
    bad = X0.copy()
    bad[5, 3] = 9
    assert _code(plm.ar_fit, bad, W0, Q0, 0.01, 0.01) == EINVAL


def test_valid_calls_need_a_device():
    """Without a gfx950 device a valid call raises PlmError (no fall-back); with one it answers."""
    calls = [lambda: plm.ar_logprob(X0, Q0, H0, J0), lambda: plm.ar_sample(H0, J0, Q0, 8),
             lambda: plm.ar_evaluate(X0, W0, Q0, 0.01, 0.01, H0, J0), lambda: plm.ar_fit(X0, W0, Q0, 0.01, 0.01, max_iter=2)]
    if _lib.load().plm_device_count() > 0:
        assert plm.ar_logprob(X0, Q0, H0, J0).shape == (N0,)
        return
    for call in calls:
        with pytest.raises(_lib.PlmError) as e:
            call()
        assert e.value.code == -3
