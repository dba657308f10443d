"""
GPU: the analysis kernels behind CouplingsModel (plm_model_pair_scores, plm_double_mutants, plm_independent_fields)
against the reference's numbers (tests/golden/model_analysis_L24.npz, make_golden_model_analysis.py) and, at sizes the
fixture does not reach, against the float64 numpy twins of tests/model_twins.py.  The reference is absent here: the
model is read with model_io.read_model_file and expanded densely in the test.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import model_twins as tw  # noqa: E402

from evcouplings_amd import _lib, model_io, plm  # noqa: E402

pytestmark = pytest.mark.gpu
ALPHABET = "-ACDEFGHIKLMNPQRSTVWY"
NEWTON_CAP = 100


@pytest.fixture(scope="module")
def golden(golden_dir):
    m = model_io.read_model_file(os.path.join(golden_dir, "hip_fit_L24.model"))
    z = np.load(os.path.join(golden_dir, "model_analysis_L24.npz"))
    L = m["L"]
    return dict(m=m, z=z, L=L, J=tw.dense_from_pairs(m["jij"], L), F=tw.dense_from_pairs(m["fij"], L),
                target=np.array([ALPHABET.index(c) for c in m["target_seq"]], np.int8))


def random_model(L, q, seed, zeros=0.3):
    """random couplings and normalised pair frequencies with about `zeros` exact zeros; f_i the marginals of f_ij"""
    rng = np.random.default_rng(seed)
    iu, ju = np.triu_indices(L, 1)
    Jb = rng.normal(size=(len(iu), q, q))
    Fb = rng.random(size=(len(iu), q, q)) * (rng.random(size=(len(iu), q, q)) >= zeros)
    Fb[Fb.sum(axis=(1, 2)) == 0, 0, 0] = 1.0        # q = 2 can mask a whole block
    Fb /= Fb.sum(axis=(1, 2), keepdims=True)
    fi = rng.random(size=(L, q))
    fi /= fi.sum(axis=1, keepdims=True)
    return tw.dense_from_pairs(Jb, L), tw.dense_from_pairs(Fb, L), fi


def assert_rel(got, want, rtol=1e-12):
    np.testing.assert_allclose(got, want, rtol=rtol, atol=rtol * np.abs(want[np.isfinite(want)]).max() * 1e-3)


def test_pair_scores_reproduce_the_reference(golden):
    z, m = golden["z"], golden["m"]
    fn, mi = plm.model_pair_scores(golden["J"], golden["F"], m["fi"])     # float32 f_i, as the .model file holds it
    assert_rel(fn, z["fn_scores"])
    assert_rel(mi, z["mi_scores_raw"])
    np.testing.assert_allclose(tw.apc(fn), z["cn_scores"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(tw.apc(mi), z["mi_scores_apc"], rtol=1e-12, atol=1e-13)
    L = golden["L"]
    iu, ju = np.triu_indices(L, 1)
    order = np.argsort(-tw.apc(fn)[iu, ju], kind="stable")
    idx = golden["m"]["index_list"]
    assert np.array_equal((idx[iu[order][:20]], idx[ju[order][:20]]), (z["ecs_i"][:20], z["ecs_j"][:20]))


def test_double_mutants_reproduce_the_reference(golden):
    z = golden["z"]
    D = plm.double_mutant_matrix(golden["J"], z["single_mut_mat"], golden["target"])
    p = z["dmm_pairs"]
    assert_rel(D[p[:, 0], p[:, 1]], z["dmm_blocks"])
    assert_rel(D[p[:, 1], p[:, 0]], z["dmm_blocks"].transpose(0, 2, 1))


def test_independent_fields_reach_the_optimum_the_reference_approaches(golden):
    z, m = golden["z"], golden["m"]
    lam, n_eff = float(z["lambda_h"]), float(z["n_eff"])
    h, iters = plm.independent_fields(m["fi"], lam, n_eff)
    fi = m["fi"].astype(np.float64)
    _, g_ref, _ = tw.objective(z["h_indep"], fi, lam, n_eff)
    _, g, _ = tw.objective(h, fi, lam, n_eff)
    # 2 lambda-strong convexity: the reference's fmin_bfgs stopped within |g(h_ref)|_2 / (2 lambda) of the optimum
    bound = np.linalg.norm(g_ref, axis=1) / (2 * lam)
    assert (np.abs(h - z["h_indep"]).max(axis=1) <= bound).all()
    assert np.abs(g).max() <= 1e-10 * n_eff
    assert (iters >= 1).all() and (iters < NEWTON_CAP).all()


def test_pair_scores_at_the_headline_shape():
    L, q = 300, 21
    J, F, fi = random_model(L, q, seed=1)
    fn, mi = plm.model_pair_scores(J, F, fi)
    fn_t, mi_t = tw.pair_scores(J, F, fi)
    assert_rel(fn, fn_t)
    assert_rel(mi, mi_t)
    assert np.all(np.diag(fn) == 0) and np.all(np.diag(mi) == 0)


@pytest.mark.parametrize("q", [2, 7, 32])
def test_every_alphabet_size(q):
    L = 40
    J, F, fi = random_model(L, q, seed=q)
    fn, mi = plm.model_pair_scores(J, F, fi)
    fn_t, mi_t = tw.pair_scores(J, F, fi)
    assert_rel(fn, fn_t)
    assert_rel(mi, mi_t)
    rng = np.random.default_rng(q)
    smm, target = rng.normal(size=(L, q)), rng.integers(0, q, size=L).astype(np.int8)
    np.testing.assert_array_equal(plm.double_mutant_matrix(J, smm, target), tw.double_mutants(J, smm, target))
    h, iters = plm.independent_fields(fi, 0.01, 250.0)
    _, g, _ = tw.objective(h, fi, 0.01, 250.0)
    assert np.abs(g).max() <= 1e-10 * 250.0 and (iters < NEWTON_CAP).all()
    h_t, _ = tw.independent_fields(fi, 0.01, 250.0)
    # both stop at |g|_inf <= 1e-12 N: each is within sqrt(q) 1e-12 N / (2 lambda) of the optimum
    np.testing.assert_allclose(h, h_t, rtol=0, atol=2 * np.sqrt(q) * 1e-12 * 250.0 / (2 * 0.01))


def test_two_sites():
    J, F, fi = random_model(2, 21, seed=7)
    fn, mi = plm.model_pair_scores(J, F, fi)
    fn_t, mi_t = tw.pair_scores(J, F, fi)
    assert_rel(fn, fn_t)
    assert_rel(mi, mi_t)
    smm, target = np.ones((2, 21)), np.array([3, 5], np.int8)
    np.testing.assert_array_equal(plm.double_mutant_matrix(J, smm, target), tw.double_mutants(J, smm, target))


def test_positive_pair_frequency_over_a_zero_marginal_gives_inf_not_nan():
    J, F, fi = random_model(5, 4, seed=3, zeros=0.0)
    fi[1, 2] = 0.0                    # f_ij(2, b) > 0 for pair (1, 3) while f_1(2) = 0
    fn, mi = plm.model_pair_scores(J, F, fi)
    fn_t, mi_t = tw.pair_scores(J, F, fi)
    assert mi[1, 3] == np.inf and mi[3, 1] == np.inf and mi[0, 1] == np.inf
    assert not np.isnan(mi).any()
    assert np.array_equal(np.isinf(mi), np.isinf(mi_t))
    fin = np.isfinite(mi_t)
    np.testing.assert_allclose(mi[fin], mi_t[fin], rtol=1e-12, atol=1e-15)
    assert_rel(fn, fn_t)


def test_double_mutants_at_L600():
    L, q = 600, 21
    rng = np.random.default_rng(600)
    iu, ju = np.triu_indices(L, 1)
    Jb = rng.normal(size=(len(iu), q, q))
    J = tw.dense_from_pairs(Jb, L)
    smm, target = rng.normal(size=(L, q)), rng.integers(0, q, size=L).astype(np.int8)
    D = plm.double_mutant_matrix(J, smm, target)
    for r0 in range(0, L, 100):                   # D[j,i] = D[i,j]^T, in row slabs (the array is 1.27 GB)
        assert np.array_equal(D[r0:r0 + 100], D[:, r0:r0 + 100].transpose(1, 0, 3, 2))
    assert not D[np.arange(L), np.arange(L)].any()
    t = target.astype(np.int64)
    for i, j in [(0, 1), (0, L - 1), (L - 2, L - 1), (17, 401), (299, 300)] + list(zip(iu[::9973], ju[::9973])):
        Jij = J[i, j]
        want = (smm[i][:, None] + smm[j][None, :] + Jij - Jij[:, t[j]][:, None] - Jij[t[i], :][None, :]
                + Jij[t[i], t[j]])
        np.testing.assert_array_equal(D[i, j], want)


def test_errors_leave_the_device_usable():
    J, F, fi = random_model(4, 33, seed=33)
    with pytest.raises(_lib.PlmError) as e:
        plm.model_pair_scores(J, F, fi)
    assert e.value.code == -4                      # PLM_EUNSUPPORTED
    with pytest.raises(_lib.PlmError) as e:
        plm.double_mutant_matrix(J, np.zeros((4, 33)), np.zeros(4, np.int8))
    assert e.value.code == -4
    J, F, fi = random_model(6, 21, seed=6)
    fn, _ = plm.model_pair_scores(J, F, fi)
    assert_rel(fn, tw.pair_scores(J, F, fi)[0])
    with pytest.raises(_lib.PlmError) as e:
        plm.independent_fields(fi, 0.0, 100.0)
    assert e.value.code == -1                      # PLM_EINVAL
    h, iters = plm.independent_fields(fi, 0.01, 100.0)
    assert np.abs(tw.objective(h, fi, 0.01, 100.0)[1]).max() <= 1e-10 * 100.0
