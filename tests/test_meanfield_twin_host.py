"""
CPU: the references of tests/meanfield_twin.py against the reference's own numbers (tests/golden/meanfield_{a,d}.npz),
against mpmath, and against each other -- and the check that no DI input of tests/test_gpu_meanfield.py has a pair
whose iteration count depends on rounding, so that the GPU tests can compare every pair.
"""
import os
import sys

import mpmath
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meanfield_twin as tw  # noqa: E402

from oracle import meanfield_ref  # noqa: E402


@pytest.fixture(scope="module", params=["a", "d"])
def golden(request, golden_dir):
    return np.load(os.path.join(golden_dir, "meanfield_%s.npz" % request.param))


def cpu_model(oracle64, q, L, N, pc):
    """the mean-field couplings and regularised frequencies of a planted alignment, all on the CPU, from frequencies
    rounded to float32 as the library hands them out"""
    msa = tw.planted_msa(q, L, N)
    w = 1.0 / oracle64.reweight(msa, tw.THETA)
    fi, fij = oracle64.marginals(msa, w, q)
    fi, fij = fi.astype(np.float32).astype(np.float64), fij.astype(np.float32).astype(np.float64)
    C = tw.covariance(fi, fij, pc)
    return C, tw.couplings_from_inverse(np.linalg.inv(C), L, q), (1.0 - pc) * fi + pc / q


def test_covariance_is_the_oracles_and_the_references(golden):
    pc = float(golden["pseudo_count"])
    C = tw.covariance(golden["fi"], golden["fij_pairs"], pc)
    np.testing.assert_allclose(C, golden["cov"], rtol=0, atol=1e-15)          # as rfi is pinned in test_oracle.py
    assert np.array_equal(C, C.T)
    L, q = golden["fi"].shape
    ref = meanfield_ref.mean_field(golden["fi"], golden["fij_pairs"], pc, want_di=False)
    assert np.array_equal(tw.couplings_from_inverse(np.linalg.inv(C), L, q), ref["jij_full"])   # the same expression


def test_extended_inverse_brackets_the_reference(golden):
    C = golden["cov"]
    L, q = golden["fi"].shape
    info = {}
    ext = tw.inverse_extended(C, info)
    assert ext.dtype == np.longdouble and len(info["residuals"]) >= 2
    assert info["residuals"][0] < 1e-12 and info["residuals"][-1] < 2.0 ** -60
    err_lu, err_chol = tw.inverse_errors(C, ext)
    assert 2.0 ** -54 < err_lu < 1e-12 and 2.0 ** -54 < err_chol < 1e-12
    J = tw.couplings_from_inverse(ext, L, q)
    err = float(np.abs(golden["jij_full"] - J).max() / np.abs(ext).max())
    print("golden jij_full against the extended inverse: %.3g, err_lu %.3g, err_chol %.3g" % (err, err_lu, err_chol))
    # the golden is numpy's LU inverse, so it misses the extended inverse by err_lu; the factor 2 is for a BLAS that
    # sums in another order than the one the golden was recorded with
    assert err <= 2.0 * max(err_lu, err_chol)


def test_extended_inverse_against_mpmath():
    """n = 60 (q = 21, L = 3 of the geometry table, on random frequencies): 40-digit inverse"""
    rng = np.random.default_rng(5)
    A = rng.normal(size=(60, 90))
    C = A @ A.T / 90 + 0.01 * np.eye(60)
    mpmath.mp.dps = 40
    inv = mpmath.matrix(C.tolist()) ** -1
    want = np.array([[np.longdouble(mpmath.nstr(inv[r, c], 25)) for c in range(60)] for r in range(60)])
    got = tw.inverse_extended(C)
    assert float(np.abs(got - want).max() / np.abs(want).max()) < 2.0 ** -56          # 1/16 of the smallest yardstick


def test_both_routes_of_the_extended_inverse_agree(golden, monkeypatch):
    """the longdouble products (small n) and the sliced float64 products (large n) on the same matrix, and the true
    residual of the sliced route's result, formed in longdouble"""
    C = golden["cov"][:150, :150]
    assert C.shape[0] <= tw.LD_DIRECT_MAX
    direct = tw.inverse_extended(C)
    monkeypatch.setattr(tw, "LD_DIRECT_MAX", 0)
    R_sliced = tw.residual(C, np.linalg.inv(C))
    sliced = tw.inverse_extended(C)
    monkeypatch.undo()
    assert np.abs(R_sliced - tw.residual(C, np.linalg.inv(C))).max() < 2.0 ** -58
    assert float(np.abs(direct - sliced).max() / np.abs(direct).max()) < 2.0 ** -56     # 1/16 of the smallest yardstick
    true_res = np.eye(150, dtype=np.longdouble) - C.astype(np.longdouble) @ sliced
    assert np.abs(true_res).max() < 1e-16


def test_sliced_route_leaves_a_true_longdouble_residual_at_n500():
    """the route taken above n = LD_DIRECT_MAX, at a size where nothing else checks it: the residual I - C X of its
    result, formed by a plain longdouble product (one product, about a second), is where the direct route ends too"""
    rng = np.random.default_rng(11)
    A = rng.normal(size=(500, 520))
    C = A @ A.T / 520 + 1e-4 * np.eye(500)
    assert C.shape[0] > tw.LD_DIRECT_MAX and np.linalg.cond(C) > 1e3
    info = {}
    X = tw.inverse_extended(C, info)
    assert X.dtype == np.longdouble and info["residuals"][0] > 1e-14
    true_res = np.eye(500, dtype=np.longdouble) - C.astype(np.longdouble) @ X
    print("true residual of the sliced route at n = 500: %.3g" % float(np.abs(true_res).max()))
    assert np.abs(true_res).max() < 1e-16


def test_fields_from_reproduces_the_reference(golden):
    h, B = tw.fields_from(golden["jij_full"], golden["rfi"])
    n = golden["cov"].shape[0]
    assert (np.abs(h - golden["hi"]) <= tw.fields_bound(B, golden["rfi"], n)).all()
    assert not h[:, -1].any()                                  # zero last row of every block, log(1) = 0


def test_traced_di_is_the_oracles(golden):
    di, iters, gap = tw.direct_information_traced(golden["jij_full"], golden["rfi"])
    assert np.array_equal(di, meanfield_ref.direct_information(golden["jij_full"], golden["rfi"]))
    L = di.shape[0]
    off = ~np.eye(L, dtype=bool)
    assert (iters[off] >= 1).all() and not iters.diagonal().any() and np.array_equal(iters, iters.T)
    assert np.isfinite(gap[off]).all() and np.array_equal(gap, gap.T)


def test_planted_alignment():
    msa = tw.planted_msa(5, 16, 300)
    assert msa.dtype == np.int8 and msa.min() == 0 and msa.max() == 4
    (a, b), (c, d) = tw.planted_pairs(16)
    assert np.array_equal(msa[:, a], msa[:, b])
    assert 0.85 < (msa[:, c] == msa[:, d]).mean() < 1.0
    assert np.array_equal(msa, tw.planted_msa(5, 16, 300))
    assert tw.planted_pairs(3)[1] is None and tw.planted_pairs(2)[0] == (0, 1)


@pytest.mark.parametrize("q,L,N,pc", [(q, L, N, 0.5) for (q, L, N) in tw.GEOMETRY_CASES] + tw.CONDITIONING_CASES)
def test_no_alignment_case_is_stop_rule_ambiguous(oracle64, q, L, N, pc):
    """every (q, L, N, pseudo-count) of the GPU file, with the inverse and the frequencies of the CPU: the references
    are finite, the matrix is positive definite, and no pair's diff comes within 1e-10 of the stop threshold.
    (21, 12, 60, 0.01) takes about 15 s here, the others 2 s at most: its two planted pairs overflow, and the oracle's
    Python loop spends 7.6e4 updates on a neighbouring pair and as long on the NaN ones before it leaves them."""
    C, J, rfi = cpu_model(oracle64, q, L, N, pc)
    np.linalg.cholesky(C)
    with np.errstate(all="ignore"):
        di, iters, gap = tw.direct_information_traced(J, rfi)
    (a, b), second = tw.planted_pairs(L)
    if (q, L, N, pc) in tw.DI_OVERFLOWS:
        bad = np.zeros((L, L), bool)
        for i, j in ((a, b), second):
            bad[i, j] = bad[j, i] = True
        assert np.array_equal(~np.isfinite(di), bad)
    else:
        assert np.isfinite(di).all()
    assert tw.ambiguous_pairs(gap) == [], "change the seed of this case"
    assert iters.max() < tw.DI_UPDATE_CAP                      # k_mf_di's loop is capped, the oracle's is not
    if (q, L, N, pc) not in tw.ORACLE_COPY_NOT_ON_TOP:
        assert di[a, b] == np.nanmax(di)


def test_conditioning_cases_reach_a_hard_matrix(oracle64):
    conds = [np.linalg.cond(cpu_model(oracle64, *case)[0]) for case in tw.CONDITIONING_CASES]
    assert max(conds) > 1e4 and min(conds) < 1e2


@pytest.mark.parametrize("q,L", tw.DI_MODEL_CASES)
def test_no_di_model_is_stop_rule_ambiguous(q, L):
    J, rfi, (i, j) = tw.random_di_model(q, L)
    assert J[0, 1, q - 1].all() and J[0, 1, :, q - 1].all()            # not in the mean-field gauge
    assert np.array_equal(J[1, 0], J[0, 1].T)
    di, iters, gap = tw.direct_information_traced(J, rfi)
    assert np.isfinite(di).all()
    assert tw.ambiguous_pairs(gap) == [], "change the seed of this case"
    assert iters.max() < tw.DI_UPDATE_CAP
    if L > 2:                                                          # at L = 2 the strong pair is the median
        assert iters[i, j] > np.median(iters[np.triu_indices(L, 1)])   # the strong pair reaches a long loop


def test_overflowing_model_is_not_ambiguous_elsewhere():
    J, rfi, bad = tw.overflowing_di_model()
    with np.errstate(all="ignore"):
        di, iters, gap = tw.direct_information_traced(J, rfi)
    finite = np.isfinite(di)
    assert not finite[bad] and not finite[bad[::-1]] and finite.sum() == di.size - 2
    assert tw.ambiguous_pairs(gap) == []
