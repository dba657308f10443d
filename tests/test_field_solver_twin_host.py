"""
CPU: tests/field_solver_twin.py against the float64 oracle and against itself -- the twin is what
tests/test_gpu_field_solver.py holds the field solver's kernels to, so it is pinned here first:
  * its field gradient is the field part of the oracle's gradient (q = 4, 5, 7, 21, 25, 32 and gap mode);
  * its exact Hessian is the derivative of its gradient (central differences);
  * fed with Hessian sums from EVERY tile, the Sinkhorn-rescaled assembly of k_hsolve returns the exact Hessian;
  * its Newton iteration converges, and the distance to the optimum obeys the strong-convexity bound
    |h - h*| <= |g_h(h) - g_h(h*)| / (2 lambda_h) that the GPU tests rely on;
  * the capped step moves no field by more than 3.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import field_solver_twin as tw  # noqa: E402

from evcouplings_amd.synthetic import synthetic_msa  # noqa: E402

LAM = 0.01


def n_params(L, q):
    return L * q + L * (L - 1) // 2 * q * q


def problem(q, N, L, seed, gap=False, scale=0.1):
    rng = np.random.default_rng(seed)
    if q == 21:
        msa, _ = synthetic_msa(N, L, seed=seed)
    else:
        msa = rng.integers(0, q, size=(N, L)).astype(np.int8)
    w = rng.uniform(0.2, 1.0, size=N).astype(np.float32)
    x = scale * rng.normal(size=n_params(L, q - 1 if gap else q))
    return msa, w, x


@pytest.mark.parametrize("q,gap", [(4, False), (5, False), (7, False), (21, False), (25, False), (32, False), (21, True)])
def test_field_gradient_is_the_oracles(oracle64, q, gap):
    N, L = 300, 9
    msa, w, x = problem(q, N, L, seed=q + 100 * gap, gap=gap)
    HJ, h = tw.potentials(msa, x, q, gap)
    live = tw.live_states(q, gap)
    sums = tw.tile_sums(HJ, h, msa, w, q, gap)
    assert sums["g"].shape[0] == 2                                   # a full tile and a partial one
    g = tw.field_gradient(sums, h, LAM, live)
    ev = oracle64.eval_gaps if gap else oracle64.eval
    qm = q - 1 if gap else q
    fx, nll, g_o = ev(msa, w.astype(np.float64), q, LAM, 0.3, x)
    g_o = g_o[:L * qm].reshape(L, qm)
    assert np.abs(g[:, live] - g_o).max() <= 1e-10 * np.abs(g_o).max()
    assert not g[:, ~live].any()
    assert sums["nll"].sum() == pytest.approx(nll, rel=1e-12)
    # the counts are the weighted one-hot sums, and m_a = gradient sum + count = sum w P_a sums to the weight per site
    ws = w.astype(np.float64)[:, None] * ((msa != 0) if gap else np.ones_like(msa))
    np.testing.assert_allclose((sums["g"] + sums["cnt"]).sum(axis=(0, 2)), ws.sum(axis=0), rtol=1e-12)


@pytest.mark.parametrize("q,gap", [(5, False), (21, True)])
def test_exact_hessian_is_the_derivative_of_the_gradient(q, gap):
    N, L = 120, 4
    msa, w, x = problem(q, N, L, seed=3, gap=gap, scale=0.3)
    HJ, h = tw.potentials(msa, x, q, gap)
    live = tw.live_states(q, gap)
    H = tw.exact_hessian(HJ, h, msa, w, q, LAM, gap)

    def grad(hh):
        return tw.field_gradient(tw.tile_sums(HJ, hh, msa, w, q, gap), hh, LAM, live)

    eps = 1e-5
    for i in range(L):
        for b in np.flatnonzero(live):
            e = np.zeros_like(h)
            e[i, b] = eps
            col = (grad(h + e) - grad(h - e))[i] / (2 * eps)
            assert np.abs(col[live] - H[i, live, b]).max() <= 1e-7 * np.abs(H[i]).max()


@pytest.mark.parametrize("q,gap,N", [(4, False, 200), (21, False, 256), (21, True, 100), (32, False, 64), (7, False, 31)])
def test_assembly_with_every_tile_sampled_is_the_exact_hessian(q, gap, N):
    """one tile, sampled (above 21 states: 64 sequences, all of them in the two waves that carry the sums): the
    rescaling has nothing to correct and H comes out exact"""
    L = 5
    msa, w, x = problem(q, N, L, seed=11, gap=gap, scale=0.5)
    Q = tw.q_template(q)
    HJ, h = tw.potentials(msa, x, q, gap)
    sums = tw.tile_sums(HJ, h, msa, w, q, gap)
    gp, dp, hp = tw.partials_from_sums(sums, Q)
    if Q > 21:
        hp = hp / 4.0                    # k_hsolve multiplies by 4: here the two waves ARE the tile
    st, Mt, Md = tw.reduce_partials(gp, dp, hp, Q)
    H = tw.assemble_hessian(st, Mt, Md, sums["cnt"].sum(axis=0), LAM)
    ref = tw.exact_hessian(HJ, h, msa, w, q, LAM, gap)
    assert np.abs(H - ref).max() <= 1e-10 * np.abs(ref).max()
    inv = tw.gauss_jordan(H)
    assert np.abs(inv - np.linalg.inv(H)).max() <= 1e-10 * np.abs(inv).max()


def test_reductions_follow_the_sampled_tiles():
    """33 tiles: the second sampled tile is the last one; scale 33 / 2; diagonal from the triangle on tiles 0 and 32"""
    rng = np.random.default_rng(5)
    S, T, Q = 3, 33, 5
    gp, dp = rng.normal(size=(S, T, Q)), rng.uniform(size=(S, T, Q))
    hp = rng.uniform(size=(S, T, Q * (Q + 1) // 2)).astype(np.float32)
    st, Mt, Md = tw.reduce_partials(gp, dp, hp, Q)
    np.testing.assert_allclose(st, gp.sum(axis=1), rtol=1e-13)
    full = tw.tri_to_full(hp.astype(np.float64), Q)
    np.testing.assert_allclose(Mt, (full[:, 0] + full[:, 32]) * 16.5, rtol=1e-13)
    idx = np.arange(Q)
    want = dp.sum(axis=1) - dp[:, 0] - dp[:, 32] + full[:, 0][:, idx, idx] + full[:, 32][:, idx, idx]
    np.testing.assert_allclose(Md, want, rtol=1e-13)
    # above 21 states every tile's diagonal comes from dp and the sampled sums count four times
    Q = 32
    gp, dp = rng.normal(size=(S, T, Q)), rng.uniform(size=(S, T, Q))
    hp = rng.uniform(size=(S, T, Q * (Q + 1) // 2)).astype(np.float32)
    st, Mt, Md = tw.reduce_partials(gp, dp, hp, Q)
    full = tw.tri_to_full(hp.astype(np.float64), Q)
    np.testing.assert_allclose(Mt, (full[:, 0] + full[:, 32]) * 66.0, rtol=1e-13)
    np.testing.assert_allclose(Md, dp.sum(axis=1), rtol=1e-13)


@pytest.mark.parametrize("q,gap", [(5, False), (21, False), (21, True)])
def test_newton_converges_and_strong_convexity_bounds_the_distance(q, gap):
    N, L = 300, 6
    msa, w, x = problem(q, N, L, seed=21, gap=gap, scale=0.4)
    HJ, h0 = tw.potentials(msa, x, q, gap)
    live = tw.live_states(q, gap)
    hstar, norm, steps = tw.solve_exact(HJ, h0, msa, w, q, LAM, gap, tol=1e-10)
    assert norm < 1e-10 and steps <= 30
    gstar = tw.field_gradient(tw.tile_sums(HJ, hstar, msa, w, q, gap), hstar, LAM, live)
    rng = np.random.default_rng(2)
    for size in (1e-6, 1e-3, 0.3):
        h = np.where(live, hstar + size * rng.normal(size=hstar.shape), 0.0)
        g = tw.field_gradient(tw.tile_sums(HJ, h, msa, w, q, gap), h, LAM, live)
        dist = np.sqrt(((h - hstar) ** 2).sum())
        assert dist <= np.sqrt(((g - gstar) ** 2).sum()) / (2 * LAM) * (1 + 1e-9)
        assert dist <= (np.sqrt((g * g).sum()) + norm) / (2 * LAM) * (1 + 1e-9)


@pytest.mark.parametrize("gap", [False, True])
def test_capped_step_moves_no_field_by_more_than_three(gap):
    q, N, L = 21, 200, 8
    msa, w, x = problem(q, N, L, seed=9, gap=gap, scale=8.0)
    HJ, h = tw.potentials(msa, x, q, gap)
    sums = tw.tile_sums(HJ, h, msa, w, q, gap)
    gp, dp, hp = tw.partials_from_sums(sums, 21)
    out = tw.predict_solve(gp, dp, hp, sums["cnt"].sum(axis=0), h, LAM, 1 if gap else 0, full=True)
    assert (out["cap"] < 1.0).any(), "the cap does not bind at this start"
    move = np.abs(out["h_new"] - h).max(axis=1)
    assert (move <= tw.CAP * (1 + 1e-12)).all()
    np.testing.assert_allclose(move[out["cap"] < 1.0], tw.CAP, rtol=1e-12)
    if gap:
        assert not (out["h_new"] - h)[:, 0].any()
