"""
CPU: tests/fixedpoint_twin.py against references that share none of its arithmetic, and the exactness preconditions of
every case tests/test_gpu_fixedpoint.py runs (DESIGN_NEXT_ROWS.md 9.17).

  * jexp at the edges of k_scale_from_max; the five digits at +-(2^38 - 1), +-128, +-32768, -1;
  * potentials_exact against the f64 oracle's single mutants (J part), within f64 rounding + L 2^-39 max|J|;
  * the integer gradient at the saturated-field points against oracle.eval, within half a unit of 1 / rscale per
    contributing sequence (the bound of test_bwd_digits_model.py);
  * every forward case: |D| < 2^38, the reference-state constant independent of the summation order, the planes a
    plane-isolating model exercises, the dominant coupling unvisited, the digit patterns of the extremes where they were
    put and visited, the plain-kernel conditions (hi + lo exact, sums below 2^24 units, half the differences in the lo plane);
  * every backward case: one sequence per cell (family a), the loud sequence alone in its cells and the rest small
    (family b), int32 headroom of every digit plane, the softmax of the saturated fields exact.
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixedpoint_twin as tw  # noqa: E402

F32, F64 = np.float32, np.float64
FWD = tw.forward_cases()


# ------------------------------------------------------------------------------------------------ scale and digits
def test_jexp_follows_the_frexp_exponent_and_clamps():
    one = lambda v: np.array([[[0.0, v], [0.0, 0.0]]], dtype=F32)
    assert tw.jexp(one(0.0)) == 0                                  # all-zero model
    assert tw.jexp(one(1.0)) == 13 and tw.jexp(one(-1.0)) == 13    # 1 = 0.5 * 2^1
    assert tw.jexp(one(np.nextafter(F32(1.0), F32(0.0)))) == 14
    assert tw.jexp(one(0.25)) == 15 and tw.jexp(one(np.nextafter(F32(0.25), F32(0.0)))) == 16
    assert tw.jexp(one(8192.0)) == 0 and tw.jexp(one(np.nextafter(F32(16384.0), F32(0.0)))) == 0
    assert tw.jexp(one(2.0 ** -120)) == 100                        # 14 + 119 = 133: clamped
    assert tw.jexp(one(2.0 ** -86)) == 99 and tw.jexp(one(2.0 ** -87)) == 100
    assert tw.jexp(one(2.0 ** 120)) == -100
    # scaled, the largest coupling lies in [2^13, 2^14) wherever the clamp is not engaged
    for v in (3e-5, 0.3, 0.5, 77.0):
        assert 2 ** 13 <= abs(v) * 2.0 ** tw.jexp(one(v)) < 2 ** 14


def test_digits_reconstruct_the_extremes():
    D = np.array([2 ** 38 - 1, -(2 ** 38 - 1), 128, -128, 32768, -32768, -1, 0, 127, -129, 2 ** 31, -(2 ** 31)] + tw.EXTREME_D)
    d = tw.digits5(D)
    assert d.dtype == np.int8 and d.shape == (D.size, 5)
    np.testing.assert_array_equal(tw.undigits5(d), D)
    assert d[0].tolist() == [-1, 0, 0, 0, 64] and d[1].tolist() == [1, 0, 0, 0, -64]
    assert d[2].tolist() == [-128, 1, 0, 0, 0] and d[3].tolist() == [-128, 0, 0, 0, 0]
    assert d[4].tolist() == [0, -128, 1, 0, 0] and d[5].tolist() == [0, -128, 0, 0, 0]
    assert d[6].tolist() == [-1, 0, 0, 0, 0]
    with pytest.raises(AssertionError):
        tw.digits5(np.array([2 ** 38]))
    rng = np.random.default_rng(0)
    D = rng.integers(-(2 ** 38) + 1, 2 ** 38, size=100000)
    np.testing.assert_array_equal(tw.undigits5(tw.digits5(D)), D)
    # the residuals' three and four digits
    for planes, lim in ((3, 8355711), (4, 2139062143)):
        R = np.concatenate([rng.integers(-lim, lim + 1, size=100000), [lim, -lim, 128, -128, 32768, -1, int(tw.QMAX[planes])]])
        dg = tw.digits_of_residual(R, planes)
        np.testing.assert_array_equal(sum(dg[:, p].astype(np.int64) << (8 * p) for p in range(planes)), R)
    assert tw.digits_of_residual(np.array([int(tw.QMAX[4])]), 4)[0].tolist() == [-128, 75, 111, 127]


def test_split_difference_places_every_pattern():
    for D in tw.EXTREME_D + [2 ** 37 - 2 ** 14 - 1, 8191, 8192, -8192, -8193]:
        A, B = tw.split_difference(D)
        assert (float(A) - float(B)) * 2.0 ** 23 == D


def test_the_twin_refuses_inputs_that_break_exactness():
    L, q = 3, 4
    j = np.zeros((3, q, q), dtype=F32)
    j[0, 1, 0], j[1, 1, 0] = 1.0, 2.0 ** -60                       # C_0(1) = 1 + 2^-60 is no f64
    with pytest.raises(AssertionError):
        tw.scaled_differences(j, L, q)
    j = np.zeros((3, q, q), dtype=F32)
    j[0, 1, 1] = F32(1.0 + 2.0 ** -11 + 2.0 ** -23)                 # 24 bits, 13 of them below the hi plane: no hi + lo pair
    with pytest.raises(AssertionError):
        tw.plain_preconditions(j, L, q)
    with pytest.raises(AssertionError):
        tw.backward_case("a", 17, False, N=22)                      # more sequences than states: cells collide


# ------------------------------------------------------------------------------------------------ against the oracle
def _x64(L, q, jij, hi=None):
    hi = np.zeros((L, q)) if hi is None else hi
    return np.concatenate([np.asarray(hi, F64).ravel(), np.asarray(jij, F64).ravel()])


@pytest.mark.parametrize("name", ["general-L17-N31-q21", "general-L33-N1-q5", "extremes-L17-N31-q21", "plain-L15-N31-q5",
                                  "planes34-L32-N31-q7", "scale-below_pow2-L47-N31-q20", "offgrid"])
def test_potentials_match_the_oracles_single_mutants(oracle64, name):
    """P[i, a] - P[i, t_i] is the J part of the oracle's single-mutant table.  Allowed: the rounding of D, documented as
    2^-39 max|J| per coupling, L of them, plus the f64 roundings of both sides (2 L 2^-53 sum_j |J|).  "offgrid" is a
    model whose couplings are NOT on a grid (only the reference-state entries are, for an exact C): D really rounds."""
    if name == "offgrid":
        L, N, q = 33, 8, 21
        rng = np.random.default_rng(77)
        jij = (0.1 * rng.standard_normal((L * (L - 1) // 2, q, q))).astype(F32)
        jij[:, :, 0] = np.rint(jij[:, :, 0] * 2 ** 20) / 2 ** 20
        jij[:, 0, :] = np.rint(jij[:, 0, :] * 2 ** 20) / 2 ** 20
        seqs = rng.integers(0, q, size=(N, L)).astype(np.int8)
    else:
        case = next(c for c in FWD if c[0] == name)
        _, _, L, N, q, _ = case
        seqs, jij = tw.forward_case(case)
    P = tw.potentials_exact(seqs, q, jij, rounded=False)
    amax = float(np.abs(jij).max())
    J4 = np.abs(tw.full_couplings(jij, L, q).astype(F64))
    for s in range(min(3, seqs.shape[0])):
        So = oracle64.single_mutants(seqs[s], q, _x64(L, q, jij))[:, :, 1]
        got = P[s] - P[s][np.arange(L), seqs[s]][:, None]
        mag = J4.max(axis=3).sum(axis=1)                              # [i, a]: sum_j max_b |J_ij(a, b)|
        bound = L * 2.0 ** -39 * amax + 4 * L * 2.0 ** -53 * (mag + mag[np.arange(L), seqs[s]][:, None])
        err = np.abs(got - So)
        assert (err <= bound).all(), (name, s, float((err / bound).max()))


@pytest.mark.parametrize("planes", [3, 4])
@pytest.mark.parametrize("family,L,gap", [("a", 2, False), ("a", 17, True), ("b", 17, False), ("b", 33, True)])
def test_integer_gradient_matches_the_oracle_at_saturated_fields(oracle64, family, L, gap, planes):
    """(V1 + V2) / rscale against the f64 oracle's pair gradient at J = 0, h = 64 on one state per site: half a unit of
    1 / rscale per contributing sequence (the rounding of R) and 2^-24 of every contributing |w_s| (the float32 product
    w_s * rscale that is rounded: with four planes R has up to 31 bits, the product 24), plus what exp(-64) leaves of the
    other states.  test_bwd_digits_model.py allows 1e-6 |g| for the second term; this is the derived, tighter form."""
    q = tw.BWD_Q
    msa, w, astar = tw.backward_case(family, L, gap, N=tw.BWD_B_N[L] if family == "b" else None)
    R = tw.residual_ints(w, planes)
    site = tw.residual_site_ints(msa, q, R, astar, gap)
    V = tw.pair_sums(msa, site, q)
    _, Vs, _, _ = tw.gradient_expected(V, w, planes, gap)
    n = tw.sequences_per_cell(msa, site, q)
    ncell = tw.pair_blocks(n) + tw.pair_blocks(n.transpose(2, 3, 0, 1))
    A = tw.pair_sums(msa, np.abs(site), q)
    mag = tw.pair_blocks(A) + tw.pair_blocks(A.transpose(2, 3, 0, 1))            # sum of the contributing |R_s|
    h = tw.saturated_fields(L, q, astar)
    if gap:
        ncell, mag = ncell[:, 1:, 1:], mag[:, 1:, 1:]
        x = _x64(L, q - 1, np.zeros((L * (L - 1) // 2, q - 1, q - 1)), h[:, 1:])
        _, _, g = oracle64.eval_gaps(msa, w.astype(F64), q, 0.01, 3.0, x)
        g = g[L * (q - 1):].reshape(Vs.shape)
    else:
        x = _x64(L, q, np.zeros((L * (L - 1) // 2, q, q)), h)
        _, _, g = oracle64.eval(msa, w.astype(F64), q, 0.01, 3.0, x)
        g = g[L * q:].reshape(Vs.shape)
    rscale, _ = tw.rscale_of(w, planes)
    got = Vs.astype(F64) / float(rscale)
    bound = (0.5 * ncell + 2.0 ** -24 * mag) / float(rscale) + 2 * q * math.exp(-64.0) * float(w.astype(F64).sum()) + 1e-15 * np.abs(g)
    assert (np.abs(got - g) <= bound).all(), float((np.abs(got - g) / np.maximum(bound, 1e-300)).max())
    assert np.abs(g).max() > 0.1 * float(w.max())                     # the point is not a trivial one


# ------------------------------------------------------------------------------------------------ forward cases
@pytest.mark.parametrize("case", FWD, ids=[c[0] for c in FWD])
def test_forward_case_meets_its_preconditions(case):
    name, kind, L, N, q, arg = case
    seqs, jij = tw.forward_case(case)
    assert seqs.shape == (N, L) and jij.shape == (L * (L - 1) // 2, q, q) and jij.dtype == F32
    out, dig, visited = tw.potentials_exact(seqs, q, jij, with_digits=True)      # asserts |D| < 2^38 and the exact C
    assert out.dtype == F32 and np.isfinite(out).all()
    D = tw.undigits5(dig)
    used = tw.planes_exercised(dig, visited)
    je = tw.jexp(jij)
    if kind == "general":
        assert (np.rint(jij.astype(F64) * 2 ** 20) == jij.astype(F64) * 2 ** 20).all()
        assert tw.order_independent(tw.full_couplings(jij, L, q)[:, :, :, 0].astype(F64), axis=1)
        assert set(used) >= {2, 3, 4}
    elif kind == "plain":
        frac, units = tw.plain_preconditions(jij, L, q)
        assert frac >= 0.5 and units < 2 ** 24
        assert np.abs(jij).max() < 1.0
    elif kind == "planes":
        assert je == 0 and used == (arg, arg + 1)
        (k, a, b), forbid = tw._dominant_slot(L, q)
        assert jij[k, a, b] == tw.DOMINANT and not visited[0, 1, a, b] and not visited[1, 0, b, a]
        for site, state in forbid:
            assert not (seqs[:, site] == state).any()
        # both planes of the pair are needed: neither alone reproduces a visited difference
        vb = visited.copy()
        vb[:, :, :, 0] = False                                          # (the reference state has D = 0 by definition)
        assert (dig[..., arg][vb] != 0).mean() > 0.9 and (dig[..., arg + 1][vb] != 0).mean() > 0.9
    elif kind == "extremes":
        assert je == 0
        _, want = tw.model_extremes(L, q, sum(ord(c) * (n + 1) for n, c in enumerate(name)) % (2 ** 31))
        iu, ju = np.triu_indices(L, 1)
        for (k, a, b), Dw in want.items():
            assert D[iu[k], ju[k], a, b] == Dw and visited[iu[k], ju[k], a, b], (k, a, b)
        assert D[L - 2, L - 1, q - 1, q - 1] == 2 ** 38 - 2 ** 14      # last site pair, last state: the largest |D|
        assert D[L - 1, L - 2, q - 1, q - 1] == 2 ** 38 - 2 ** 14      # and as the last site's own row
        v = dig[visited]
        assert (v == -128).any() and (v == 127).any() and (D[visited] < 0).any()
        assert (v[:, 4] != 0).any() and (v[:, 0] != 0).any()
    else:
        want_je = {"pow2": 15, "below_pow2": 16, "tiny": 100, "zero": 0, "single": 15}[arg]
        assert je == want_je
        amax = float(np.abs(jij).max())
        assert amax == {"pow2": 0.25, "below_pow2": float(np.nextafter(F32(0.25), F32(0))), "tiny": 2.0 ** -120,
                        "zero": 0.0, "single": float(F32(0.3))}[arg]
        if arg == "zero":
            assert not out.any()
        if arg == "single":
            assert np.count_nonzero(jij) == 1 and out.any()
        if arg == "tiny":
            nz = np.abs(out[out != 0])
            assert nz.size and nz.min() >= 2.0 ** -126                  # no float32 subnormal in the expected output


# ------------------------------------------------------------------------------------------------ backward cases
def _headroom_ok(msa, site, q, planes):
    return tw.headroom(msa, site, q, planes) < 2 ** 31


@pytest.mark.parametrize("planes", [3, 4])
@pytest.mark.parametrize("gap", [False, True])
@pytest.mark.parametrize("L,q", [(L, tw.BWD_Q) for L in tw.BWD_L] + [(17, q) for q in tw.OTHER_Q])
def test_family_a_has_one_sequence_per_cell(L, q, gap, planes):
    msa, w, astar = tw.backward_case("a", L, gap, N=q, q=q)
    assert msa.shape == (q, L) and w.max() == F32(tw.WMAX) == w[0]
    if q >= 13:
        assert w.min() <= 2.0 ** -11 * tw.WMAX and w.min() >= 2.0 ** -13 * tw.WMAX   # the weights span 2^0 .. 2^-12
    R = tw.residual_ints(w, planes)
    dg = tw.digits_of_residual(R, planes)
    assert all((dg[:, p] != 0).sum() >= q // 2 - 1 for p in range(planes))              # every plane carries digits
    for site in (tw.marginal_site_ints(msa, q, R), tw.residual_site_ints(msa, q, R, astar, gap)):
        assert tw.sequences_per_cell(msa, site, q).max() == 1
        assert _headroom_ok(msa, site, q, planes)
        V = tw.pair_sums(msa, site, q)
        assert np.abs(V).max() == R.max()                                             # the top plane is asserted too


@pytest.mark.parametrize("planes", [3, 4])
@pytest.mark.parametrize("gap", [False, True])
@pytest.mark.parametrize("L", tw.BWD_L)
def test_family_b_has_one_loud_sequence_and_small_cells(L, gap, planes):
    q, N = tw.BWD_Q, tw.BWD_B_N[L]
    msa, w, astar = tw.backward_case("b", L, gap, N=N)
    assert N in (130, 257, 700) and msa.shape == (N, L)
    assert (msa[0] == q - 1).all() and not (msa[1:] == q - 1).any()
    assert w[0] == F32(tw.WMAX) and w[1:].max() <= 2.0 ** -9 * tw.WMAX
    R = tw.residual_ints(w, planes)
    site = tw.marginal_site_ints(msa, q, R)
    V = tw.pair_sums(msa, site, q)
    loud = np.zeros(V.shape, dtype=bool)
    loud[:, q - 1, :, q - 1] = True
    assert (V[loud] == R[0]).all() and tw.sequences_per_cell(msa, site, q)[loud].max() == 1
    assert _headroom_ok(msa, site, q, planes)
    if planes == 3:
        assert np.abs(V[~loud]).max() < 2 ** 22         # the integer is recovered from the output by rint(out / scale)
    assert (np.abs(tw.pair_blocks(V)) < 2 ** 22).mean() > (0.9 if planes == 3 else 0.05)
    rsite = tw.residual_site_ints(msa, q, R, astar, gap)
    assert _headroom_ok(msa, rsite, q, planes)
    many = tw.sequences_per_cell(msa, rsite, q)
    assert many.max() > 1                                # many sequences per cell: the sums are real sums


def test_headroom_case_sits_at_the_int32_limit():
    """All sequences equal, all weights 1: R = QMAX.  With four planes its digits are (-128, 75, 111, 127): plane 0 of a
    K range of n sequences holds (-128)(-128) n, plane 3 holds -128 * 127 n.  n = 130 816 (1022 steps of 128, the largest
    range of one split) stays below 2^31; 131 328 sequences in ONE range would not, in the two ranges pick_ksplit must
    form they do."""
    w = np.ones(8, dtype=F32)
    for planes in (3, 4):
        R = tw.residual_ints(w, planes)
        assert (R == int(tw.QMAX[planes])).all()
    dg = tw.digits_of_residual(tw.residual_ints(w, 4)[:1], 4)[0].astype(np.int64)
    assert dg.tolist() == [-128, 75, 111, 127]
    n1, n2 = tw.HEADROOM_N
    assert n1 % 256 == 0 and n1 // 128 == 1022 and (n2 + 255) // 256 * 256 // 128 == 1026
    assert max(abs(128 * int(d) * n1) for d in dg) < 2 ** 31
    assert abs(128 * int(dg[0]) * n2) >= 2 ** 31
    per_range = (1026 + 1) // 2 * 128
    assert max(abs(128 * int(d) * per_range) for d in dg) < 2 ** 31
    # the twin's expected frequency: the one occupied cell of every pair holds float32(scale * float32(-128 N R))
    for n in (n1, n2):
        wn = np.ones(n, dtype=F32)
        assert tw.neff_of(wn) == float(n)
        V = np.array([[[[n * int(tw.QMAX[4])]]]])
        f = F32(tw.marginal_scale(wn, 4, False)) * tw.combine(V, unit=n)
        assert abs(float(f.ravel()[0]) - 1.0) < 2e-7
