"""
GPU: the kernels that turn gradients into steps (plm_kernels.hip, "L-BFGS streaming kernels" and "vector-free L-BFGS":
k_dots, k_dots_final, k_lincomb, k_multidot<1..4>, k_multiaxpy with and without the fused trial point, k_sy_multidot,
k_dots_final2) and the H0 diagonal (k_precond_j / k_precond_h) against tests/lbfgs_vector_twin.py, through the diagnostic
entry points plm_lbfgs_* / plm_ctx_precond_diagonal.  The entries prefill the dot scratch and every output with NaN bytes: a
partial sum or an output that a kernel fails to write comes back as NaN, and NaN anywhere fails.  No entry is masked out.

Inputs: one seeded normal float32 vector per slot and role, all different -- a swapped position changes a Gram entry by
O(sqrt n), not by rounding; dinv uniform in [0.5, 2] with a run of exact zeros (the structural zeros of the real diagonal);
slot `end` of S / Y holds NaN on entry (the pass must overwrite it, never read it).

Tolerances, all derived:
  pair        bit-exact (one IEEE subtraction)
  dots        |gpu - twin| <= n 2^-53 sum |a_i b_i|: n f64 additions of exact products (one missing float4 is ~1e6 times
              larger at the biggest n)
  direction   per entry |gpu - twin| <= (nb + 2) 2^-24 (sum_k |c_k b_k| (. dinv)): one f32 rounding per fused multiply-add,
              the dinv product and the f32 rounding of the coefficients
  lincomb     2 roundings with b, 1 without; trial point: 1 rounding on the GPU's own float32 direction
  identities  dir of the plain launch == dir of the fused launch; trial == plm_launch_lincomb(1, xacc, stp0, dir), bit for
              bit (the line search skips its first lincomb on that assumption)
  H0          rtol 8 x 2^-24 (at most eight f32 roundings in the expression), exact zero where the twin says structural zero

Shapes.  The dot grids sweep 1024 x 256 float4 = 1 048 576 floats per step, multiaxpy / lincomb 2 097 152:
  n = 4 (one lane works, 1023 blocks must still write zeros), 1028 (crosses a block), 1 048 576 / 1 048 580 (second
  grid-stride step for one float4), 2 097 156, 2 621 444;  nh in {0, 4, a multiple of 4 that is no multiple of 1024, n};
  (m, nst, end): (1,1,0) no old vector (the bp = g stand-in), (6,1,0) first iteration, (6,3,2), (6,6,0/2/5) exactly one
  chunk of 10 with the pair first / middle / last, (7,7,3) a second chunk of 2, (10,10,9), (20,20,7) four chunks, nb = 42,
  wb bit 41.  m = 20 runs up to n = 1 048 580, the two largest n with m <= 7.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lbfgs_vector_twin as tw  # noqa: E402
from test_host_layer import _two_loop_dense  # noqa: E402
from test_lbfgs_vector_twin_host import check_error_paths, coefficients, ring_steps  # noqa: E402

from evcouplings_amd._lib import PlmError  # noqa: E402
from evcouplings_amd.synthetic import synthetic_msa  # noqa: E402

pytestmark = pytest.mark.gpu
PLM_EINVAL = -1
U53, U24 = 2.0 ** -53, 2.0 ** -24
F32 = np.float32
N_GRID = 1048576


@pytest.fixture(scope="module")
def plm():
    from evcouplings_amd import plm as _plm
    assert _plm.device_count() >= 1, "no gfx950 device: the HIP path has no fallback"
    return _plm


def normals(rng, *shape):
    return rng.standard_normal(shape, dtype=F32)


def make_dinv(rng, n):
    d = rng.uniform(0.5, 2.0, size=n).astype(F32)
    z0 = n // 3
    d[z0:z0 + max(1, min(n // 8, 5000))] = 0.0
    return d


def check_dots(gpu, ref, mag, n, what):
    gpu, ref, mag = np.asarray(gpu).ravel(), np.asarray(ref).ravel(), np.asarray(mag).ravel()
    assert gpu.shape == ref.shape
    assert np.isfinite(gpu).all(), "%s: entries %s are not finite (never written?)" % (what, np.flatnonzero(~np.isfinite(gpu)))
    bad = np.flatnonzero(~(np.abs(gpu - ref) <= n * U53 * mag))
    assert bad.size == 0, "%s: entries %s: gpu %s twin %s bound %s" % (what, bad, gpu[bad], ref[bad], n * U53 * mag[bad])


def check_vector(gpu, ref, mag, units, what):
    assert gpu.dtype == F32 and np.isfinite(gpu).all(), "%s: non-finite entries" % what
    err, bound = np.abs(gpu.astype(np.float64) - ref), units * U24 * mag
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, "%s: %d entries beyond the bound, first %s: gpu %s twin %s bound %s" % (
        what, bad.size, bad[:4], gpu[bad[:4]], ref[bad[:4]], bound[bad[:4]])


# ---- the Gram pass (k_sy_multidot + k_dots_final2) -------------------------------------------------------------------
RINGS = [(1, 1, 0), (6, 1, 0), (6, 3, 2), (6, 6, 0), (6, 6, 2), (6, 6, 5), (7, 7, 3), (10, 10, 9), (20, 20, 7)]
GRAM_CASES = sorted(set(
    [(1028, (0, 4, 516, 1028)[k % 4]) + r for k, r in enumerate(RINGS)] +
    [(1028, nh, 6, 3, 2) for nh in (0, 4, 516, 1028)] +
    [(4, 0, 1, 1, 0), (4, 4, 6, 6, 2), (4, 0, 7, 7, 3), (4, 4, 20, 20, 7)] +
    [(N_GRID, N_GRID, 6, 6, 2), (N_GRID, 4, 20, 20, 7)] +
    [(N_GRID + 4, N_GRID + 4, 7, 7, 3), (N_GRID + 4, 1000, 20, 20, 7), (N_GRID + 4, 0, 6, 1, 0)] +
    [(2 * N_GRID + 4, N_GRID + 4, 6, 3, 2)] +
    [(2621444, 2621444, 7, 7, 3), (2621444, 4, 1, 1, 0)]))


@pytest.mark.parametrize("with_dinv", [False, True], ids=["plain", "metric"])
@pytest.mark.parametrize("n,nh,m,nst,end", GRAM_CASES, ids=lambda v: str(v))
def test_gram_pass(plm, n, nh, m, nst, end, with_dinv):
    rng = np.random.default_rng([n, nh, m, nst, end])
    S, Y = np.full((m, n), np.nan, F32), np.full((m, n), np.nan, F32)      # slots >= nst are in no basis
    S[:nst], Y[:nst] = normals(rng, nst, n), normals(rng, nst, n)
    S[end] = Y[end] = np.nan
    x, xp, g, gp, direction = normals(rng, 5, n)
    dinv = make_dinv(rng, n) if with_dinv else None
    s_gpu, y_gpu, md_gpu, ex_gpu = plm.lbfgs_gram(S, Y, x, xp, g, gp, direction, end, nst, nh, dinv)
    s_new, y_new, md, md_abs, ex, ex_abs = tw.gram(S, Y, x, xp, g, gp, direction, m, end, nst, nh, dinv)
    np.testing.assert_array_equal(s_gpu, s_new)
    np.testing.assert_array_equal(y_gpu, y_new)
    check_dots(md_gpu, md, md_abs, n, "md")
    check_dots(ex_gpu, ex, ex_abs, n, "ex")
    if with_dinv and n <= 1028:      # the metric is no no-op on these inputs: exactly the flagged entries differ from the plain ones
        plain = tw.gram(S, Y, x, xp, g, gp, direction, m, end, nst, nh, None)[2]
        flagged = np.array([e[2] for e in tw.gram_layout(m, end, nst)[0]])
        assert np.all(plain[flagged] != md[flagged]) and np.all(plain[~flagged] == md[~flagged])


# ---- plm_launch_multidot (k_multidot<NQ> + k_dots_final) ---------------------------------------------------------------
def wb_patterns(nb):
    return [0, (1 << nb) - 1, 0x2AAAAAAAAAA & ((1 << 42) - 1), 1 << 13, 1 << 14, 1 << 41]


@pytest.mark.parametrize("nb", [1, 2, 14, 15, 28, 29, 42])
@pytest.mark.parametrize("nq", [1, 2, 3, 4])
def test_multidot_flags_and_chunk_boundaries(plm, nq, nb):
    """MD_CHUNK = 14 basis vectors per blockIdx.y: 14 / 15, 28 / 29 and 42 are its boundaries; every wq x wb pattern"""
    n = 1028
    rng = np.random.default_rng([nq, nb])
    V = normals(rng, nq + nb, n)
    dinv = make_dinv(rng, n)
    qi, bi = np.arange(nq), nq + np.arange(nb)
    for wq in (0, 1, 0b1010, 0b1111):
        for wb in wb_patterns(nb):
            out = plm.lbfgs_multidot(V, qi, bi, dinv, wq, wb)
            ref, mag = tw.multidot(V[qi], V[bi], dinv, wq, wb)
            check_dots(out, ref, mag, n, "wq=%x wb=%x" % (wq, wb))
    out = plm.lbfgs_multidot(V, qi, bi, None, 0b1111, (1 << 42) - 1)         # no dinv: the flags mean nothing
    ref, mag = tw.multidot(V[qi], V[bi])
    check_dots(out, ref, mag, n, "no dinv")


@pytest.mark.parametrize("n", [4, N_GRID, N_GRID + 4])
@pytest.mark.parametrize("nq,nb,wq,wb", [(4, 42, 0b1010, 0x2AAAAAAAAAA), (3, 15, 0b110, 1 << 14), (1, 29, 1, 1 << 28)])
def test_multidot_lengths(plm, n, nq, nb, wq, wb):
    rng = np.random.default_rng([n, nq, nb])
    V = normals(rng, nq + nb, n)
    dinv = make_dinv(rng, n)
    qi, bi = np.arange(nq), nq + np.arange(nb)
    out = plm.lbfgs_multidot(V, qi, bi, dinv, wq, wb)
    ref, mag = tw.multidot(V[qi], V[bi], dinv, wq, wb)
    check_dots(out, ref, mag, n, "multidot")


@pytest.mark.parametrize("n", [4, 1028, N_GRID + 4, 2621444])
@pytest.mark.parametrize("with_dinv", [False, True], ids=["plain", "metric"])
def test_multidot_same_vector_on_both_sides(plm, n, with_dinv):
    """the fit's (g; g, g) call with wq = 1, wb = 1: gDg and gg from one vector"""
    rng = np.random.default_rng([n, 11])
    V = normals(rng, 1, n)
    dinv = make_dinv(rng, n) if with_dinv else None
    out = plm.lbfgs_multidot(V, [0], [0, 0], dinv, 1, 1)
    ref, mag = tw.multidot([V[0]], [V[0], V[0]], dinv, 1, 1)
    check_dots(out, ref, mag, n, "gDg, gg")
    assert (out[0, 0] != out[0, 1]) == with_dinv


# ---- plm_launch_dots (k_dots<NP> + k_dots_final), plm_launch_lincomb -----------------------------------------------------
NS = [4, 1028, N_GRID, N_GRID + 4, 2 * N_GRID + 4, 2621444]


@pytest.mark.parametrize("n", NS)
def test_dots_one_to_four_pairs_and_the_prefix(plm, n):
    """the prefix length is how the fit's norm_dots uses the launcher: x.x over the fields"""
    rng = np.random.default_rng([n, 5])
    V = normals(rng, 5, n)
    pairs = [(0, 1), (2, 3), (4, 0), (1, 1)]
    prefixes = sorted({n, 0, 4, max(0, n - 8) if n <= 1028 else N_GRID + 4 if n > N_GRID + 4 else 1000})
    full = {p: tw.dot(V[p[0]], V[p[1]]) for p in pairs}
    for npairs in (1, 2, 3, 4):
        ai, bi = [p[0] for p in pairs[:npairs]], [p[1] for p in pairs[:npairs]]
        for k in prefixes:
            out = plm.lbfgs_dots(V, ai, bi, k)
            ref = [full[p] if k == n else tw.dot(V[p[0]], V[p[1]], n=k) for p in pairs[:npairs]]
            check_dots(out, [r[0] for r in ref], [r[1] for r in ref], n, "%d pairs over %d" % (npairs, k))


@pytest.mark.parametrize("n", NS)
def test_lincomb_with_and_without_b(plm, n):
    rng = np.random.default_rng([n, 6])
    a, b = normals(rng, 2, n)
    ca, cb = 0.7310586, -1.3e-3
    ref, mag = tw.lincomb(ca, a, cb, b)
    check_vector(plm.lbfgs_lincomb(ca, a, cb, b), ref, mag, 2, "ca a + cb b")
    ref, mag = tw.lincomb(ca, a)
    check_vector(plm.lbfgs_lincomb(ca, a), ref, mag, 1, "ca a")
    np.testing.assert_array_equal(plm.lbfgs_lincomb(1.0, a, 0.0, b), a)


# ---- the direction (k_multiaxpy, plain and with the fused trial point) -------------------------------------------------
def spd_pairs(rng, m, n):
    """S normal, Y = S H with H = diag(h) + u u^T / n (SPD, applied without forming it), all float32"""
    S = normals(rng, m, n)
    h = rng.uniform(0.5, 2.0, size=n)
    u = rng.standard_normal(n)
    Y = (S.astype(np.float64) * h + np.outer(S.astype(np.float64) @ u, u) / n).astype(F32)
    return S, Y


DIRECTION_CASES = ([(1028,) + r for r in [(6, 0, 0), (6, 3, 3), (6, 6, 2), (6, 5, 2), (20, 20, 7)]] +
                   [(4, 6, 6, 2), (4, 6, 0, 0), (N_GRID, 6, 3, 3), (N_GRID + 4, 20, 20, 7), (2 * N_GRID + 4, 6, 6, 2),
                    (2621444, 6, 5, 2), (2621444, 6, 0, 0)])


def check_direction(plm, S, Y, g, cs, cy, cg, m, stored, end, dinv, rng):
    n = g.size
    xacc, stp0 = normals(rng, n), 0.37
    d_plain = plm.lbfgs_direction(S, Y, g, cs, cy, cg, stored, end, dinv)
    d_fused, trial = plm.lbfgs_direction(S, Y, g, cs, cy, cg, stored, end, dinv, xacc=xacc, stp0=stp0)
    np.testing.assert_array_equal(d_fused, d_plain)
    np.testing.assert_array_equal(trial, plm.lbfgs_lincomb(1.0, xacc, stp0, d_plain))
    nb = 2 * stored + 1
    ref, mag = tw.direction(S, Y, g, cs, cy, cg, m, stored, end, dinv)
    check_vector(d_plain, ref, mag, nb + 2, "direction")
    t_ref, t_mag = tw.trial_point(xacc, stp0, d_plain)
    check_vector(trial, t_ref, t_mag, 1, "trial point")
    live = tw.live_slots(m, stored, end)
    dense = _two_loop_dense(g.astype(np.float64), [(S[j].astype(np.float64), Y[j].astype(np.float64)) for j in reversed(live)],
                            None if dinv is None else dinv.astype(np.float64))
    check_vector(d_plain, dense, mag, nb + 2, "direction against the dense two-loop recursion")
    return d_plain


@pytest.mark.parametrize("with_dinv", [False, True], ids=["plain", "metric"])
@pytest.mark.parametrize("n,m,stored,end", DIRECTION_CASES, ids=lambda v: str(v))
def test_direction_and_fused_trial_point(plm, n, m, stored, end, with_dinv):
    rng = np.random.default_rng([n, m, stored, end])
    S, Y = spd_pairs(rng, m, n)
    g = normals(rng, n)
    dinv = make_dinv(rng, n) if with_dinv else None
    live = tw.live_slots(m, stored, end)
    for j in range(m):
        if j not in live:
            S[j] = Y[j] = np.nan                          # dead slots are never read
    SY, YDY, Sg, YDg, gDg = tw.gram_dense(S, Y, g, m, live, dinv, exact=n <= 1028)
    cs, cy, cg, dg = coefficients(m, stored, end, SY, YDY, Sg, YDg, gDg)
    assert dg < 0 and np.isfinite(cs).all() and np.isfinite(cy).all()
    check_direction(plm, S, Y, g, cs, cy, cg, m, stored, end, dinv, rng)


# ---- chained: Gram pass on the GPU -> host indexing -> coefficients -> direction on the GPU --------------------------
def host_gram_from_layout(md, m, end, nst):
    """SY / YDY / Sg / YDg / gDg / gg from md as plm_ctx_optimize fills them after an accepted step, looked up by MEANING in
    the twin's layout"""
    layout = tw.gram_layout(m, end, nst)[0]
    at = lambda qv, bv, metric: md[layout.index((qv, bv, metric, False))]
    e = end
    SY, YDY = np.full((m, m), np.nan), np.full((m, m), np.nan)
    Sg, YDg = np.full(m, np.nan), np.full(m, np.nan)
    for j in range(nst):
        SY[e, j] = at(("S", e), ("Y", j), False)
        SY[j, e] = at(("Y", e), ("S", j), False)
        YDY[e, j] = YDY[j, e] = at(("Y", e), ("Y", j), True)
        Sg[j] = at("g", ("S", j), False)
        YDg[j] = at("g", ("Y", j), True)
    return SY, YDY, Sg, YDg, at("g", "g", True), at("g", "g", False)


@pytest.mark.parametrize("with_dinv", [False, True], ids=["plain", "metric"])
@pytest.mark.parametrize("m,stored,end", [(6, 6, 2), (6, 5, 2), (6, 3, 3)])
def test_chain_gram_coefficients_direction(plm, m, stored, end, with_dinv):
    """the ring is filled by GPU passes the way the fit fills it ((6, 5, 2): the last pair is skipped on a full ring)"""
    n, nh = 1028, 84
    rng = np.random.default_rng([m, stored, end, 9])
    A = rng.normal(size=(n, n))
    H = A @ A.T / n + np.eye(n)
    dinv = make_dinv(rng, n) if with_dinv else None
    S, Y = np.full((m, n), np.nan, F32), np.full((m, n), np.nan, F32)
    SY, YDY = np.full((m, m), np.nan), np.full((m, m), np.nan)
    Sg, YDg = np.full(m, np.nan), np.full(m, np.nan)
    accepted, skipped = ring_steps(m, stored, end)
    skip_last, steps = skipped > 0, accepted + skipped
    cur_stored = cur_end = 0
    for t in range(steps):
        xp = normals(rng, n)
        x = xp + normals(rng, n)
        gp = normals(rng, n)
        g = gp + (H @ (x.astype(np.float64) - xp)).astype(F32)
        nst = min(m, cur_stored + 1)
        S[cur_end] = Y[cur_end] = np.nan
        s_new, y_new, md, ex = plm.lbfgs_gram(S, Y, x, xp, g, gp, normals(rng, n), cur_end, nst, nh, dinv)
        assert np.isfinite(md).all() and np.isfinite(ex).all()
        S[cur_end], Y[cur_end] = s_new, y_new
        rSY, rYDY, rSg, rYDg, gDg, gg = host_gram_from_layout(md, m, cur_end, nst)
        for a, b in zip(tw.gram_to_host(md, m, cur_end, nst), (rSY, rYDY, rSg, rYDg, gDg, gg)):
            np.testing.assert_array_equal(a, b)           # the twin's indexing is the one written out above
        new = ~np.isnan(rSY)
        SY[new], YDY[new] = rSY[new], rYDY[new]
        Sg[:nst], YDg[:nst] = rSg[:nst], rYDg[:nst]
        if skip_last and t == steps - 1:
            cur_stored = min(cur_stored, m - 1)
        else:
            cur_stored, cur_end = nst, (cur_end + 1) % m
    assert (cur_stored, cur_end) == (stored, end)
    cs, cy, cg, dg = coefficients(m, stored, end, SY, YDY, Sg, YDg, gDg)
    assert dg < 0
    check_direction(plm, S, Y, g, cs, cy, cg, m, stored, end, dinv, rng)


# ---- the H0 diagonal (k_precond_j / k_precond_h through the native -> canonical path) ----------------------------------
@pytest.mark.parametrize("L,q,gaps", [(2, 21, False), (17, 21, False), (33, 21, True), (33, 20, False), (17, 5, False),
                                      (17, 4, False), (20, 7, False), (20, 26, True)])
def test_precond_diagonal(plm, L, q, gaps):
    N = 203
    msa, _ = synthetic_msa(N, L, seed=L * 100 + q, q=q)
    rng = np.random.default_rng([L, q])
    if gaps:
        msa[rng.random(msa.shape) < 0.1] = 0
    w = rng.choice(np.array([0.25, 0.5, 1.0], F32), size=N)      # dyadic: N_eff is exact in float32 and float64 alike
    lam_h = 0.01
    with plm.PlmContext(msa, q=q, lambda_h=lam_h, ignore_gaps=gaps) as ctx:
        ctx.set_weights(w)
        with pytest.raises(PlmError) as e:                # no frequencies yet
            ctx.precond_diagonal()
        assert e.value.code == PLM_EINVAL
        fi, _ = ctx.marginals(pairs=False)
        if gaps:
            fi = np.concatenate([np.zeros((L, 1), F32), fi], axis=1)
        d = ctx.precond_diagonal()
        lam_j = ctx.lambda_j
    ref, zero = tw.precond_diagonal(fi, float(w.astype(np.float64).sum()), lam_h, lam_j, gaps)
    assert d.shape == ref.shape and np.isfinite(d).all()
    assert np.all(d[zero] == 0.0)
    assert np.all(ref[~zero] > 0)
    rel = np.abs(d[~zero].astype(np.float64) - ref[~zero]) / ref[~zero]
    assert rel.max() <= 8 * U24, (rel.max() / U24, int(np.argmax(rel)))
    assert np.unique(d[~zero]).size > 0.5 * L * q         # distinct values: a permuted entry would not go unnoticed


def test_precond_diagonal_needs_a_single_shard(plm):
    msa, _ = synthetic_msa(64, 17, seed=3)
    with plm.PlmContext(msa, q=21, n_shards=2, shard=0) as sharded:
        with pytest.raises(PlmError) as e:
            sharded.precond_diagonal()
        assert e.value.code == PLM_EINVAL


# ---- invalid arguments ---------------------------------------------------------------------------------------------------
def test_invalid_arguments_launch_nothing(plm):
    check_error_paths()
