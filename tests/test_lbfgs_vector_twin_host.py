"""
CPU: tests/lbfgs_vector_twin.py against the textbook two-loop recursion -- the twin is what tests/test_gpu_lbfgs_vectors.py
holds the L-BFGS vector kernels to, so its layout of the Gram pass is tied here to the meaning plm_ctx_optimize gives it.

A ring of m slots is filled the way the fit fills it: one Gram pass of the twin per accepted step, whose md vector goes into
the host's SY / YDY / Sg / YDg by the indexing plm_ctx_optimize applies (gram_to_host); a last pass may be a skipped pair
(full ring, slot `end` dead).  The library's own plm_lbfgs_coefficients (host code, no device) then turns that Gram matrix
into coefficients, the twin's direction applies them, and the result must be the dense two-loop recursion on the same
vectors.  A wrong position, a wrong flag or a wrong slot anywhere in gram_layout changes a Gram entry by O(1) and fails this.

The diagonal H0 takes its entries from {0, 1/2, 1, 2}: the twin rounds dinv * query to float32 as the kernel does, and with
powers of two that product is exact, so the dense recursion in float64 sees the same metric.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lbfgs_vector_twin as tw  # noqa: E402
from test_host_layer import _two_loop_dense  # noqa: E402

N_VEC, NH = 40, 8


def coefficients(m, stored, end, SY, YDY, Sg, YDg, gDg):
    from evcouplings_amd import _lib
    lib = _lib.load()
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (SY, YDY, Sg, YDg)]
    cs, cy = np.full(m, 7.0), np.full(m, 7.0)
    cg, dg = C.c_double(0), C.c_double(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.plm_lbfgs_coefficients(m, stored, end, *[p(a) for a in arrs], float(gDg), p(cs), p(cy), C.byref(cg), C.byref(dg))
    return cs, cy, cg.value, dg.value


def ring_steps(m, stored, end):
    """(accepted steps, then skipped ones) after which a ring of m slots stands at (stored, end): `stored` steps while it
    fills (end == stored), m + end on a full ring, and with stored == m - 1 on a full ring one more pass whose pair is
    dropped -- slot `end` dead, wherever the ring stands"""
    if stored < m and end == stored:
        return stored, 0
    assert stored >= m - 1
    return m + end, m - stored


def fill_ring(m, stored, end, dinv, seed):
    """Run the twin's Gram pass once per step until the ring stands at (stored, end); returns the vectors and the host's
    Gram pieces as the fit would hold them.  stored == m - 1 with the ring full: the last pass is a skipped pair."""
    rng = np.random.default_rng(seed)
    n = N_VEC
    A = rng.normal(size=(n, n))
    H = A @ A.T + n * np.eye(n)                           # SPD: s.y > 0 for every pair
    S, Y = np.full((m, n), np.nan, np.float32), np.full((m, n), np.nan, np.float32)
    SY, YDY = np.full((m, m), np.nan), np.full((m, m), np.nan)
    Sg, YDg = np.full(m, np.nan), np.full(m, np.nan)
    accepted, skipped = ring_steps(m, stored, end)
    skip_last, steps = skipped > 0, accepted + skipped
    cur_stored, cur_end = 0, 0
    gDg = g = None
    for t in range(steps):
        xp = rng.normal(size=n).astype(np.float32)
        x = (xp + rng.normal(size=n).astype(np.float32)).astype(np.float32)
        gp = rng.normal(size=n).astype(np.float32)
        g = (gp + (H @ (x.astype(np.float64) - xp)).astype(np.float32)).astype(np.float32)
        direction = rng.normal(size=n).astype(np.float32)
        nst = min(m, cur_stored + 1)
        S[cur_end] = Y[cur_end] = np.nan                  # the slot's old contents must never be read
        s_new, y_new, md, _, ex, _ = tw.gram(S, Y, x, xp, g, gp, direction, m, cur_end, nst, NH, dinv)
        assert np.isfinite(md).all() and np.isfinite(ex).all()
        S[cur_end], Y[cur_end] = s_new, y_new
        rSY, rYDY, rSg, rYDg, gDg, gg = tw.gram_to_host(md, m, cur_end, nst)
        new = ~np.isnan(rSY)
        SY[new], YDY[new] = rSY[new], rYDY[new]
        Sg[:nst], YDg[:nst] = rSg[:nst], rYDg[:nst]
        # what else the fit reads from the pass
        assert gg == tw.dot(g, g)[0]
        assert md[3 * (2 * nst + 2)] == tw.dot(s_new, s_new, n=NH)[0]
        assert ex[0] == tw.dot(g, direction)[0] and ex[1] == tw.dot(x, x)[0] and ex[2] == tw.dot(x, x, n=NH)[0]
        if skip_last and t == steps - 1:
            cur_stored = min(cur_stored, m - 1)           # the pair is dropped: slot `end` is dead, the ring stays
        else:
            cur_stored, cur_end = nst, (cur_end + 1) % m
    assert (cur_stored, cur_end) == (stored, end), (cur_stored, cur_end)
    return S, Y, g, SY, YDY, Sg, YDg, gDg


@pytest.mark.parametrize("precond", [False, True], ids=["plain", "diagonal"])
@pytest.mark.parametrize("m,stored,end", [(6, 6, 2), (6, 5, 2), (4, 3, 1), (20, 20, 7)])
def test_twin_gram_and_direction_are_the_two_loop_recursion(m, stored, end, precond):
    rng = np.random.default_rng(7)
    dinv = rng.choice(np.array([0.0, 0.5, 1.0, 2.0], np.float32), size=N_VEC, p=[0.1, 0.3, 0.3, 0.3]) if precond else None
    S, Y, g, SY, YDY, Sg, YDg, gDg = fill_ring(m, stored, end, dinv, seed=m * 100 + stored * 10 + end)
    live = tw.live_slots(m, stored, end)
    # the Gram matrix the passes left is the Gram matrix of the vectors, entry by entry
    dSY, dYDY, dSg, dYDg, dgDg = tw.gram_dense(S, Y, g, m, live, dinv)
    for i in live:
        for j in live:
            assert SY[i, j] == dSY[i, j] and YDY[i, j] == dYDY[i, j], (i, j)
        assert Sg[i] == dSg[i] and YDg[i] == dYDg[i]
    assert gDg == dgDg
    cs, cy, cg, dg = coefficients(m, stored, end, SY, YDY, Sg, YDg, gDg)
    p, mag = tw.direction(S, Y, g, cs, cy, cg, m, stored, end, dinv)
    d64 = None if dinv is None else dinv.astype(np.float64)
    ref = _two_loop_dense(g.astype(np.float64), [(S[j].astype(np.float64), Y[j].astype(np.float64)) for j in reversed(live)], d64)
    np.testing.assert_allclose(p, ref, rtol=1e-9, atol=1e-12)
    assert dg == pytest.approx(g.astype(np.float64).dot(ref), rel=1e-9)
    assert dg < 0
    assert np.all(mag >= np.abs(p) * (1 - 1e-12))


def test_gram_layout_positions_and_flags():
    """(m, nst, end) = (6, 3, 1): nb = 8; the pair is S[1] / Y[1]; flags on Y0..Y2 and the first g x queries y_new, g"""
    md, ex = tw.gram_layout(6, 1, 3)
    assert len(md) == 3 * 8 + 1 and len(ex) == 3
    assert md[0] == (("S", 1), ("S", 0), False, False)
    assert md[1 * 8 + 3] == (("Y", 1), ("Y", 0), True, False)
    assert md[0 * 8 + 4] == (("S", 1), ("Y", 1), False, False)          # s.y of the new pair: never in the metric
    assert md[2 * 8 + 6] == ("g", "g", True, False) and md[2 * 8 + 7] == ("g", "g", False, False)
    assert md[1 * 8 + 7] == (("Y", 1), "g", False, False)
    assert md[24] == (("S", 1), ("S", 1), False, True)
    assert ex == [("g", "dir", False, False), ("x", "x", False, False), ("x", "x", False, True)]


def test_metric_needs_both_flags_and_rounds_in_float32():
    rng = np.random.default_rng(3)
    a, b = rng.normal(size=(2, 64)).astype(np.float32)
    dinv = rng.uniform(0.5, 2.0, size=64).astype(np.float32)
    val, _ = tw.multidot([a, a], [b, b], dinv, wq=0b01, wb=0b10)
    plain = tw.dot(a, b)[0]
    weighted = float(((a * dinv).astype(np.float64) * b.astype(np.float64)).astype(np.longdouble).sum())
    assert val[0, 0] == plain and val[1, 0] == plain and val[1, 1] == plain and val[0, 1] == weighted
    assert weighted != float((a.astype(np.float64) * dinv.astype(np.float64) * b.astype(np.float64)).sum())
    assert tw.multidot([a], [b], None, wq=1, wb=1)[0][0, 0] == plain


def test_precond_diagonal_twin_matches_its_formulas_entry_by_entry():
    rng = np.random.default_rng(5)
    L, q, neff, lh, lj = 3, 4, 17.5, 0.01, 0.3
    f = rng.dirichlet(np.ones(q), size=L).astype(np.float32)
    for gap in (False, True):
        fi = f.copy()
        if gap:
            fi[:, 0] = 0
        d, zero = tw.precond_diagonal(fi, neff, lh, lj, gap)
        assert d.size == L * q + 3 * q * q and np.array_equal(d == 0, zero)
        a0 = 1 if gap else 0
        f64 = fi.astype(np.float64)
        p = [(f64[i, a0:] + 1 / neff) / (f64[i, a0:] + 1 / neff).sum() for i in range(L)]
        v = lambda i, a: p[i][a - a0] * (1 - p[i][a - a0])
        assert d[1 * q + 2] == pytest.approx(1 / (neff * v(1, 2) + 2 * lh), rel=1e-14)
        pair_02 = L * q + 1 * q * q                       # pairs in order (0,1), (0,2), (1,2)
        assert d[pair_02 + 1 * q + 3] == pytest.approx(1 / (neff * (f64[2, 3] * v(0, 1) + f64[0, 1] * v(2, 3)) + 2 * lj), rel=1e-14)
        assert (d[pair_02 + 0 * q + 3] == 0) == gap and (d[0] == 0) == gap


# ---- invalid arguments of the diagnostic entries: refused before any device call, so this runs without a GPU too ------
def check_error_paths():
    """every invalid argument returns PLM_EINVAL with a message, and no output is touched (they stay NaN)"""
    from evcouplings_amd import _lib
    lib = _lib.load()
    PLM_EINVAL = -1
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    f32 = lambda *shape: np.ones(shape, np.float32)

    def refused(rc, outs):
        assert rc == PLM_EINVAL
        assert lib.plm_last_error()
        for o in outs:
            assert np.isnan(o).all()

    def gram(n, nh, m, end, nst, rows=None):
        rows = max(1, min(nst, 21)) if rows is None else rows
        S, Y = f32(rows, max(n, 4)), f32(rows, max(n, 4))
        v = f32(max(n, 4))
        outs = [np.full(max(n, 4), np.nan, np.float32), np.full(max(n, 4), np.nan, np.float32),
                np.full(3 * 44 + 1, np.nan), np.full(3, np.nan)]
        rc = lib.plm_lbfgs_gram(n, nh, m, end, nst, p(S), p(Y), p(v), p(v), p(v), p(v), p(v), None, 0, *[p(o) for o in outs])
        refused(rc, outs)

    gram(1026, 0, 6, 0, 1)            # n not a multiple of 4
    gram(1028, 6, 6, 0, 1)            # nh not a multiple of 4
    gram(1028, 1032, 6, 0, 1)         # nh > n
    gram(1028, 0, 21, 0, 21)          # 44 basis vectors
    gram(1028, 0, 6, 6, 6)            # end >= m
    gram(1028, 0, 6, 7, 6)
    gram(1028, 0, 6, -1, 6)
    gram(1028, 0, 6, 0, 7)            # nst > m
    gram(1028, 0, 6, 3, 2)            # the pair's slot is not in the basis
    gram(0, 0, 6, 0, 1)

    def direction(n, m, stored, end, trial_without_xacc=False):
        S, Y, g = f32(m, max(n, 4)), f32(m, max(n, 4)), f32(max(n, 4))
        cs, cy = np.ones(m), np.ones(m)
        outs = [np.full(max(n, 4), np.nan, np.float32), np.full(max(n, 4), np.nan, np.float32)]
        rc = lib.plm_lbfgs_direction(n, m, stored, end, p(S), p(Y), p(g), p(cs), p(cy), -1.0, None,
                                     None if trial_without_xacc else p(g), 0.5, 0, p(outs[0]), p(outs[1]))
        refused(rc, outs)

    direction(1030, 6, 3, 3)          # n not a multiple of 4
    direction(1028, 22, 21, 0)        # 43 basis vectors
    direction(1028, 6, 3, 6)          # end >= m
    direction(1028, 6, 7, 0)          # stored > m
    direction(1028, 6, 3, 3, trial_without_xacc=True)

    def multidot(n, nq, nb, bad_index=False):
        V = f32(2, max(n, 4))
        qi = np.zeros(max(nq, 1), np.int32)
        bi = np.full(max(nb, 1), 2 if bad_index else 1, np.int32)
        out = np.full(5 * 44, np.nan)
        refused(lib.plm_lbfgs_multidot(n, 2, p(V), nq, p(qi), nb, p(bi), None, 0, 0, 0, p(out)), [out])

    multidot(1029, 1, 1)              # n not a multiple of 4
    multidot(1028, 5, 1)              # more than 4 queries
    multidot(1028, 0, 1)
    multidot(1028, 1, 43)             # more than 42 basis vectors
    multidot(1028, 1, 0)
    multidot(1028, 1, 2, bad_index=True)

    def dots(stride, npairs, n):
        V = f32(2, max(stride, 4))
        ai, bi = np.zeros(max(npairs, 1), np.int32), np.ones(max(npairs, 1), np.int32)
        out = np.full(8, np.nan)
        refused(lib.plm_lbfgs_dots(stride, 2, p(V), npairs, p(ai), p(bi), n, 0, p(out)), [out])

    dots(1028, 5, 1028)               # more than 4 pairs
    dots(1028, 0, 1028)
    dots(1028, 1, 1026)               # prefix not a multiple of 4
    dots(1028, 1, 1032)               # prefix beyond the vectors
    dots(1027, 1, 4)

    a, out = f32(1028), np.full(1028, np.nan, np.float32)
    refused(lib.plm_lbfgs_lincomb(1027, 1.0, p(a), 1.0, p(a), 0, p(out)), [out])
    refused(lib.plm_lbfgs_lincomb(1028, 1.0, None, 1.0, p(a), 0, p(out)), [out])
    assert lib.plm_ctx_precond_diagonal(None, p(out)) == PLM_EINVAL and np.isnan(out).all()


def test_invalid_arguments_are_refused_before_any_device_call():
    check_error_paths()
