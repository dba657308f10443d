"""
Float64 twin of the L-BFGS vector kernels (plm_kernels.hip: k_dots, k_lincomb, k_multidot, k_multiaxpy, k_sy_multidot) and of
the H0 diagonal (k_precond_j / k_precond_h).  Plain numpy, nothing imported from the library.

Arithmetic the twin shares with the kernels, so that the GPU tests need no measured tolerance:
  * the pair s = x - xp, y = g - gp is ONE float32 subtraction per entry: bit-exact;
  * a product of two float32 values is exact in float64; the twin sums the exact products in extended precision
    (numpy.longdouble, pairwise), so its own error is far below one f64 rounding of the result;
  * in the H0 metric a flagged query is first multiplied by dinv in float32 (rounded to float32), then by the basis entry in
    float64 -- and only where BOTH the query and the basis vector are flagged and a dinv is given.
Every dot comes with sum |a_i b_i|, the yardstick of the GPU test's bound n 2^-53 sum |a_i b_i|.
"""
import numpy as np

F32, F64, LD = np.float32, np.float64, np.longdouble


# ---- the pair ------------------------------------------------------------------------------------------------------------
def pair(x, xp, g, gp):
    x, xp, g, gp = (np.asarray(a, F32) for a in (x, xp, g, gp))
    return x - xp, g - gp


# ---- dot products --------------------------------------------------------------------------------------------------------
def dot(a, b, dinv=None, n=None):
    """(sum a_i b_i, sum |a_i b_i|) over the first n entries (default all); dinv: the H0 metric on the query side `a`"""
    a, b = np.asarray(a, F32)[:n], np.asarray(b, F32)[:n]
    if dinv is not None:
        a = a * np.asarray(dinv, F32)[:n]              # float32 product, rounded: the kernel's qd
    p = a.astype(F64) * b.astype(F64)                  # exact
    return float(p.astype(LD).sum()), float(np.abs(p).sum())


def multidot(queries, basis, dinv=None, wq=0, wb=0, n=None):
    """out[q][k] = <queries[q], basis[k]>; bit q of wq and bit k of wb both set and dinv given: in the metric.
    Returns (values, abs sums), each (len(queries), len(basis)) float64."""
    val, mag = np.zeros((len(queries), len(basis))), np.zeros((len(queries), len(basis)))
    for q, a in enumerate(queries):
        for k, b in enumerate(basis):
            metric = dinv is not None and (wq >> q) & 1 and (wb >> k) & 1
            val[q, k], mag[q, k] = dot(a, b, dinv if metric else None, n)
    return val, mag


# ---- the Gram pass ---------------------------------------------------------------------------------------------------------
def gram_layout(m, end, nst):
    """What plm_ctx_optimize reads from the Gram pass, written down from its rules (not from the C helper): the new pair
    sits in ring slot `end`, the basis is S[0..nst), Y[0..nst), g, g (nb = 2 nst + 2); the Y's and the first g are flagged on
    the basis side, the queries y_new and g on the query side.
    Returns (md, ex): lists of (query, basis, metric, prefix) with vectors named ("S", slot), ("Y", slot), "g", "x", "dir"
    and prefix = True for a sum over the first nh entries only.
      md[q nb + pos], q = (s_new, y_new, g);  md[3 nb] = s_new.s_new over the fields;  ex = g.dir, x.x, x.x (fields)"""
    assert 1 <= nst <= m and 0 <= end < nst
    basis = [("S", i) for i in range(nst)] + [("Y", i) for i in range(nst)] + ["g", "g"]
    flagged_b = [False] * nst + [True] * nst + [True, False]
    queries = [("S", end), ("Y", end), "g"]
    flagged_q = [False, True, True]
    md = [(qv, bv, fq and fb, False) for qv, fq in zip(queries, flagged_q) for bv, fb in zip(basis, flagged_b)]
    md.append((("S", end), ("S", end), False, True))
    ex = [("g", "dir", False, False), ("x", "x", False, False), ("x", "x", False, True)]
    return md, ex


def gram(S, Y, x, xp, g, gp, direction, m, end, nst, nh, dinv=None):
    """The pass on explicit vectors: (s_new, y_new, md, md_abs, ex, ex_abs).  Slot `end` of S / Y is never read."""
    s_new, y_new = pair(x, xp, g, gp)
    vec = {"g": np.asarray(g, F32), "x": np.asarray(x, F32), "dir": np.asarray(direction, F32)}
    for i in range(nst):
        vec[("S", i)] = s_new if i == end else np.asarray(S[i], F32)
        vec[("Y", i)] = y_new if i == end else np.asarray(Y[i], F32)
    md_l, ex_l = gram_layout(m, end, nst)
    cache = {}

    def entry(e):
        qv, bv, metric, prefix = e
        key = (qv, bv, bool(metric and dinv is not None), prefix)
        if key not in cache:
            cache[key] = dot(vec[qv], vec[bv], dinv if key[2] else None, nh if prefix else None)
        return cache[key]

    md = np.array([entry(e) for e in md_l])
    ex = np.array([entry(e) for e in ex_l])
    return s_new, y_new, md[:, 0], md[:, 1], ex[:, 0], ex[:, 1]


def gram_to_host(md, m, end, nst):
    """The host's Gram pieces of the slots the pass covers, by the indexing plm_ctx_optimize applies to md after an
    accepted step (slot e = end): SY, YDY (m x m), Sg, YDg (m), gDg, gg.  Entries between two OLD slots are not part of
    one pass (the host keeps them from earlier passes) and stay NaN here."""
    nb, e = 2 * nst + 2, end
    SY, YDY = np.full((m, m), np.nan), np.full((m, m), np.nan)
    Sg, YDg = np.full(m, np.nan), np.full(m, np.nan)
    for j in range(nst):
        SY[e, j] = md[0 * nb + nst + j]
        SY[j, e] = md[1 * nb + j]
        YDY[e, j] = YDY[j, e] = md[1 * nb + nst + j]
        Sg[j] = md[2 * nb + j]
        YDg[j] = md[2 * nb + nst + j]
    return SY, YDY, Sg, YDg, md[2 * nb + 2 * nst], md[2 * nb + 2 * nst + 1]


# ---- the direction ---------------------------------------------------------------------------------------------------------
def live_slots(m, stored, end):
    """live ring slots, newest first"""
    return [(end - 1 - i) % m for i in range(stored)]


def direction(S, Y, g, cs, cy, cg, m, stored, end, dinv=None):
    """p = sum cs_j s_j + dinv (.) (sum cy_j y_j + cg g) over the live slots in float64, and the magnitude
    sum |cs_j s_j| + dinv (.) (sum |cy_j y_j| + |cg g|) the rounding bound of the f32 kernel is stated in"""
    g = np.asarray(g, F64)
    d = np.ones_like(g) if dinv is None else np.asarray(dinv, F64)
    plain, weighted = np.zeros_like(g), float(cg) * g
    mag_p, mag_w = np.zeros_like(g), np.abs(float(cg) * g)
    for j in live_slots(m, stored, end):
        sj, yj = np.asarray(S[j], F64), np.asarray(Y[j], F64)
        plain += cs[j] * sj
        weighted += cy[j] * yj
        mag_p += np.abs(cs[j] * sj)
        mag_w += np.abs(cy[j] * yj)
    return plain + d * weighted, mag_p + d * mag_w


def trial_point(xacc, stp0, dir32):
    """xacc + stp0 float32(dir) in float64, and |xacc| + |stp0 dir|"""
    xacc, dir32 = np.asarray(xacc, F32).astype(F64), np.asarray(dir32, F32).astype(F64)
    stp0 = float(F32(stp0))
    return xacc + stp0 * dir32, np.abs(xacc) + np.abs(stp0 * dir32)


def lincomb(ca, a, cb=0.0, b=None):
    """ca a + cb b in float64 (coefficients as the float32 the kernel receives), and |ca a| + |cb b|"""
    ca, cb = float(F32(ca)), float(F32(cb))
    a = np.asarray(a, F32).astype(F64)
    if b is None:
        return ca * a, np.abs(ca * a)
    b = np.asarray(b, F32).astype(F64)
    return ca * a + cb * b, np.abs(ca * a) + np.abs(cb * b)


def gram_dense(S, Y, g, m, live, dinv=None, exact=True):
    """Gram pieces of plm_lbfgs_coefficients for the live slots from explicit vectors (dead slots NaN).  exact = False:
    float64 matrix products instead of extended-precision sums -- for long vectors, where the pieces only serve as the
    input of plm_lbfgs_coefficients and are compared with nothing."""
    SY, YDY = np.full((m, m), np.nan), np.full((m, m), np.nan)
    Sg, YDg = np.full(m, np.nan), np.full(m, np.nan)
    if not exact:
        live = list(live)
        g64 = np.asarray(g, F64)
        gd = g64 if dinv is None else (np.asarray(g, F32) * np.asarray(dinv, F32)).astype(F64)
        if live:
            s = np.asarray(S, F32)[live].astype(F64)
            y = np.asarray(Y, F32)[live].astype(F64)
            yd = y if dinv is None else (np.asarray(Y, F32)[live] * np.asarray(dinv, F32)).astype(F64)
            SY[np.ix_(live, live)] = s @ y.T
            YDY[np.ix_(live, live)] = yd @ y.T
            Sg[live], YDg[live] = s @ g64, yd @ g64
        return SY, YDY, Sg, YDg, float(gd @ g64)
    for i in live:
        for j in live:
            SY[i, j] = dot(S[i], Y[j])[0]
            YDY[i, j] = dot(Y[i], Y[j], dinv)[0]
        Sg[i] = dot(S[i], g)[0]
        YDg[i] = dot(Y[i], g, dinv)[0]
    return SY, YDY, Sg, YDg, dot(g, g, dinv)[0]


# ---- the H0 diagonal -----------------------------------------------------------------------------------------------------
def precond_diagonal(fi, n_eff, lambda_h, lambda_j, gap_mode=False):
    """1 / (Hessian diagonal of the independent-site model at the start point), canonical layout (h [L][q], then the i<j
    blocks [q][q]), float64.  With p_i = (f_i + 1/N_eff) / sum (the start distribution; gap mode: over states >= 1) and
    v = p (1 - p):   d2f/dh_i(a)^2 = N_eff v_i(a) + 2 lambda_h,
                     d2f/dJ_ij(a,b)^2 = N_eff (f_j(b) v_i(a) + f_i(a) v_j(b)) + 2 lambda_J.
    Gap mode: every entry that involves state 0 is a structural zero.  Returns (dinv, structural-zero mask)."""
    f = np.asarray(fi, F32).astype(F64)
    L, q = f.shape
    a0 = 1 if gap_mode else 0
    p = np.zeros_like(f)
    p[:, a0:] = f[:, a0:] + 1.0 / n_eff
    p /= p.sum(axis=1, keepdims=True)
    v = p * (1.0 - p)
    dh = 1.0 / (n_eff * v + 2.0 * lambda_h)
    zh = np.zeros((L, q), bool)
    ii, jj = np.triu_indices(L, 1)
    dj = 1.0 / (n_eff * (f[jj][:, None, :] * v[ii][:, :, None] + f[ii][:, :, None] * v[jj][:, None, :]) + 2.0 * lambda_j)
    zj = np.zeros(dj.shape, bool)
    if gap_mode:
        zh[:, 0] = True
        zj[:, 0, :] = zj[:, :, 0] = True
    dh[zh] = 0.0
    dj[zj] = 0.0
    return np.concatenate([dh.ravel(), dj.ravel()]), np.concatenate([zh.ravel(), zj.ravel()])
