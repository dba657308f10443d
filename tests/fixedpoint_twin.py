"""
Integer twin of the fixed-point operands of the two GEMMs (DESIGN_NEXT_ROWS.md 9.17), written from
the comments of evcouplings_amd/csrc/plm_kernels.hip and plm_host.cpp -- numpy and Python integers only:

  forward   k_maxabs / k_scale_from_max (jexp), k_expand_x + k_fwd_x (39-bit fixed point in five signed base-256 digit
            planes, int32 / int64 sums, one f64 and one f32 rounding) and, for operands of at most 22 bits, k_expand +
            k_fwd (hi + lo f16 planes, f32 accumulation): potentials_exact()
  backward  R = rint(f32(w rscale) (P - [x = a])) (k_hpass, k_onehot_rt), its signed digits (digits_of / planes_of4),
            the int32 slabs of k_bwd / k_bwd_w against the -128 one-hot and g_combine / k_assemble: residual_ints(),
            pair_sums(), marginals_expected(), gradient_expected()

Every function asserts the preconditions under which its result is what the kernels must produce BIT FOR BIT; an input
that breaks one fails here, not silently on the GPU.  The shared case lists of tests/test_fixedpoint_twin_host.py (CPU:
preconditions of every case, twin against the f64 oracle) and tests/test_gpu_fixedpoint.py (GPU) are at the end.
"""
import math

import numpy as np

F32, F64, I64 = np.float32, np.float64, np.int64
PLM_R_EXP = 14                                    # plm_internal.h
FWDX_SHIFT, FWDX_PLANES = 23, 5                   # plm_kernels.hip PLM_FWDX_SHIFT / PLM_FWDX_PLANES
QMAX = {3: 8355000.0, 4: 2138000000.0}            # PLM_R_QMAX3 / PLM_R_QMAX4
ONEHOT = -128                                     # PLM_BWD_ONEHOT_VALUE
BIAS5 = 0x8080808080
SATURATED_FIELD = 64.0


# ------------------------------------------------------------------------------------------------ forward operands
def jexp(jij):
    """k_scale_from_max: 14 - frexp exponent of max|J| over the couplings, clamped to +-100; 0 for an all-zero model"""
    m = float(np.abs(np.asarray(jij, dtype=F32)).max()) if np.size(jij) else 0.0
    if not m > 0.0:
        return 0
    assert math.isfinite(m)
    return max(-100, min(100, PLM_R_EXP - math.frexp(m)[1]))


def digits5(D):
    """the five signed base-256 digits of D (k_expand_x): bytes of (D + 0x8080808080) ^ 0x8080808080; |D| < 2^38"""
    D = np.asarray(D, dtype=I64)
    assert (np.abs(D) < 2 ** 38).all(), "a scaled difference of 2^38 or more has no five-digit form"
    u = (D + BIAS5) ^ BIAS5
    d = np.stack([((u >> (8 * p)) & 0xff).astype(np.uint8).view(np.int8) for p in range(FWDX_PLANES)], axis=-1)
    return d


def undigits5(d):
    return sum(d[..., p].astype(I64) << (8 * p) for p in range(FWDX_PLANES))


def full_couplings(jij, L, q):
    """J4[i, j, a, b] = J_ij(a, b) for every ordered pair (zero for i == j) from the i < j blocks [L(L-1)/2][q][q]"""
    jij = np.asarray(jij, dtype=F32).reshape(L * (L - 1) // 2, q, q)
    J4 = np.zeros((L, L, q, q), dtype=F32)
    iu, ju = np.triu_indices(L, 1)
    J4[iu, ju] = jij
    J4[ju, iu] = jij.transpose(0, 2, 1)
    return J4


def _unit_exponent(x):
    """exponent u of the largest power of two that divides every non-zero entry of the f64 array x (None: all zero)"""
    x = np.abs(np.asarray(x, dtype=F64))
    x = x[x > 0]
    if x.size == 0:
        return None
    m, e = np.frexp(x)
    mi = np.ldexp(m, 53).astype(I64)                     # exact: 53-bit integers
    low = (mi & -mi).astype(F64)
    return int((np.log2(low) + e - 53).min())


def order_independent(x, axis):
    """True where the f64 sum of x along `axis` is exact in ANY order: all terms are multiples of 2^u and the sum of the
    magnitudes stays below 2^(u + 53), so every partial sum of every subset is representable."""
    u = _unit_exponent(x)
    if u is None:
        return True
    return bool((np.abs(np.asarray(x, dtype=F64)).sum(axis=axis) < math.ldexp(1.0, u + 53)).all())


def scaled_differences(jij, L, q):
    """D[i, j, a, b] = rint((J_ij(a,b) - J_ij(a,0)) 2^(jexp + 23)), difference in f64, ties to even (k_expand_x);
    C[i, a] = sum_{j != i} J_ij(a, 0) in f64 (k_fwd_ref).  Asserts |D| < 2^38 and that C does not depend on the order of
    its additions (the kernel adds 64 strided partial sums in a shuffle tree)."""
    J4 = full_couplings(jij, L, q).astype(F64)
    je = jexp(jij)
    diff = J4 - J4[:, :, :, :1]
    D = np.rint(np.ldexp(diff, je + FWDX_SHIFT))
    assert (np.abs(D) < 2.0 ** 38).all()
    D = D.astype(I64)
    ref = J4[:, :, :, 0]                                 # [i, j, a]; zero on the diagonal
    assert order_independent(ref, axis=1), "the reference-state constant of this model depends on the summation order"
    C = ref.sum(axis=1)
    return D, C, je


def potentials_exact(seqs, q, jij, with_digits=False, rounded=True):
    """HJ[s, i, a] = sum_{j != i} J_ij(a, x_sj) as k_fwd_x must return it: S = sum_j D (integers), then
    float32(float64(S 2^-(jexp + 23) + C_i(a))) -- one f64 rounding, one f32 rounding.  The integer sum fits int64
    (|S| <= L 2^38) and 128 |S| < 2^53 (the kernel's sums carry the -128 of the one-hot operand into its f64 fma).
    with_digits: also the five digits of every D, [i, j, a, b, plane], and the mask of the (i, j, a, b) some sequence
    visits.  rounded=False: the float64 value before the last rounding (for comparisons with a float64 reference)."""
    seqs = np.asarray(seqs)
    N, L = seqs.shape
    assert seqs.min() >= 0 and seqs.max() < q
    D, C, je = scaled_differences(jij, L, q)
    assert L * 2 ** 38 * 128 < 2 ** 53
    S = np.zeros((N, L, q), dtype=I64)
    for j in range(L):
        S += D[:, j, :, :][:, :, seqs[:, j]].transpose(2, 0, 1)          # [s, i, a]
    v = np.ldexp(S.astype(F64), -(je + FWDX_SHIFT))                        # exact: |S| < 2^53, a power-of-two scale
    assert (np.ldexp(v, je + FWDX_SHIFT) == S).all()
    out = v + C[None]
    if rounded:
        out = out.astype(F32)
    if not with_digits:
        return out
    visited = np.zeros(D.shape, dtype=bool)
    for j in range(L):
        for b in np.unique(seqs[:, j]):
            visited[:, j, :, b] = True
    visited[np.arange(L), np.arange(L)] = False
    return out, digits5(D), visited


def planes_exercised(dig, visited):
    """the digit planes in which some VISITED difference has a non-zero digit"""
    return tuple(p for p in range(FWDX_PLANES) if (dig[..., p][visited] != 0).any())


def plain_preconditions(jij, L, q):
    """The conditions under which the PLAIN forward GEMM (k_expand + k_fwd: hi = f16(v), lo = f16(v - hi) of the f32
    difference v = (J(a,b) - J(a,0)) 2^jexp, f32 accumulation) must equal potentials_exact() bit for bit:
      * the f32 difference is exact and hi + lo == v (at most 22 significant bits, nothing below f16's 2^-24);
      * every sum of magnitudes over j -- hence every partial sum in any order, plane by plane -- stays below 2^24 units
        of the smallest bit in use: f32 accumulation loses nothing, however the matrix core orders or aligns it.
    Returns (fraction of the non-zero differences whose lo plane is non-zero, largest sum in units)."""
    J4 = full_couplings(jij, L, q)
    je = jexp(jij)
    d32 = J4 - J4[:, :, :, :1]
    assert (d32.astype(F64) == J4.astype(F64) - J4[:, :, :, :1].astype(F64)).all(), "f32 difference not exact"
    v = np.ldexp(d32, je).astype(F32)
    assert (v.astype(F64) == np.ldexp(d32.astype(F64), je)).all()
    hi = v.astype(np.float16)
    assert np.isfinite(hi).all()
    lo = (v - hi.astype(F32)).astype(np.float16)
    assert (hi.astype(F64) + lo.astype(F64) == v.astype(F64)).all(), "a difference does not fit hi + lo f16 planes"
    u = _unit_exponent(np.concatenate([hi.astype(F64).ravel(), lo.astype(F64).ravel()]))
    if u is None:
        return 0.0, 0
    mag = np.abs(hi.astype(F64)) + np.abs(lo.astype(F64))
    units = np.ldexp(mag.max(axis=3).sum(axis=1), -u).max()               # worst state per neighbour, all neighbours
    assert units < 2 ** 24, "a partial sum can reach 2^24 units: f32 accumulation may round"
    # with D = v 2^23 an integer the two kernels share one expected value
    assert (np.ldexp(v.astype(F64), FWDX_SHIFT) == np.rint(np.ldexp(v.astype(F64), FWDX_SHIFT))).all()
    nz = v != 0
    return float((lo != 0)[nz].mean()) if nz.any() else 0.0, int(units)


def split_difference(D, je=0):
    """two f32 values A, B with (A - B) 2^(je + 23) == D exactly and |A|, |B| < 2^(14 - je): A carries the bits of D from
    2^14 up (at most 24 of them), B minus the signed remainder.  Used to place chosen digit patterns in a model."""
    D = int(D)
    lowbits = ((D + 2 ** 13) % 2 ** 14) - 2 ** 13
    hi = D - lowbits
    A, B = F32(math.ldexp(hi, -(je + FWDX_SHIFT))), F32(math.ldexp(-lowbits, -(je + FWDX_SHIFT)))
    assert int(math.ldexp(float(A), je + FWDX_SHIFT)) == hi and int(math.ldexp(float(B), je + FWDX_SHIFT)) == -lowbits
    assert abs(float(A)) < 2.0 ** (14 - je) and abs(float(B)) < 2.0 ** (14 - je)
    return A, B


# ------------------------------------------------------------------------------------------------ backward operands
def rscale_of(w, planes):
    """ctx_set_accurate: rscale = QMAX / wmax, gscale = wmax / (QMAX * -128), both formed in float32"""
    wmax = F32(np.asarray(w, dtype=F32).max())
    assert wmax > 0
    qmax = F32(QMAX[planes])
    return F32(qmax / wmax), F32(wmax / F32(qmax * F32(ONEHOT)))


def residual_ints(w, planes):
    """R_s = rint(float32(w_s) * float32(rscale)) in float32 (ties to even), as int64; |R| <= QMAX by construction"""
    w = np.asarray(w, dtype=F32)
    assert (w >= 0).all() and np.isfinite(w).all()
    rscale, _ = rscale_of(w, planes)
    R = np.rint((w * rscale).astype(F32)).astype(I64)
    lim = 127 * sum(256 ** k for k in range(planes))
    assert (np.abs(R) <= lim).all()
    return R


def digits_of_residual(R, planes):
    """signed digits of digits_of(): bytes of (R + bias) ^ bias in 32-bit wrap-around arithmetic"""
    bias = 0x80808080 if planes == 4 else 0x00808080
    u = ((np.asarray(R, dtype=I64) + bias) & 0xffffffff) ^ bias
    return np.stack([((u >> (8 * p)) & 0xff).astype(np.uint8).view(np.int8) for p in range(planes)], axis=-1)


def onehot(msa, q):
    msa = np.asarray(msa)
    return (msa[:, :, None] == np.arange(q)[None, None, :])


def marginal_site_ints(msa, q, R):
    """R[s, (i, a)] of k_onehot_rt: R_s [x_si = a]"""
    return onehot(msa, q) * np.asarray(R, dtype=I64)[:, None, None]


def saturated_fields(L, q, astar):
    h = np.zeros((L, q), dtype=F32)
    h[np.arange(L), astar] = SATURATED_FIELD
    return h


def residual_site_ints(msa, q, R, astar, gap):
    """R[s, (i, a)] of k_hpass at zero couplings and fields 64 on state astar[i], 0 elsewhere: the softmax is exactly
    (Z, P(a*)) = (1, 1), every other P times w rscale rounds to 0, so R_s(i, a) = R_s ([a = a*_i] - [a = x_si]); in gap
    mode a sequence has no weight at a site where it holds state 0."""
    msa = np.asarray(msa)
    N, L = msa.shape
    astar = np.asarray(astar)
    assert not gap or (astar >= 1).all()
    # what the kernel's float32 arithmetic does with the other states: exp(-64) (1 + (q - 1) exp(-64)) rounds Z to 1 and
    # QMAX4 exp(-64) is far below one half
    assert F32(1.0) + F32((q - 1) * math.exp(-SATURATED_FIELD)) == F32(1.0)
    assert QMAX[4] * q * math.exp(-SATURATED_FIELD) * 1.01 < 0.5
    out = (np.arange(q)[None, None, :] == astar[None, :, None]).astype(I64) - onehot(msa, q).astype(I64)
    out = out * np.asarray(R, dtype=I64)[:, None, None]
    if gap:
        out[msa == 0] = 0
    return out


def pair_sums(msa, Rsite, q):
    """V[i, a, j, b] = sum_s Rsite[s, i, a] [x_sj = b], exact integers.  Computed by a float64 matrix product; the
    assertion makes that exact (sum of magnitudes below 2^53)."""
    msa = np.asarray(msa)
    N, L = msa.shape
    A = np.asarray(Rsite, dtype=I64).reshape(N, L * q)
    assert int(np.abs(A).sum(axis=0).max()) < 2 ** 53
    V = A.astype(F64).T @ onehot(msa, q).reshape(N, L * q).astype(F64)
    return V.astype(I64).reshape(L, q, L, q)


def sequences_per_cell(msa, Rsite, q):
    """number of sequences that contribute a non-zero R to every cell ((i, a), (j, b))"""
    msa = np.asarray(msa)
    N, L = msa.shape
    A = (np.asarray(Rsite).reshape(N, L * q) != 0).astype(F64)
    return (A.T @ onehot(msa, q).reshape(N, L * q).astype(F64)).astype(I64).reshape(L, q, L, q)


def headroom(msa, Rsite, q, planes, ksteps_per_range=None):
    """largest |int32 partial| of any digit plane: sum over the sequences of one K range of -128 digit [x_sj = b] (an upper
    bound over ranges: the whole alignment as one range unless the K steps of 128 sequences per range are given).  Must stay
    below 2^31."""
    msa = np.asarray(msa)
    N, L = msa.shape
    dig = digits_of_residual(np.asarray(Rsite, dtype=I64).reshape(N, L * q), planes)
    oh = onehot(msa, q).reshape(N, L * q).astype(F64)
    worst = 0
    step = N if ksteps_per_range is None else 128 * ksteps_per_range
    for s0 in range(0, N, step):
        for p in range(planes):
            G = (dig[s0:s0 + step, :, p].astype(F64).T @ oh[s0:s0 + step]) * ONEHOT
            worst = max(worst, int(np.abs(G).max()))
    return worst


def neff_of(w):
    """plm_ctx_set_weights: the float32 weights added up in order in a double"""
    acc = 0.0
    for x in np.asarray(w, dtype=F32).tolist():
        acc += x
    return acc


def pair_blocks(V):
    """[L, q, L, q] -> the i < j blocks [L(L-1)/2][q][q]"""
    L = V.shape[0]
    iu, ju = np.triu_indices(L, 1)
    return V[iu, :, ju, :]


def combine(V, unit=1):
    """g_combine: the planes' int64 sums, weighted 256^p, added in f64 and rounded ONCE to float32.  The f64 sum is the
    exact integer -128 V when every plane sum is a multiple of 128 * unit and 128 |V| < 2^53 lowbit(128 * unit) (unit = 1
    in general; unit = N for N equal sequences of equal weight, whose plane sums are -128 N digit)."""
    V = np.asarray(V, dtype=I64)
    u = 128 * int(unit)
    low = u & -u
    assert all(abs(int(v)) * 128 < 2 ** 53 * low and int(v) % int(unit) == 0 for v in (V.min(), V.max()))
    return np.array([float(int(v) * ONEHOT) for v in V.ravel().tolist()], dtype=F64).reshape(V.shape).astype(F32) \
        if unit != 1 else (V * ONEHOT).astype(F64).astype(F32)


def marginal_scale(w, planes, gap):
    _, gscale = rscale_of(w, planes)
    inv = F32(1.0) if gap else F32(1.0 / neff_of(w))
    return F32(gscale * inv)


def marginals_expected(V, w, planes, gap):
    """pair frequencies as plm_ctx_marginals must return them from the integer sums V[i, a, j, b]: k_assemble mode 1 gives
    scale * float32(-128 V) with scale = float32(gscale * float32(1 / n_eff)), one float32 product; gap mode: raw counts
    (scale = gscale), then every block divided by its f64 total over a, b >= 1 in block order, row and column 0 dropped."""
    scale = marginal_scale(w, planes, gap)
    f = (scale * combine(pair_blocks(V))).astype(F32)
    if not gap:
        return f, scale
    out = np.zeros((f.shape[0], f.shape[1] - 1, f.shape[2] - 1), dtype=F32)
    for k in range(f.shape[0]):
        tot = 0.0
        for x in f[k, 1:, 1:].ravel().tolist():
            tot += x
        if tot > 0:
            out[k] = (f[k, 1:, 1:].astype(F64) / tot).astype(F32)
    return out, scale


def gradient_expected(V, w, planes, gap):
    """pair gradient at zero couplings: k_assemble mode 0 gives fma(gscale, float32(-128 V1) + float32(-128 V2), 0) with
    V1 = V[i, a, j, b] and V2 = V[j, b, i, a]: one float32 sum, one float32 product.  Also returns V1 + V2, gscale and
    max(|V1|, |V2|)."""
    _, gscale = rscale_of(w, planes)
    V1 = pair_blocks(V)
    V2 = pair_blocks(V.transpose(2, 3, 0, 1))                       # [pair, a, b] = V[j, b, i, a]
    g = (gscale * (combine(V1) + combine(V2)).astype(F32)).astype(F32)
    Vs, Vmag = V1 + V2, np.maximum(np.abs(V1), np.abs(V2))
    if gap:
        g, Vs, Vmag = g[:, 1:, 1:], Vs[:, 1:, 1:], Vmag[:, 1:, 1:]
    return g, Vs, gscale, Vmag


def recover_ints(out, scale):
    """the integer behind an output: rint(out / (scale * -128)) in float64 (scale holds the sign of the -128 one-hot, the
    slabs its magnitude); exact for |V| < 2^22, where the float32 roundings stay under a quarter unit"""
    return np.rint(np.asarray(out, dtype=F64) / (float(scale) * ONEHOT)).astype(I64)


# ------------------------------------------------------------------------------------------------ models of the cases
def _sequences(rng, N, L, q, forbid=()):
    """random states with state 0 (the reference state) and state q - 1 present in every column where N allows; forbid:
    (site, state) pairs no sequence may hold"""
    s = rng.integers(0, q, size=(N, L)).astype(np.int8)
    if N >= 3:
        s[0, :] = 0
        s[1, :] = q - 1
    for site, state in forbid:
        col = s[:, site]
        col[col == state] = (state - 1) % q
    return s


def model_general(L, q, seed):
    """0.1 * normal rounded to a 2^-20 grid: every f64 sum of couplings is exact in any order"""
    rng = np.random.default_rng(seed)
    j = 0.1 * rng.standard_normal((L * (L - 1) // 2, q, q))
    return (np.rint(j * 2 ** 20) / 2 ** 20).astype(F32)


DOMINANT = 8192.0          # frexp exponent 14: jexp = 0, one unit of D is 2^-23


def _dominant_slot(L, q):
    """the (pair, a, b) of the dominant coupling and the (site, state) pairs a sequence must avoid so as not to visit it:
    pair (0, 1), states (q - 2, q - 2) -- not the reference state, whose entry would enter every difference of its row"""
    a = max(1, q - 2)
    return (0, a, a), ((0, a), (1, a))


def model_planes(L, q, lo_plane, seed):
    """every coupling E 2^-23 with E = e_p 256^p + e_(p+1) 256^(p+1), |e| <= 60 (15 in plane 4): the differences to state 0
    have digits of at most 120 (30) in planes p, p + 1 and none elsewhere -- no carries.  One dominant coupling of 8192
    fixes jexp = 0."""
    rng = np.random.default_rng(seed)
    p = lo_plane
    top = 15 if p + 1 == 4 else 60
    shape = (L * (L - 1) // 2, q, q)
    E = rng.integers(-60, 61, size=shape) * 256 ** p + rng.integers(-top, top + 1, size=shape) * 256 ** (p + 1)
    j = np.ldexp(E.astype(F64), -FWDX_SHIFT).astype(F32)
    assert (np.ldexp(j.astype(F64), FWDX_SHIFT) == E).all() and np.abs(j).max() < DOMINANT
    (k, a, b), forbid = _dominant_slot(L, q)
    j[k, a, b] = DOMINANT
    return j, forbid


# digit patterns with borrow chains: each entry is a scaled difference D (unit 2^-23 at jexp = 0)
EXTREME_D = [
    -0x808080, 0x7f7f7f, 0x1f7f7f7f7f, -0x1f80808080, 128, -129, 32768, -32769, -1, 127, -128, 32767, -32768,
    0x7f7f7f7f, -0x80808080, 2 ** 37 - 2 ** 14 - 1, -(2 ** 37 - 2 ** 14 - 1), 0x0180, -0x8000 + 128,
]


def model_extremes(L, q, seed):
    """max|J| = M, the float32 below 2^14 (jexp = 0).  The last state of the last pair holds J(q-1, q-1) = +M against
    J(q-1, 0) = -M: |D| = 2^38 - 2^14, the largest a model can produce.  The EXTREME_D patterns (digits -128 and +127,
    borrow chains, negative D) are written, as pairs (A, B) = (J(a, b), J(a, 0)), over the last pair from its last state
    downwards and again from the start of the model; everything else is 0.1 normal on the 2^-20 grid."""
    j = model_general(L, q, seed + 1).astype(F32)
    M = np.nextafter(F32(16384.0), F32(0.0))
    npair = L * (L - 1) // 2
    slots = [(k, a, b) for k in (npair - 1, 0) for a in range(q - 1, -1, -1) for b in range(q - 1, 0, -1)]
    j[npair - 1, q - 1, q - 1], j[npair - 1, q - 1, 0] = M, -M
    j[npair - 1, 0, q - 1] = -M                      # the same difference in the row of the LAST site (J_ji(b, a) = J_ij(a, b))
    used_rows = {(npair - 1, q - 1), (npair - 1, 0)}
    want = {}
    it = iter(EXTREME_D * 2)
    for (k, a, b) in slots:
        if (k, a) in used_rows:
            continue
        try:
            D = next(it)
        except StopIteration:
            break
        used_rows.add((k, a))                 # one pattern per row: J(a, 0) belongs to the whole row
        A, B = split_difference(D)
        j[k, a, b], j[k, a, 0] = A, B
        want[(k, a, b)] = D
    want[(npair - 1, q - 1, q - 1)] = 2 ** 38 - 2 ** 14
    return j, want


def model_scale_edge(L, q, kind, seed):
    """max|J| at the edges of k_scale_from_max"""
    rng = np.random.default_rng(seed)
    npair = L * (L - 1) // 2
    if kind == "zero":
        return np.zeros((npair, q, q), dtype=F32)
    if kind == "single":
        j = np.zeros((npair, q, q), dtype=F32)
        j[npair - 1, q - 1, q - 1] = F32(0.3)
        return j
    if kind == "tiny":                               # max|J| = 2^-120: 14 + 119 = 133 clamps to 100; one unit is 2^-123
        k = rng.integers(-8, 9, size=(npair, q, q))
        j = np.ldexp(k.astype(F64), -123).astype(F32)
        j[0, 0, min(1, q - 1)] = F32(2.0 ** -120)
        return j
    top = {"pow2": F32(0.25), "below_pow2": np.nextafter(F32(0.25), F32(0.0))}[kind]
    j = np.clip(model_general(L, q, seed) * F32(0.5), -0.1875, 0.1875).astype(F32)      # 2^-21 grid, below the top entry
    j[npair - 1, 0, q - 1] = top
    return j


def model_plain(L, q, seed):
    """couplings k 2^-(B-1) with |k| < 2^(B-1), B = 23 - ceil(log2(L - 1)) (22 at L = 2): differences of up to B bits, of
    which the hi f16 plane holds 11, and sums over the L - 1 neighbours below 2^24 units"""
    rng = np.random.default_rng(seed)
    B = 22 if L == 2 else 23 - int(math.ceil(math.log2(L - 1)))
    k = rng.integers(-2 ** (B - 1) + 1, 2 ** (B - 1), size=(L * (L - 1) // 2, q, q))
    return np.ldexp(k.astype(F64), -(B - 1)).astype(F32)


# ------------------------------------------------------------------------------------------------ shared case lists
# (L, N, q): the cross of L in {2, 15, 16, 17, 31, 32, 33, 47, 65}, N in {1, 31, 257} and q in {4, 5, 20, 21, 32} + the
# padded alphabets 7 and 13, thinned so that every value of each axis and every pair (L at a tile edge, large N) appears
FWD_SHAPES = [(2, 1, 4), (2, 31, 21), (15, 31, 5), (16, 257, 20), (17, 31, 21), (17, 257, 4), (31, 1, 32), (32, 31, 7),
              (33, 257, 21), (33, 1, 5), (47, 31, 13), (47, 257, 20), (65, 257, 21), (65, 31, 32)]
PLANE_PAIRS = (0, 1, 2, 3)                                               # lower plane of (0,1), (1,2), (2,3), (3,4)
SCALE_EDGES = ("pow2", "below_pow2", "tiny", "zero", "single")


def forward_cases():
    """(name, kind, L, N, q, arg) of every forward case; forward_case() builds it"""
    out = []
    for (L, N, q) in FWD_SHAPES:
        out.append(("general-L%d-N%d-q%d" % (L, N, q), "general", L, N, q, None))
        out.append(("plain-L%d-N%d-q%d" % (L, N, q), "plain", L, N, q, None))
    for n, (L, N, q) in enumerate([(2, 31, 21), (17, 257, 4), (33, 257, 21), (47, 31, 13), (65, 31, 32), (16, 257, 20),
                                   (15, 31, 5), (32, 31, 7)]):
        p = PLANE_PAIRS[n % 4]
        out.append(("planes%d%d-L%d-N%d-q%d" % (p, p + 1, L, N, q), "planes", L, N, q, p))
    for (L, N, q) in [(2, 31, 4), (17, 31, 21), (33, 257, 5), (47, 31, 13), (65, 31, 32), (16, 257, 20)]:
        out.append(("extremes-L%d-N%d-q%d" % (L, N, q), "extremes", L, N, q, None))
    for n, kind in enumerate(SCALE_EDGES):
        for (L, N, q) in [(17, 31, 21), (33, 257, 7)] if n % 2 == 0 else [(2, 1, 4), (47, 31, 20)]:
            out.append(("scale-%s-L%d-N%d-q%d" % (kind, L, N, q), "scale", L, N, q, kind))
    return out


def forward_case(case):
    """-> (seqs, jij, accurate_only): plain cases run both kernels, all others the accurate one"""
    name, kind, L, N, q, arg = case
    seed = sum(ord(c) * (n + 1) for n, c in enumerate(name)) % (2 ** 31)
    rng = np.random.default_rng(seed)
    forbid = ()
    if kind == "general":
        jij = model_general(L, q, seed)
    elif kind == "plain":
        jij = model_plain(L, q, seed)
    elif kind == "planes":
        jij, forbid = model_planes(L, q, arg, seed)
    elif kind == "extremes":
        jij, _ = model_extremes(L, q, seed)
    else:
        jij = model_scale_edge(L, q, arg, seed)
    seqs = _sequences(rng, N, L, q, forbid)
    return seqs, jij


# backward: q = 21 (both backward kernels), L so that column tiles end inside a tile of 9 fragments
BWD_L = (2, 17, 33, 47)
BWD_Q = 21
WMAX = 0.7


def backward_case(family, L, gap, N=None, q=BWD_Q):
    """-> (msa, w, astar).  Family "a": one sequence per cell, N <= q, x_sj = (s + c_j) mod q, weights wmax u 2^-(s mod 13)
    with u in [0.5, 1] (sequence 0: wmax).  Family "b": N in {130, 257, 700}; sequence 0 has weight wmax and consists of
    the reserved state q - 1 that no other sequence holds; the other weights are at most 2^-9 wmax."""
    rng = np.random.default_rng(1000 * L + 10 * (N or 0) + gap)
    if family == "a":
        N = q if N is None else N
        assert N <= q
        c = rng.integers(0, q, size=L)
        msa = ((np.arange(N)[:, None] + c[None, :]) % q).astype(np.int8)
        w = (WMAX * rng.uniform(0.5, 1.0, N) * 2.0 ** -(np.arange(N) % 13)).astype(F32)
        w[0] = F32(WMAX)
    else:
        msa = rng.integers(0, q - 1, size=(N, L)).astype(np.int8)
        msa[0, :] = q - 1
        w = (WMAX * 2.0 ** -9 * rng.uniform(0.05, 1.0, N)).astype(F32)
        w[0] = F32(WMAX)
    astar = rng.integers(1, q, size=L)
    return msa, w, astar


BWD_B_N = {2: 130, 17: 257, 33: 700, 47: 257}        # family b: N per L (every N of {130, 257, 700} appears)
OTHER_Q = (4, 5, 7, 20, 32)                         # family a at L = 17 on the other alphabets (7 runs padded as 20)
HEADROOM_L, HEADROOM_Q = 17, 21
HEADROOM_N = (130816, 131328)                        # nst128 = 1022 (one K range of the largest size) / 1026 (two)
