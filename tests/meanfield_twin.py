"""
Stage-by-stage references for the mean-field DCA path (csrc/plm_meanfield.hip), plain numpy, no GPU.  Built on
oracle/meanfield_ref.py: the covariance matrix is the oracle's own expression, the DI iteration is the oracle's own
loop (observed through its `trace` hook).  What is added here is what the oracle cannot say:
  * the inverse in extended precision, so that a float64 inverse can be judged by its own rounding error and not by
    its distance to another float64 inverse;
  * how far two backward-stable float64 routes (LU, Cholesky) are from that inverse -- the yardstick for a third;
  * the summation bound of the fields;
  * which pairs of a DI input pass so close to the stop threshold that the iteration count depends on rounding.
Also the inputs shared by tests/test_meanfield_twin_host.py and tests/test_gpu_meanfield.py (shapes, seeds, generators).
"""
import numpy as np

from oracle import meanfield_ref

LD = np.longdouble
STOP = 1e-4                 # the iteration's stop threshold (meanfield_ref.direct_information)
AMBIGUOUS = 1e-10           # a diff this close to STOP can fall on either side under another summation order
LD_DIRECT_MAX = 160         # largest n whose residual is formed by a plain longdouble product (numpy has no BLAS there)


# ---------------------------------------------------------------- covariance
def covariance(fi, fij_pairs, pc):
    """C[(i,a),(j,b)] = rf_ij(a,b) - rf_i(a) rf_j(b), a, b < q-1: n x n float64, as meanfield_ref.mean_field forms it"""
    fi = np.asarray(fi, dtype=np.float64)
    L, q = fi.shape
    rfi, rfij = meanfield_ref.regularize(
        fi, meanfield_ref.dense_pair_frequencies(fi, np.asarray(fij_pairs, dtype=np.float64)), pc)
    n = L * (q - 1)
    C = (rfij[:, :, :q - 1, :q - 1] - rfi[:, None, :q - 1, None] * rfi[None, :, None, :q - 1])
    return C.transpose(0, 2, 1, 3).reshape(n, n)


def couplings_from_inverse(Cinv, L, q):
    """-C^-1 as dense L x L x q x q with a zero last row / column in every block (dtype of Cinv)"""
    J = np.zeros((L, L, q, q), dtype=Cinv.dtype)
    J[:, :, :q - 1, :q - 1] = -Cinv.reshape(L, q - 1, L, q - 1).transpose(0, 2, 1, 3)
    return J


# ---------------------------------------------------------------- extended-precision inverse
def _int_slices(A, axis, beta, count):
    """A (float64) = sum_s I_s * 2^(e - beta*s) along `axis`'s lines + a remainder below 2^(e - beta*count - 1):
    I_s integer-valued float64 with |I_s| <= 2^beta, e the exponent of the line's largest entry.  Every step is exact."""
    amax = np.abs(A).max(axis=axis, keepdims=True)
    e = np.frexp(np.where(amax > 0, amax, 1.0))[1]            # |A| < 2^e on the line
    rem = A.copy()
    out = []
    for s in range(1, count + 1):
        I = np.rint(np.ldexp(rem, beta * s - e))
        out.append(I)
        rem = rem - np.ldexp(I, e - beta * s)
    return out, e


def _exact_product(C, X):
    """C @ X for float64 C, X with an error of about 2^-64 of the result, in float64 BLAS calls: both factors are cut
    into integer slices so short that every slice product is exact in float64 whatever the summation order
    (2 beta + log2 n <= 53, the Ozaki scheme); the slice products are added in longdouble, smallest first."""
    n = C.shape[1]
    beta = (53 - int(np.ceil(np.log2(max(n, 2))))) // 2
    assert n * 4.0 ** beta <= 2.0 ** 53                        # n products of two slices: every partial sum is exact
    count = -(-80 // beta)                                     # slices down to 2^-80 of the line's largest entry
    Cs, ec = _int_slices(C, 1, beta, count)
    Xs, ex = _int_slices(X, 0, beta, count)
    pairs = [(s, t) for s in range(count) for t in range(count) if beta * (s + t) < 80]
    acc = np.zeros((C.shape[0], X.shape[1]), LD)
    for s, t in sorted(pairs, key=lambda p: -(p[0] + p[1])):
        acc += np.ldexp((Cs[s] @ Xs[t]).astype(LD), (ec - beta * (s + 1)) + (ex - beta * (t + 1)))
    return acc


def residual(C, X):
    """I - C X in longdouble for float64 C and float64 X"""
    n = C.shape[0]
    CX = C.astype(LD) @ X.astype(LD) if n <= LD_DIRECT_MAX else _exact_product(C, X)
    return np.eye(n, dtype=LD) - CX


def inverse_extended(C, info=None):
    """C^-1 in longdouble: numpy.linalg.inv(C), then Newton-Schulz steps X <- X + X (I - C X) until max|I - C X| stops
    falling (two steps, ending near 2e-17).  info, if a dict, receives the residual before every step.
    Up to n = LD_DIRECT_MAX this is done as written, in longdouble products.  numpy has no BLAS for longdouble (4 s per
    product at n = 1000), so above that X is held as X0 + S, X0 the float64 start and S the accumulated correction:
    the residual of the start, R0 = I - C X0, is the one product that needs extended precision (_exact_product);
    R = R0 - C S and the update X R involve S and R only, which are 1e-11 of X and of I, and are taken in float64 (their
    rounding is 2^-53 of 1e-11).  The residuals recorded on this route are those of the recurrence: they stop
    meaning anything below the 2^-64 of R0 itself, and the loop stops there."""
    C = np.asarray(C, dtype=np.float64)
    n = C.shape[0]
    X0 = np.linalg.inv(C)
    history = []
    if n <= LD_DIRECT_MAX:
        Cl, X, eye = C.astype(LD), X0.astype(LD), np.eye(n, dtype=LD)
        R = eye - Cl @ X
        while True:
            history.append(float(np.abs(R).max()))
            X_new = X + X @ R
            R_new = eye - Cl @ X_new
            if not float(np.abs(R_new).max()) < history[-1]:
                break
            X, R = X_new, R_new
    else:
        R0 = residual(C, X0)
        S, R = np.zeros((n, n)), R0
        while True:
            history.append(float(np.abs(R).max()))
            if history[-1] < 2.0 ** -64:
                break
            R64 = R.astype(np.float64)
            S_new = S + X0 @ R64 + (S @ R64 if S.any() else 0.0)
            R_new = R0 - (C @ S_new).astype(LD)
            if not float(np.abs(R_new).max()) < history[-1]:
                break
            S, R = S_new, R_new
        X = X0.astype(LD) + S.astype(LD)
    if info is not None:
        info["residuals"] = history
    return X


def inverse_errors(C, ext=None):
    """(err_lu, err_chol): max-abs error of numpy.linalg.inv(C) and of the float64 Cholesky route (Li = inv(cholesky(C)),
    Li.T @ Li) against inverse_extended(C), relative to max|C^-1|.  The yardstick for any other float64 inverse."""
    C = np.asarray(C, dtype=np.float64)
    ext = inverse_extended(C) if ext is None else ext
    scale = np.abs(ext).max()
    lu = np.linalg.inv(C)
    Li = np.linalg.inv(np.linalg.cholesky(C))
    chol = Li.T @ Li
    return float(np.abs(lu - ext).max() / scale), float(np.abs(chol - ext).max() / scale)


def inverse_bound(err_lu, err_chol):
    """what a float64 inverse may be off by, relative to max|C^-1|: two backward-stable float64 routes differ from
    each other by up to 8.4x in either direction (LU against Cholesky, n = 240), a third summation order gets 10x"""
    return 10.0 * max(err_lu, err_chol, 2.0 ** -52)


# ---------------------------------------------------------------- fields
def fields_from(J_full, rfi):
    """h_i(a) = log(rf_i(a) / rf_i(q-1)) - sum_{j != i, b} J_ij(a,b) rf_j(b) summed in longdouble, returned as float64,
    and the summation bound B[i,a] = sum_{j != i, b} |J_ij(a,b)| rf_j(b)"""
    J = np.asarray(J_full, dtype=np.float64)
    rfi = np.asarray(rfi, dtype=np.float64)
    L = rfi.shape[0]
    off = (~np.eye(L, dtype=bool))[:, :, None, None]
    s = np.einsum("ijab,jb->ia", (J * off).astype(LD), rfi.astype(LD))
    B = np.einsum("ijab,jb->ia", np.abs(J * off), rfi)
    h = log_term(rfi).astype(LD) - s
    return h.astype(np.float64), B


def log_term(rfi):
    return np.log(rfi / rfi[:, -1:])


def fields_bound(B, rfi, n):
    """|h_gpu - h| <= 4 n 2^-53 B + 4 2^-53 |log term|: the bound of a length-n float64 sum in any order"""
    return 4.0 * n * 2.0 ** -53 * B + 4.0 * 2.0 ** -53 * np.abs(log_term(rfi))


# ---------------------------------------------------------------- direct information
def direct_information_traced(J, rfi):
    """meanfield_ref.direct_information(J, rfi) -> (di, iterations [L,L], gap [L,L]): for every pair i < j (mirrored)
    the number of updates its fixed-point iteration took and the smallest |diff - 1e-4| it met on the way"""
    rfi = np.asarray(rfi, dtype=np.float64)
    L = rfi.shape[0]
    iters = np.zeros((L, L), np.int64)
    gap = np.full((L, L), np.inf)

    def trace(i, j, diff):
        iters[i, j] += 1
        iters[j, i] += 1
        if np.isfinite(diff):
            gap[i, j] = gap[j, i] = min(gap[i, j], abs(diff - STOP))

    di = meanfield_ref.direct_information(np.asarray(J, dtype=np.float64), rfi, trace=trace)
    return di, iters, gap


def ambiguous_pairs(gap):
    """pairs whose diff passed within AMBIGUOUS of the stop threshold: they may stop one update earlier or later"""
    i, j = np.nonzero(np.triu(gap < AMBIGUOUS, 1))
    return list(zip(i.tolist(), j.tolist()))


# ---------------------------------------------------------------- shared inputs
THETA = 0.9
# (q, L, N): n = L (q-1) against the 64-wide block columns of the inverse
GEOMETRY_CASES = [
    (2, 2, 64),         # n = 2     one block, identity tail of 62
    (21, 3, 200),       # n = 60    one block
    (32, 2, 300),       # n = 62    one block
    (4, 21, 200),       # n = 63    one block
    (2, 64, 300),       # n = 64    one block, no tail
    (5, 16, 300),       # n = 64    one block, no tail
    (6, 13, 300),       # n = 65    two blocks, tail 63
    (2, 127, 400),      # n = 127   two blocks
    (5, 32, 300),       # n = 128   two blocks, no tail
    (4, 43, 300),       # n = 129   three blocks
    (32, 5, 400),       # n = 155   three blocks
    (21, 100, 400),     # n = 2000  32 blocks
]
CONDITIONING_CASES = [(q, L, N, pc) for (q, L, N) in [(21, 12, 60), (5, 30, 300)] for pc in (0.5, 0.05, 0.01)]
OPTIONS_CASE = (5, 16, 300)
# Where the oracle itself, on the CPU's couplings, does not rank the exact copy first.  These are the strongly coupled
# cases (max|J| of 95 to 3 800 against 5 to 76 elsewhere): the fixed-point iteration of a planted pair creeps (2e4 to
# 8e4 updates) and stops at its 1e-4 rule well before the two-site marginals match, so the DI it reports is not the
# converged one and the 10 %-shuffled copy or a chance pair of a 60-sequence alignment comes out above the exact copy.
# At (21, 12, 60, 0.01) the oracle's exp(J) overflows on both planted pairs and their DI is NaN.  That ranking is an
# accident of the stop rule and nothing is asserted about it: in these cases the tests ask that the top pair be the
# oracle's top pair, and elsewhere also that it be the exact copy.
ORACLE_COPY_NOT_ON_TOP = {(32, 5, 400, 0.5), (21, 12, 60, 0.05), (21, 12, 60, 0.01), (5, 30, 300, 0.05),
                          (5, 30, 300, 0.01)}
DI_OVERFLOWS = {(21, 12, 60, 0.01)}
# k_mf_di gives up after this many updates of a pair; the oracle's loop has no such cap.  The longest loop of the
# inputs used here is about 8e4 updates, so every DI test asserts that its oracle run stayed below the cap: past it
# the kernel and the oracle would differ by design.
DI_UPDATE_CAP = 100000
DI_MODEL_CASES = [(2, 2), (2, 40), (3, 7), (21, 40), (32, 2), (32, 17)]


def case_seed(q, L, N=0):
    return 1000003 * q + 1009 * L + N


def planted_pairs(L):
    """columns of the exact copy and of the 10 %-shuffled copy (None where L has no room for a second pair)"""
    return (0, L - 1), ((1, L - 2) if L >= 4 else None)


def planted_msa(q, L, N, seed=None):
    """uniform random states; column L-1 an exact copy of column 0; column L-2 a copy of column 1 with its values
    permuted among 10 % of the rows (L >= 4)"""
    rng = np.random.default_rng(case_seed(q, L, N) if seed is None else seed)
    msa = rng.integers(0, q, size=(N, L)).astype(np.int8)
    (a, b), second = planted_pairs(L)
    msa[:, b] = msa[:, a]
    if second is not None:
        c, d = second
        msa[:, d] = msa[:, c]
        rows = rng.choice(N, size=max(2, N // 10), replace=False)
        msa[rows, d] = msa[rng.permutation(rows), d]
    return msa


def random_di_model(q, L, seed=None, strong=8.0):
    """dense couplings with every entry of every block from N(0, 1) (no gauge: last rows / columns are not zero),
    J[j,i] = J[i,j].T, +strong on the block diagonal of one pair; random strictly positive normalised frequencies.
    -> J [L,L,q,q], rfi [L,q], the strong pair (i, j)"""
    rng = np.random.default_rng(case_seed(q, L) if seed is None else seed)
    J = rng.normal(size=(L, L, q, q))
    iu, ju = np.triu_indices(L, 1)
    J[ju, iu] = J[iu, ju].transpose(0, 2, 1)
    i, j = (0, L - 1) if L > 2 else (0, 1)
    J[i, j] += strong * np.eye(q)
    J[j, i] = J[i, j].T
    rfi = rng.random(size=(L, q)) + 0.05
    rfi /= rfi.sum(axis=1, keepdims=True)
    return J, rfi, (i, j)


def overflowing_di_model(q=5, L=6, seed=77):
    """random_di_model with +800 on one entry of the block of pair (1, 4): exp overflows there and nowhere else"""
    J, rfi, _ = random_di_model(q, L, seed)
    J[1, 4, 0, 1] += 800.0
    J[4, 1] = J[1, 4].T
    return J, rfi, (1, 4)
