"""
Numpy twin of the last stage of an evaluation: what turns the backward GEMM's integer sums into the gradient and the
objective value (k_pair_norms, k_assemble / k_assemble_v, k_assemble_h, the reg_part partials and k_finish_fx in
evcouplings_amd/csrc/plm_kernels.hip), written from the formulas of include/plm_hip.h (plm_problem_t: lambda_h,
lambda_j, lambda_group, PLM_GROUP_DELTA) and the kernels' comments -- numpy only, no GPU and no library call.

The data part of an evaluation (the integer sums times gscale) does not depend on the regulariser strengths, so the
twin models the regulariser alone, exactly as the kernels form it:

  couplings   g = fmaf(gscale, v1 + v2, p),  p = fl32(fl32(2 lambda_j + gcoef) x),  gcoef = fl32(lambda_g / gnorm) or 0
              gnorm = fl32(sqrt(fl32(n2) + fl32(delta^2))),  n2 = the f64 sum of squares of the block (k_pair_norms)
  fields      g = fmaf(gscale, v, p),        p = fl32(fl32(2 lambda_h) x)
  value       fx - nll = lambda_h sum h^2 + lambda_j sum J^2 + lambda_g sum_{i<j} gnorm_ij in f64, the strengths
              rounded to float32 first (the kernels receive them as `float`)

reg_gradient() returns p in np.float32 arithmetic: for lambda_g = 0 bit for bit what the kernels add before the single
rounding of the fused multiply-add; with lambda_g > 0 up to the last bits of n2 (summed in another order), sqrtf and the
division.  reg_coefficients() returns the float32 factor in front of x, whose product with x is exact in float64: that
is how tests/test_assemble_twin_host.py ties the twin to the f64 oracle without the twin's own last rounding.

The vector layout everywhere is the canonical one of include/plm_hip.h: [L qm fields | pairs qm qm couplings], pairs
i < j row-major, qm the number of MODEL states (q, or q - 1 with ignore_gaps).  The raw vector of plm_ctx_get_g keeps all
q states in gap mode; raw_structural_zeros() marks the entries of that vector no parameter owns.  (States >= Qc of a
padded alphabet exist in the kernels' native layout only: the canonical vector has no place for them, so at this
boundary they can show only as a wrong live entry.)

MUTANTS are deliberately wrong twins; the host test shows that each of them breaks the comparison the right twin passes.
"""
import numpy as np

F32, F64 = np.float32, np.float64
GROUP_DELTA = 1e-4                                   # PLM_GROUP_DELTA
DELTA2_F32 = F32(GROUP_DELTA * GROUP_DELTA)          # (float)(PLM_GROUP_DELTA * PLM_GROUP_DELTA)
TINY_NORM = 2e-3                                     # blocks below this Frobenius norm are the "tiny" ones of cases()
MUTANTS = ("lambda_not_doubled", "group_counted_qm_times", "delta_omitted")


# ------------------------------------------------------------------------------------------------ layout
def n_params(L, qm):
    return L * qm + L * (L - 1) // 2 * qm * qm


def n_pairs(L):
    return L * (L - 1) // 2


def fields_of(x, L, qm):
    return np.asarray(x)[:L * qm].reshape(L, qm)


def couplings_of(x, L, qm):
    return np.asarray(x)[L * qm:].reshape(n_pairs(L), qm, qm)


def pair_sites(L):
    """(i, j) of every pair block in canonical order"""
    return np.triu_indices(L, 1)


def pair_of_entry(L, qm):
    """the pair block every COUPLING entry of the canonical vector belongs to (length pairs qm qm)"""
    return np.repeat(np.arange(n_pairs(L)), qm * qm)


def embed_gaps(x, L, q):
    """(q-1)-state vector -> the raw q-state vector with zeros where state 0 takes part"""
    x = np.asarray(x)
    out = np.zeros(n_params(L, q), dtype=x.dtype)
    fields_of(out, L, q)[:, 1:] = fields_of(x, L, q - 1)
    couplings_of(out, L, q)[:, 1:, 1:] = couplings_of(x, L, q - 1)
    return out


def strip_gaps(x, L, q):
    """raw q-state vector -> the (q-1)-state vector of the model"""
    return np.concatenate([fields_of(x, L, q)[:, 1:].ravel(), couplings_of(x, L, q)[:, 1:, 1:].ravel()])


def raw_structural_zeros(L, q, gap):
    """mask over the raw q-state canonical vector: entries no parameter owns (gap mode: every entry with state 0 in it)"""
    m = np.zeros(n_params(L, q), dtype=bool)
    if gap:
        fields_of(m, L, q)[:, 0] = True
        couplings_of(m, L, q)[:, 0, :] = True
        couplings_of(m, L, q)[:, :, 0] = True
    return m


def ulp32(a):
    """spacing of float32 at |a| (towards larger magnitudes) as float64: a correctly rounded float32 result r is within
    ulp32(r) / 2 of the exact value"""
    return np.spacing(np.abs(np.asarray(a)).astype(F32)).astype(F64)


# ------------------------------------------------------------------------------------------------ the regulariser
def block_norms(x, L, qm, mutant=None):
    """(n2, gnorm) per pair block in float32: n2 = fl32(f64 sum of squares), gnorm = fl32(sqrt(n2 + fl32(delta^2)))"""
    J = couplings_of(x, L, qm).astype(F64).reshape(n_pairs(L), qm * qm)
    n2 = (J * J).sum(axis=1).astype(F32)
    gnorm = np.sqrt((n2 + DELTA2_F32).astype(F32)).astype(F32)
    if mutant == "delta_omitted":
        tiny = (n2 > 0) & (n2 < F32(TINY_NORM * TINY_NORM))
        gnorm = np.where(tiny, np.sqrt(n2).astype(F32), gnorm)
    return n2, gnorm


def reg_parts(x, L, qm, lambda_h, lambda_j, lambda_g, mutant=None):
    """(field part, coupling L2 part, group part) of fx - nll in float64"""
    x = np.asarray(x, dtype=F32)
    h = fields_of(x, L, qm).astype(F64)
    J = couplings_of(x, L, qm).astype(F64)
    lh, lj, lg = F64(F32(lambda_h)), F64(F32(lambda_j)), F64(F32(lambda_g))
    group = 0.0
    if lg > 0:
        _, gnorm = block_norms(x, L, qm, mutant)
        group = float(lg * gnorm.astype(F64).sum())
        if mutant == "group_counted_qm_times":
            group *= qm
    return float(lh * (h * h).sum()), float(lj * (J * J).sum()), group


def reg_value(x, L, qm, lambda_h, lambda_j, lambda_g, mutant=None):
    """the float64 value fx - nll must have"""
    return float(sum(reg_parts(x, L, qm, lambda_h, lambda_j, lambda_g, mutant)))


def reg_coefficients(x, L, qm, lambda_h, lambda_j, lambda_g, mutant=None):
    """the float32 factor c of every entry with p = fl32(c x): 2 lambda_h on fields, fl32(2 lambda_j + gcoef) on couplings"""
    x = np.asarray(x, dtype=F32)
    two = F32(1.0) if mutant == "lambda_not_doubled" else F32(2.0)
    c = np.empty(x.shape, dtype=F32)
    c[:L * qm] = two * F32(lambda_h)
    if F32(lambda_g) > 0:
        _, gnorm = block_norms(x, L, qm, mutant)
        gcoef = (F32(lambda_g) / gnorm).astype(F32)
    else:
        gcoef = np.zeros(n_pairs(L), dtype=F32)
    c[L * qm:] = np.repeat((two * F32(lambda_j) + gcoef).astype(F32), qm * qm)
    return c


def reg_gradient(x, L, qm, lambda_h, lambda_j, lambda_g, mutant=None):
    """p: the float32 the kernels add to the data part inside the fused multiply-add"""
    x = np.asarray(x, dtype=F32)
    p = reg_coefficients(x, L, qm, lambda_h, lambda_j, lambda_g, mutant) * x
    assert p.dtype == F32
    return p


def value_terms(L, qm):
    """number of float64 additions behind fx - nll: one per parameter and one per pair block"""
    return n_params(L, qm) + n_pairs(L)


# ------------------------------------------------------------------------------------------------ shared cases
N_SEQS = 130                                        # not a multiple of 64
SITES = (2, 16, 17, 33)                             # one diagonal block / a block edge / one over / three blocks, ragged
ALPHABETS = ((21, False), (21, True), (20, False), (5, False), (32, False), (7, False), (27, False))   # 7, 27: padded
SETTINGS = ((0.0, 0.0, 0.0), (0.01, 1.7, 0.0), (0.3, 40.0, 0.0), (0.01, 1.7, 7.5), (0.01, 0.0, 7.5))
PAIRS = ((1, 0), (2, 0), (3, 0), (4, 0), (1, 2))    # indices into SETTINGS: every setting against zero, and 1 against 2
BIG = 3.0


def cases():
    """(name, L, q, gap) of every case"""
    return [("L%d-q%d%s" % (L, q, "-gaps" if gap else ""), L, q, gap) for L in SITES for (q, gap) in ALPHABETS]


def case_seed(case):
    return sum(ord(c) * (n + 1) for n, c in enumerate(case[0])) % (2 ** 31)


def case_alignment(case, N=N_SEQS):
    """N sequences over 0..q-1: mutated copies of eight ancestors (so that the cluster weights differ), 5 % of state 0"""
    _, L, q, _ = case
    rng = np.random.default_rng(case_seed(case))
    anc = rng.integers(0, q, size=(8, L))
    msa = anc[rng.integers(0, 8, size=N)]
    fresh = rng.integers(0, q, size=(N, L))
    msa = np.where(rng.random((N, L)) < rng.uniform(0.0, 0.6, size=(N, 1)), fresh, msa)
    msa[rng.random((N, L)) < 0.05] = 0
    return np.ascontiguousarray(msa, dtype=np.int8)


def model_x(L, qm, seed, plant_max_in_block_pairs=False):
    """-> (x, kind): N(0, 1) fields and N(0, 0.1) couplings; kind[pair] = 0 for a block that is exactly zero (a third of
    them), 1 for a block scaled to a Frobenius norm of 10^U(-5, -3) (a tenth, around delta = 1e-4), 2 for the rest, a few
    entries of which are +-3.  plant_max_in_block_pairs: one entry of 3 in every pair of 16-site blocks, so that every
    shard of a sharded-state context sees the same max|J|."""
    rng = np.random.default_rng(seed + 17)
    npair = n_pairs(L)
    h = rng.normal(0.0, 1.0, size=(L, qm))
    J = rng.normal(0.0, 0.1, size=(npair, qm, qm))
    kind = np.full(npair, 2, dtype=np.int8)
    order = rng.permutation(npair)
    nzero = npair // 3
    ntiny = max(1, npair // 10) if npair >= 10 else 0
    kind[order[:nzero]] = 0
    kind[order[nzero:nzero + ntiny]] = 1
    iu, ju = pair_sites(L)
    if plant_max_in_block_pairs:
        for I in range((L + 15) // 16):
            for Jb in range(I, (L + 15) // 16):
                i, j = 16 * I, 16 * Jb + 1
                assert i < j < L
                k = int(np.flatnonzero((iu == i) & (ju == j))[0])
                kind[k] = 2
    J[kind == 0] = 0.0
    for k in np.flatnonzero(kind == 1):
        J[k] *= 10.0 ** rng.uniform(-5.0, -3.0) / np.sqrt((J[k] ** 2).sum())
    normal = np.flatnonzero(kind == 2)
    for k in normal[rng.permutation(normal.size)[:6]]:
        J[k, rng.integers(0, qm), rng.integers(0, qm)] = BIG * rng.choice([-1.0, 1.0])
    if plant_max_in_block_pairs:
        for I in range((L + 15) // 16):
            for Jb in range(I, (L + 15) // 16):
                k = int(np.flatnonzero((iu == 16 * I) & (ju == 16 * Jb + 1))[0])
                J[k, qm - 1, qm // 2] = BIG
    x = np.concatenate([h.ravel(), J.ravel()]).astype(F32)
    assert np.abs(x[L * qm:]).max() <= BIG
    return x, kind


def case_x(case):
    _, L, q, gap = case
    return model_x(L, q - 1 if gap else q, case_seed(case))


def live_coupling_entries(L, qm, kind):
    """mask over the coupling entries: those of blocks that are not exactly zero (p = 0 on the others)"""
    return np.repeat(kind != 0, qm * qm)


def gradient_bound(gA, gB, pA, pB, settingA, settingB):
    """the bound of the differencing test for every entry: |(gA - gB) - (pA - pB)| <= ulp32(gA) / 2 + ulp32(gB) / 2 -- each
    gradient is ONE rounding of data + p, the data part being the same exact product in both -- plus 4 ulp32(p) for a
    context with lambda_g > 0 (n2 summed in another order and rounded, sqrtf, the division: the build has no -ffast-math)"""
    b = 0.5 * ulp32(gA) + 0.5 * ulp32(gB)
    if settingA[2] > 0:
        b = b + 4.0 * ulp32(pA)
    if settingB[2] > 0:
        b = b + 4.0 * ulp32(pB)
    return b
