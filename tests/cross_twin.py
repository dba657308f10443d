"""numpy float64 twin of plm_cross_energies (include/plm_hip.h, inter-protein energies): the two sums in the contract's
order -- j ascending into V, then i ascending into E -- vectorised over the rows (s, t), so that the library's results
can be compared bit for bit; the error bound for sums taken in another order; a brute-force assignment for tiny groups."""
import itertools

import numpy as np

BEST = np.dtype([("index", np.int64), ("best", np.float64), ("second", np.float64)])


def potentials(jab, seqs_b, skip_state=None):
    """V[t][i][a] = sum_j (double) jab[i][j][a][b_tj], j ascending, from +0.0; a skipped b_tj adds nothing"""
    jab = np.asarray(jab, np.float32)
    seqs_b = np.asarray(seqs_b).astype(np.int64)
    LA, LB, q, _ = jab.shape
    V = np.zeros((seqs_b.shape[0], LA, q))
    for j in range(LB):
        b = seqs_b[:, j]
        term = jab[:, j][:, :, b].astype(np.float64).transpose(2, 0, 1)          # (n_b, LA, q)
        if skip_state is None:
            V += term
        else:
            keep = b != skip_state
            V[keep] += term[keep]
    return V


def table(jab, seqs_a, seqs_b, skip_state=None):
    """E[s][t] = sum_i V[t][i][a_si], i ascending, from +0.0; a skipped a_si adds nothing"""
    seqs_a = np.asarray(seqs_a).astype(np.int64)
    V = potentials(jab, seqs_b, skip_state)
    E = np.zeros((seqs_a.shape[0], V.shape[0]))
    for i in range(seqs_a.shape[1]):
        a = seqs_a[:, i]
        term = V[:, i, :][:, a].T                                                 # (n_a, n_b)
        if skip_state is None:
            E += term
        else:
            keep = a != skip_state
            E[keep] += term[keep]
    return E


def best_of(E, axis_offset, transpose=False):
    """(index, best, second) of every row of E (of every column with transpose): ties to the smallest index, second the
    largest value over the other partners; indices are shifted by axis_offset"""
    E = E.T if transpose else E
    out = np.empty(E.shape[0], BEST)
    out["index"], out["best"], out["second"] = -1, -np.inf, -np.inf
    if E.shape[1] == 0:
        return out
    k = np.argmax(E, axis=1)                      # numpy's argmax returns the first of equal maxima
    out["index"] = k + axis_offset
    out["best"] = E[np.arange(E.shape[0]), k]
    if E.shape[1] > 1:
        rest = E.copy()
        rest[np.arange(E.shape[0]), k] = -np.inf
        out["second"] = rest.max(axis=1)
    return out


def block_offsets(a_offsets, b_offsets):
    ao, bo = np.asarray(a_offsets, np.int64), np.asarray(b_offsets, np.int64)
    return np.concatenate([[0], np.cumsum(np.diff(ao) * np.diff(bo))]).astype(np.int64)


def cross_energies(jab, seqs_a, seqs_b, a_offsets=None, b_offsets=None, skip_state=None, matrix=True, best=True, device=0):
    """the twin of plm.cross_energies, same arguments, same dict"""
    jab = np.asarray(jab, np.float32)
    seqs_a = np.asarray(seqs_a, np.int8).reshape(-1, jab.shape[0])
    seqs_b = np.asarray(seqs_b, np.int8).reshape(-1, jab.shape[1])
    n_a, n_b = len(seqs_a), len(seqs_b)
    if a_offsets is None:
        a_offsets, b_offsets = [0, n_a], [0, n_b]
    ao, bo = np.asarray(a_offsets, np.int64), np.asarray(b_offsets, np.int64)
    off = block_offsets(ao, bo)
    m = np.empty(int(off[-1]))
    rows, cols = np.empty(n_a, BEST), np.empty(n_b, BEST)
    V = potentials(jab, seqs_b, skip_state) if n_b else np.zeros((0,) + jab.shape[:1] + jab.shape[2:3])
    for g in range(len(ao) - 1):
        a0, a1, b0, b1 = ao[g], ao[g + 1], bo[g], bo[g + 1]
        E = np.zeros((a1 - a0, b1 - b0))
        for i in range(jab.shape[0]):
            a = seqs_a[a0:a1, i].astype(np.int64)
            term = V[b0:b1, i, :][:, a].T
            if skip_state is None:
                E += term
            else:
                keep = a != skip_state
                E[keep] += term[keep]
        m[off[g]:off[g + 1]] = E.ravel()
        rows[a0:a1] = best_of(E, b0)
        cols[b0:b1] = best_of(E, a0, transpose=True)
    return dict(matrix=m if matrix else None, block_offsets=off, rows_best=rows if best else None,
                cols_best=cols if best else None)


def bound(n_terms, sum_abs):
    """2 n_terms 2^-53 sum|value|: what two float64 sums of the same n_terms values may differ by, whatever their orders
    (the bound of mutants_twin)"""
    return 2.0 * np.asarray(n_terms) * 2.0 ** -53 * np.asarray(sum_abs)


def sum_abs(jab, seqs_a, seqs_b):
    """sum over (i, j) of |jab[i][j][a_si][b_tj]| for every (s, t), float64, for `bound`"""
    return table(np.abs(np.asarray(jab, np.float32)), seqs_a, seqs_b)


def brute_assignment(E, maximize=True):
    """the best assignment of min(n, m) pairs of a tiny n x m table by trying every one: (partner_of_row, total)"""
    E = np.asarray(E, np.float64)
    n, m = E.shape
    best_total, best_partner = None, np.full(n, -1, np.int64)
    if n == 0 or m == 0:
        return best_partner, 0.0
    if n <= m:
        candidates = (dict(zip(range(n), cols)) for cols in itertools.permutations(range(m), n))
    else:
        candidates = (dict(zip(rows, range(m))) for rows in itertools.permutations(range(n), m))
    for cand in candidates:
        total = sum(E[r, c] for r, c in cand.items())
        if best_total is None or (total > best_total if maximize else total < best_total):
            best_total, best = total, cand
    for r, c in best.items():
        best_partner[r] = c
    return best_partner, float(best_total)


def model_from_inter(jab):
    """a model-file style dict of L_A + L_B sites whose inter blocks are jab (sites of A first) and whose other blocks are 0"""
    jab = np.asarray(jab, np.float32)
    LA, LB, q, _ = jab.shape
    L = LA + LB
    jij = np.zeros((L * (L - 1) // 2, q, q), np.float32)
    for i in range(LA):
        for j in range(LB):
            jij[i * (2 * L - i - 1) // 2 + (LA + j - i - 1)] = jab[i, j]
    return dict(L=L, q=q, jij=jij, hi=np.zeros((L, q), np.float32), index_list=np.arange(1, L + 1, dtype=np.int32),
                alphabet="-ACDEFGHIKLMNPQRSTVWY"[:q])


def planted_case(seed, LA=8, LB=6, q=21, n_species=12, n_paralogs=5):
    """Uniform random sequences in true pairs (row k of A with row k of B before the shuffle); jab = the one-hot
    co-occurrence counts of the true pairs minus their block mean plus 0.05 N(0,1), float32; the B rows of every species
    shuffled.  Returns a dict: model, jab, a, b, species_a, species_b, ids_a, ids_b, truth {id_1: id_2}."""
    rng = np.random.default_rng(seed)
    n = n_species * n_paralogs
    a = rng.integers(0, q, (n, LA)).astype(np.int8)
    b = rng.integers(0, q, (n, LB)).astype(np.int8)
    counts = np.zeros((LA, LB, q, q))
    for s in range(n):
        counts[np.arange(LA)[:, None], np.arange(LB)[None, :], a[s][:, None], b[s][None, :]] += 1.0
    jab = (counts - counts.mean(axis=(2, 3), keepdims=True) + 0.05 * rng.normal(size=counts.shape)).astype(np.float32)
    species = np.repeat(["sp%02d" % k for k in range(n_species)], n_paralogs)
    ids_a = np.array(["a%03d" % k for k in range(n)])
    ids_b = np.array(["b%03d" % k for k in range(n)])
    order = np.concatenate([g * n_paralogs + rng.permutation(n_paralogs) for g in range(n_species)])
    return dict(model=model_from_inter(jab), jab=jab, a=a, b=b[order], species_a=species, species_b=species[order],
                ids_a=ids_a, ids_b=ids_b[order], truth=dict(zip(ids_a, ids_b)), sites_a=np.arange(LA),
                sites_b=np.arange(LA, LA + LB))
