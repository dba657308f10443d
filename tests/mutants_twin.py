"""
numpy float64 twin of plm_mutant_effects / plm_mutant_scan (DESIGN_NEXT_ROWS.md section 9.16): the arithmetic of the
issue, restated per variant with plain loops.

    S_h[i,a]  = h_i(a) - h_i(t_i)            S_J[i,a] = sum_{j != i} ( J_ij(a, t_j) - J_ij(t_i, t_j) )
    E_ij(a,b) = J_ij(a,b) - J_ij(a,t_j) - J_ij(t_i,b) + J_ij(t_i,t_j)
    dH_h = sum_m S_h[i_m,a_m]     dH_J = sum_m S_J[i_m,a_m] + sum_{m<n} E(i_m,i_n; a_m,a_n)     dH = dH_J + dH_h

Beside the three energies every variant carries `n_terms` and `sum_abs`: the count and the absolute sum of all h and J
values that enter.  Any float64 summation of those (exactly representable, float32) values, in any order and grouping, is
within (n_terms - 1) 2^-53 sum_abs of the exact sum to first order, so two such summations differ by at most
    bound = 2 n_terms 2^-53 sum_abs.
"""
import itertools

import numpy as np

OK, ETOOMANY, EPOSITION, ESTATE, EREPEAT = 0, 1, 2, 3, 4


def dense(hi, jij, q):
    """(h [L, q], J [L, L, q, q]) in float64 from float32 fields and i<j blocks; J[j, i] = J[i, j].T, zero diagonal."""
    h = np.asarray(hi, np.float32).astype(np.float64)
    L = h.shape[0]
    blocks = np.asarray(jij, np.float32).astype(np.float64).reshape(L * (L - 1) // 2, q, q)
    J = np.zeros((L, L, q, q))
    iu, ju = np.triu_indices(L, 1)
    J[iu, ju] = blocks
    J[ju, iu] = blocks.transpose(0, 2, 1)
    return h, J


def delta(target, h, J, pos, sub):
    """((dH, dH_J, dH_h), n_terms, sum_abs) of one valid variant."""
    L = h.shape[0]
    t = target
    dh = dj = sum_abs = 0.0
    n_terms = 0
    M = len(pos)
    for m in range(M):
        i, a = int(pos[m]), int(sub[m])
        dh += h[i, a] - h[i, t[i]]
        sum_abs += abs(h[i, a]) + abs(h[i, t[i]])
        n_terms += 2
        for j in range(L):
            if j != i:
                dj += J[i, j, a, t[j]] - J[i, j, t[i], t[j]]
                sum_abs += abs(J[i, j, a, t[j]]) + abs(J[i, j, t[i], t[j]])
                n_terms += 2
    for m in range(M):
        i, a = int(pos[m]), int(sub[m])
        for n in range(m + 1, M):
            j, b = int(pos[n]), int(sub[n])
            terms = (J[i, j, a, b], J[i, j, a, t[j]], J[i, j, t[i], b], J[i, j, t[i], t[j]])
            dj += terms[0] - terms[1] - terms[2] + terms[3]
            sum_abs += sum(abs(v) for v in terms)
            n_terms += 4
    return (dj + dh, dj, dh), n_terms, sum_abs


def status_of(L, q, pos, sub):
    pos, sub = np.asarray(pos, np.int64), np.asarray(sub, np.int64)
    if len(pos) > L:
        return ETOOMANY
    if ((pos < 0) | (pos >= L)).any():
        return EPOSITION
    if ((sub < 0) | (sub >= q)).any():
        return ESTATE
    if len(set(pos.tolist())) != len(pos):
        return EREPEAT
    return OK


def mutant_effects(target, q, hi, jij, offsets, positions, states, device=0, tables=False, info=False):
    """plm.mutant_effects; with info=True (out, status, n_terms, sum_abs)."""
    h, J = dense(hi, jij, q)
    L = h.shape[0]
    target = np.asarray(target).ravel().astype(np.int64)
    offsets = np.asarray(offsets, np.int64)
    n = len(offsets) - 1
    out, status = np.full((n, 3), np.nan), np.zeros(n, np.uint8)
    n_terms, sum_abs = np.zeros(n, np.int64), np.zeros(n)
    for v in range(n):
        pos, sub = positions[offsets[v]:offsets[v + 1]], states[offsets[v]:offsets[v + 1]]
        status[v] = status_of(L, q, pos, sub)
        if status[v] == OK:
            out[v], n_terms[v], sum_abs[v] = delta(target, h, J, pos, sub)
    if info:
        return out, status, n_terms, sum_abs
    if tables:
        return out, status, single_tables(target, q, hi, jij)
    return out, status


def bound(n_terms, sum_abs):
    return 2.0 * np.asarray(n_terms, np.float64) * 2.0 ** -53 * np.asarray(sum_abs, np.float64)


def single_tables(target, q, hi, jij):
    """L x q x 2 (S_J, S_h)."""
    h, J = dense(hi, jij, q)
    L = h.shape[0]
    target = np.asarray(target).ravel().astype(np.int64)
    tab = np.zeros((L, q, 2))
    for i in range(L):
        for a in range(q):
            (_, dj, dh), _, _ = delta(target, h, J, [i], [a])
            tab[i, a] = dj, dh
    return tab


def csr(variants):
    """[(positions, states), ...] -> (offsets int64, positions int32, states int8)"""
    offsets = np.zeros(len(variants) + 1, np.int64)
    offsets[1:] = np.cumsum([len(p) for p, _ in variants])
    positions = np.array([x for p, _ in variants for x in p], np.int32)
    states = np.array([x for _, s in variants for x in s], np.int8)
    return offsets, positions, states


def scan_variants(q, sites, letters=None, first=0, count=None, product_limit=1 << 20):
    """the combinations first .. first + count - 1 of itertools.product over the letter lists, as variants.  A range that
    ends beyond `product_limit` is not walked to from the start: its members are decoded from their mixed-radix index
    (the last site fastest), which is what itertools.product enumerates."""
    lists = [list(range(q))] * len(sites) if letters is None else [list(l) for l in letters]
    total = 1
    for l in lists:
        total *= len(l)
    stop = total if count is None else first + count
    if stop <= product_limit:
        combos = itertools.islice(itertools.product(*lists), first, stop)
        return [(list(sites), list(c)) for c in combos]
    out = []
    for index in range(first, stop):
        combo = []
        for l in reversed(lists):
            index, d = divmod(index, len(l))
            combo.append(l[d])
        out.append((list(sites), combo[::-1]))
    return out


def mutant_scan(target, q, hi, jij, sites, letters=None, first=0, count=None, energies=False, edges=None, threshold=None,
                capacity=1 << 16, device=0, info=False):
    """plm.mutant_scan through itertools.product over `delta`; with info=True also `n_terms` and `sum_abs`."""
    variants = scan_variants(q, sites, letters, first, count)
    sizes = [q if letters is None else len(l) for l in (letters if letters is not None else sites)]
    total = int(np.prod(sizes, dtype=object)) if len(sizes) else 1
    out, status, n_terms, sum_abs = mutant_effects(target, q, hi, jij, *csr(variants), info=True)
    assert (status == OK).all()
    n = len(variants)
    res = dict(n_combinations=total, first=first, count=n,
               dh_min=float(out[:, 0].min()) if n else np.inf, dh_max=float(out[:, 0].max()) if n else -np.inf)
    if energies:
        res["energies"] = out
    if edges is not None:
        bins = np.searchsorted(np.asarray(edges, np.float64), out[:, 0], side="right")
        res["histogram"] = np.bincount(bins, minlength=len(edges) + 1).astype(np.uint64)
    if threshold is not None:
        keep = np.nonzero(out[:, 0] >= threshold)[0]
        fits = len(keep) <= capacity
        res.update(n_kept=len(keep), kept_index=(keep + first).astype(np.int64) if fits else None,
                   kept_energies=out[keep] if fits else None)
    if info:
        res.update(n_terms=n_terms, sum_abs=sum_abs)
    return res
