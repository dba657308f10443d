"""
Numpy twin of the pairwise identities and the greedy redundancy filter (include/plm_hip.h, plm_cross_identities /
plm_redundancy_filter): the definitions written out by broadcasting, the rational tie rule in Python integers, the
filter as a plain loop.  Test oracle only; quadratic memory, small shapes.
"""
import math

import numpy as np

DENOMS = ("columns", "both", "shorter")


def pair_counts(a, b, gap_state=None, block=64):
    """m [n_a, n_b] matching columns (with a gap state: a column where either row has the gap is no match), both
    [n_a, n_b] columns where neither row has the gap (L without a gap state), residues of every row of a and of b."""
    a, b = np.asarray(a, np.int16), np.asarray(b, np.int16)
    n_a, L = a.shape
    m = np.zeros((n_a, b.shape[0]), np.int64)
    both = np.full((n_a, b.shape[0]), L, np.int64)
    ga = (a == gap_state) if gap_state is not None else np.zeros(a.shape, bool)
    gb = (b == gap_state) if gap_state is not None else np.zeros(b.shape, bool)
    for s0 in range(0, n_a, block):      # blocks of rows of a: bounds the broadcast temporaries
        sl = slice(s0, s0 + block)
        ok = ~ga[sl, None, :] & ~gb[None, :, :]
        m[sl] = ((a[sl, None, :] == b[None, :, :]) & ok).sum(axis=2)
        both[sl] = ok.sum(axis=2)
    return m, both, (~ga).sum(axis=1).astype(np.int64), (~gb).sum(axis=1).astype(np.int64)


def denominators(both, res_a, res_b, L, denominator):
    if denominator == "columns":
        return np.full(both.shape, L, np.int64)
    if denominator == "both":
        return both
    if denominator == "shorter":
        return np.minimum(res_a[:, None], res_b[None, :])
    raise ValueError(denominator)


def similarity(m, d, L, threshold, denominator):
    """columns: m >= ceil(threshold L - 1e-9), the threshold of the reweighting; both / shorter: d > 0 and
    m >= ceil(threshold d - 1e-9)."""
    if denominator == "columns":
        return m >= int(math.ceil(threshold * float(L) - 1e-9))
    return (d > 0) & (m >= np.ceil(threshold * d.astype(np.float64) - 1e-9))


def cross_identities(a, b, threshold=0.8, gap_state=None, denominator="columns", exclude_self=False):
    """Twin of plm.cross_identities: dict of int32 arrays best_index, best_match, best_denom, n_within."""
    if denominator != "columns" and gap_state is None:
        raise ValueError("both / shorter need a gap state")
    a, b = np.asarray(a), np.asarray(b)
    L = a.shape[1]
    m, both, res_a, res_b = pair_counts(a, b, gap_state)
    d = denominators(both, res_a, res_b, L, denominator)
    sim = similarity(m, d, L, threshold, denominator)
    n_a, n_b = m.shape
    rows = np.arange(n_a)
    bi, bm, bd = np.full(n_a, -1, np.int64), np.zeros(n_a, np.int64), np.zeros(n_a, np.int64)
    cnt = np.zeros(n_a, np.int64)
    for t in range(n_b):     # ascending t, every row of a at once; the products stay far below 2^63
        ok = rows != t if exclude_self else np.ones(n_a, bool)
        cnt += ok & sim[:, t]
        mm, dd = m[:, t], d[:, t]
        # largest m / d exactly, d = 0 as identity 0; strictly larger only: ties stay with the smallest index
        better = ok & ((bi < 0) | (mm * np.maximum(bd, 1) > bm * np.maximum(dd, 1)))
        bi[better], bm[better], bd[better] = t, mm[better], dd[better]
    return dict(best_index=bi.astype(np.int32), best_match=bm.astype(np.int32), best_denom=bd.astype(np.int32),
                n_within=cnt.astype(np.int32))


def similarity_matrix(msa, threshold, gap_state=None, denominator="columns"):
    msa = np.asarray(msa)
    m, both, res, _ = pair_counts(msa, msa, gap_state)
    d = denominators(both, res, res, msa.shape[1], denominator)
    return similarity(m, d, msa.shape[1], threshold, denominator)


def greedy_filter(sim):
    """keep[0] = True; keep[s] iff no kept t < s is similar to s -- the sequential definition."""
    n = sim.shape[0]
    keep = np.zeros(n, bool)
    for s in range(n):
        keep[s] = not (sim[s, :s] & keep[:s]).any()
    return keep


def redundancy_filter(msa, threshold, gap_state=None, denominator="columns"):
    return greedy_filter(similarity_matrix(msa, threshold, gap_state, denominator))


def planted_families(n, L, q, seed, gap_state=None, threshold=0.8, n_families=None):
    """n rows of L states below q: random ancestors with descendants at mutation rates that put identities on both
    sides of `threshold`, plus exact duplicates, a descendant with exactly ceil(threshold L) columns in common with
    its ancestor, gap runs and (with a gap state) a row of only gaps."""
    rng = np.random.default_rng(seed)
    fams = n_families or max(1, n // 8)
    anc = rng.integers(0, q, size=(fams, L))
    rates = np.array([0.0, 0.05, 1 - threshold - 0.03, 1 - threshold + 0.03, 0.5])
    rows = np.empty((n, L), np.int64)
    for s in range(n):
        base = anc[s % fams]
        rate = rates[rng.integers(len(rates))]
        mut = rng.random(L) < rate
        # a mutated site always changes its state, so the identity to the ancestor is exactly the unmutated share
        rows[s] = np.where(mut, (base + rng.integers(1, max(q, 2), size=L)) % q, base)
    if n > fams + 1:        # exactly at the threshold: ceil(threshold L) unchanged columns
        need = int(math.ceil(threshold * L - 1e-9))
        s = fams + 1
        rows[s] = anc[s % fams]
        change = rng.permutation(L)[:L - need]
        rows[s, change] = (rows[s, change] + 1) % q
    if gap_state is not None:
        gaps = rng.random((n, L)) < 0.08
        rows[gaps] = gap_state
        if n > 3:
            rows[n - 2] = gap_state     # a row of only gaps
    if n > 5:
        rows[n - 1] = rows[1]           # exact duplicates: the nearest neighbour is the smallest index
        rows[n // 2] = rows[1]
    return rows.astype(np.int8)
