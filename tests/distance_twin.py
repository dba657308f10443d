"""
numpy twins of the residue distance kernels (include/plm_hip.h, "residue distance maps"): no GPU, float64 throughout.

    d2(a, b)  = (dx dx + dy dy) + dz dz        every difference, product and sum one numpy operation, so rounded once
    dist(i,j) = min(1e6, sqrt(min d2))         np.sqrt is correctly rounded

A minimum does not depend on the order of its arguments, so this twin and the kernels must agree to the bit whatever
the launch plan.  The aggregation twin is the reference's recipe spelled out: every map placed into its own NaN-filled
layer of an explicit (S, M_i, M_j) stack, nanmin over the layers, and the number of layers that hold a value.
"""
import warnings

import numpy as np

LARGE_DIST = 1e6


def d2_rows(atoms_i, coords_j):
    """(len(atoms_i), len(coords_j)) squared distances in the fixed order"""
    d = atoms_i[:, None, :] - coords_j[None, :, :]
    s = d * d
    return (s[:, :, 0] + s[:, :, 1]) + s[:, :, 2]


def _column_min(v, ranges_j):
    """minimum of the vector v (one value per atom of axis j) over every range; +inf for an empty one"""
    first, last = ranges_j[:, 0].astype(np.int64), ranges_j[:, 1].astype(np.int64)
    n = last - first + 1
    k = int(n[0]) if len(n) else 0
    if k >= 1 and (n == k).all() and (first == first[0] + k * np.arange(len(n))).all():   # equal adjacent ranges
        return v[first[0]:first[0] + k * len(n)].reshape(len(n), k).min(axis=1)
    out = np.full(len(n), np.inf)
    for j in range(len(n)):
        if n[j] >= 1:
            out[j] = v[first[j]:last[j] + 1].min()
    return out


def residue_distances(coords_i, ranges_i, coords_j=None, ranges_j=None):
    """The twin of plm.residue_distances.  The symmetric call (axis j None) is the unsymmetric call on the same chain
    twice: d2(a, b) and d2(b, a) are the same sums of the same squares, so that matrix is symmetric by itself."""
    coords_i = np.asarray(coords_i, dtype=np.float64).reshape(-1, 3)
    ranges_i = np.asarray(ranges_i).reshape(-1, 2)
    if coords_j is None:
        coords_j, ranges_j = coords_i, ranges_i
    coords_j = np.asarray(coords_j, dtype=np.float64).reshape(-1, 3)
    ranges_j = np.asarray(ranges_j).reshape(-1, 2).astype(np.int64)
    used = ranges_j[ranges_j[:, 1] >= ranges_j[:, 0]]
    if len(used):                                    # only the span of atoms that axis j names
        lo, hi = int(used[:, 0].min()), int(used[:, 1].max())
        coords_j, ranges_j = coords_j[lo:hi + 1], ranges_j - lo
    m = np.full((len(ranges_i), len(ranges_j)), np.inf)
    for i, (first, last) in enumerate(ranges_i.tolist()):
        if last >= first:
            m[i] = _column_min(d2_rows(coords_i[first:last + 1], coords_j).min(axis=0), ranges_j)
    return np.minimum(LARGE_DIST, np.sqrt(m))


def aggregate_distance_maps(coords, ranges, chain_offsets, slots_i, maps, m_i, slots_j=None, m_j=None):
    """The twin of plm.aggregate_distance_maps: (agg, count) from an explicit stack of the S maps."""
    coords = np.asarray(coords, dtype=np.float64).reshape(-1, 3)
    ranges = np.asarray(ranges).reshape(-1, 2)
    off = np.asarray(chain_offsets)
    slots_i = np.asarray(slots_i)
    slots_j = slots_i if slots_j is None else np.asarray(slots_j)
    m_j = m_i if m_j is None else m_j
    maps = np.asarray(maps).reshape(-1, 2)
    stack = np.full((len(maps), m_i, m_j), np.nan)
    cache = {}
    for s, (a, b) in enumerate(maps.tolist()):
        if (a, b) not in cache:
            cache[(a, b)] = residue_distances(coords, ranges[off[a]:off[a + 1]], coords, ranges[off[b]:off[b + 1]])
        d = cache[(a, b)]
        si, sj = slots_i[off[a]:off[a + 1]], slots_j[off[b]:off[b + 1]]
        ri, rj = np.where(si >= 0)[0], np.where(sj >= 0)[0]
        stack[s][np.ix_(si[ri], sj[rj])] = d[np.ix_(ri, rj)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # all-NaN cells
        agg = np.nanmin(stack, axis=0)
    return agg, (~np.isnan(stack)).sum(axis=0).astype(np.int32)
