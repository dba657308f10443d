"""numpy twin of the three-site statistics (include/plm_hip.h, "three-site counts, frequencies and connected
correlations"): the weight quantisation, integer counts, integer marginals, and f, C, norm2, maxabs, argmax in float64.
The oracle of tests/test_triplet_host.py and tests/test_gpu_triplets.py; written from the definitions, not from the
kernels."""
import math

import numpy as np

from evcouplings_amd.plm import triplet_index


def quantise(weights, n):
    """-> (wq int64 [n], W as a Python int).  weights=None: all ones."""
    if weights is None:
        return np.ones(n, np.int64), int(n)
    w = np.asarray(weights, dtype=np.float32).astype(np.float64)
    if w.shape != (n,) or not np.isfinite(w).all() or (w < 0).any() or not (w > 0).any():
        raise ValueError("weights must be n finite non-negative values, not all zero")
    e = 30
    while math.ldexp(float(w.max()), e) > 2.0 ** 30:
        e -= 1
    wq = np.array([int(np.rint(math.ldexp(float(x), e))) for x in w], dtype=np.int64)   # rint: ties to even, as llrint
    W = int(sum(int(x) for x in wq))
    if W == 0:
        raise ValueError("W = 0")
    return wq, W


def counts(msa, q, triplet, wq):
    """count_ijk [q,q,q] as int64 (exact: W < 2^63)."""
    msa = np.asarray(msa).astype(np.int64)
    i, j, k = (int(x) for x in triplet)
    flat = (msa[:, i] * q + msa[:, j]) * q + msa[:, k]
    out = np.zeros(q * q * q, np.int64)
    np.add.at(out, flat, wq)
    return out.reshape(q, q, q)


def connected(cnt, W):
    """-> (freq, C) float64 [q,q,q] from the integer counts; the marginals are integer sums."""
    Wf = float(W)
    f3 = cnt.astype(np.float64) / Wf
    fij, fik, fjk = (cnt.sum(axis=ax).astype(np.float64) / Wf for ax in (2, 1, 0))
    fi, fj, fk = (cnt.sum(axis=ax).astype(np.float64) / Wf for ax in ((1, 2), (0, 2), (0, 1)))
    C = (f3 - fij[:, :, None] * fk[None, None, :] - fik[:, None, :] * fj[None, :, None]
         - fjk[None, :, :] * fi[:, None, None] + 2.0 * fi[:, None, None] * fj[None, :, None] * fk[None, None, :])
    return f3, C


def admissible(q, skip_state):
    m = np.ones((q, q, q), bool)
    if skip_state is not None and skip_state >= 0:
        m[skip_state, :, :] = m[:, skip_state, :] = m[:, :, skip_state] = False
    return m


def reductions(C, skip_state=None):
    """-> (norm2, maxabs, argmax flat cell) over the admissible cells."""
    q = C.shape[0]
    m = admissible(q, skip_state)
    a = np.where(m, np.abs(C), -1.0)
    return float((C[m] ** 2).sum()), float(a.max()), int(a.argmax())


def triplet_stats(msa, q, triplets, weights=None):
    msa = np.asarray(msa)
    wq, W = quantise(weights, msa.shape[0])
    trip = np.asarray(triplets, np.int64).reshape(-1, 3)
    cnt = np.stack([counts(msa, q, t, wq) for t in trip])
    fc = [connected(c, W) for c in cnt]
    return {"counts": cnt, "freq": np.stack([f for f, _ in fc]), "connected": np.stack([c for _, c in fc]), "total": W}


def triplet_scan_multi(msa, q, weights=None, sites=None, skips=(None,), probes=None):
    """The scan for several skip states in one loop over triplet_index, one triplet at a time:
    -> (triplets, {skip: (norm2, maxabs, argmax flat cell, probed)}).  probes: None or {skip: one flat cell per
    triplet}; probed[t] = |C_t[probes[skip][t]]| (how good somebody else's argmax is)."""
    msa = np.asarray(msa)
    wq, W = quantise(weights, msa.shape[0])
    trip = triplet_index(msa.shape[1] if sites is None else sites)
    T = len(trip)
    out = {s: (np.zeros(T), np.zeros(T), np.zeros(T, np.int64), np.zeros(T)) for s in skips}
    for t, ijk in enumerate(trip):
        _, C = connected(counts(msa, q, ijk, wq), W)
        for s in skips:
            out[s][0][t], out[s][1][t], out[s][2][t] = reductions(C, s)
            if probes is not None:
                out[s][3][t] = abs(C.reshape(-1)[int(probes[s][t])])
    return trip, out


def triplet_scan(msa, q, weights=None, sites=None, skip_state=None, probe=None):
    """-> (triplets, norm2, maxabs, argmax flat cell, probed) for one skip state."""
    trip, out = triplet_scan_multi(msa, q, weights, sites, (skip_state,), None if probe is None else {skip_state: probe})
    return (trip,) + out[skip_state]
