"""
Python host API over the C ABI of libplm_hip.so: numpy in, numpy out.

This is the in-process replacement for what the reference obtains from the plmc child
process (evcouplings/couplings/tools.py:202-307): sequence weights, frequencies, the
fitted fields/couplings and the CN scores.  All arithmetic happens in the HIP library on
an MI355X; nothing here computes on the CPU and there is no fallback path.
"""
import ctypes as C

import numpy as np

from evcouplings_amd import _lib
from evcouplings_amd._lib import PlmProblem, PlmResult, check


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _msa(msa):
    msa = np.ascontiguousarray(msa, dtype=np.int8)
    if msa.ndim != 2:
        raise ValueError("msa must be a 2-D (N, L) int8 matrix")
    return msa


def n_params(L, q):
    return L * q + L * (L - 1) // 2 * q * q


def default_lambda_j(L, q, base=0.01):
    """lambda_J * (q-1) * (L-1), the scaling of evcouplings/couplings/protocol.py:159-179."""
    return base * (q - 1) * (L - 1)


def device_count():
    return _lib.load().plm_device_count()


# convention switches (include/plm_hip.h PLM_CONV_*): selectable conventions of plmc that cannot be verified here
CONV_THRESHOLD_F32 = 32        # App. D-1: float32 evaluation of the cluster threshold
CONV_G_GAPS_IDENTICAL = 64     # -g: gap-gap positions count as identical in reweighting
CONV_G_UNGAPPED_LENGTH = 128   # -g: threshold on the positions where both sequences are ungapped
CONV_G_FREQ_TOTAL = 256        # -g: frequencies normalised by N_eff instead of the ungapped weight
CONV_FN_NO_GAP = 512           # App. D-3: Frobenius norm without the gap state
CONV_MASK = 32 | 64 | 128 | 256 | 512


def conventions_from_env(conventions=None):
    """Explicit value, else the environment variable PLM_HIP_CONVENTIONS (an integer, e.g. "320" or "0x140"), else 0:
    lets an unmodified pipeline select conventions for the run_plmc drop-in."""
    import os
    if conventions is None:
        conventions = int(os.environ.get("PLM_HIP_CONVENTIONS", "0"), 0)
    conventions = int(conventions)
    if conventions & ~CONV_MASK:
        raise ValueError("unknown convention bits in %d (known: %d)" % (conventions, CONV_MASK))
    return conventions


def reweight(msa, theta_id=0.8, ignore_gaps=False, conventions=0):
    """Cluster sizes (incl. self) at identity >= theta_id; twin of alignment.py:1193-1233.
    ignore_gaps / conventions: plmc -g semantics and PLM_CONV_* switches.
    States are 0..123 (PLM_REWEIGHT_MAX_STATE); one column is enough."""
    lib = _lib.load()
    msa = _msa(msa)
    counts = np.zeros(msa.shape[0], dtype=np.int32)
    flags = (FLAG_IGNORE_GAPS if ignore_gaps else 0) | int(conventions)
    check(lib.plm_reweight_ex(_ptr(msa), msa.shape[0], msa.shape[1], float(theta_id), flags, _ptr(counts)))
    return counts


def marginals(msa, weights, q, pairs=True):
    """f_i (L,q) and f_ij (L(L-1)/2,q,q) for i<j; twin of alignment.py:1079-1153."""
    lib = _lib.load()
    msa = _msa(msa)
    N, L = msa.shape
    w = np.ascontiguousarray(weights, dtype=np.float32)
    fi = np.zeros((L, q), dtype=np.float32)
    fij = np.zeros((L * (L - 1) // 2, q, q), dtype=np.float32) if pairs else None
    check(lib.plm_marginals(_ptr(msa), _ptr(w), N, L, q, _ptr(fi), _ptr(fij)))
    return fi, fij


def evaluate(msa, weights, q, lambda_h, lambda_j, x):
    """Objective, its unregularised part and the gradient at x (canonical layout)."""
    lib = _lib.load()
    msa = _msa(msa)
    N, L = msa.shape
    w = np.ascontiguousarray(weights, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.size != n_params(L, q):
        raise ValueError("x has %d entries, expected %d" % (x.size, n_params(L, q)))
    g = np.zeros_like(x)
    fx, nll = C.c_double(0), C.c_double(0)
    check(lib.plm_eval(_ptr(msa), _ptr(w), N, L, q, float(lambda_h), float(lambda_j), _ptr(x),
                       C.byref(fx), C.byref(nll), _ptr(g)))
    return fx.value, nll.value, g


def scores(jij, L, q, conventions=0):
    """FN and CN (APC) matrices from i<j coupling blocks; twin of model.py:179-233, 744-827.
    conventions & CONV_FN_NO_GAP: state 0 left out of the Frobenius norm."""
    lib = _lib.load()
    jij = np.ascontiguousarray(jij, dtype=np.float32)
    fn = np.zeros((L, L), dtype=np.float32)
    cn = np.zeros((L, L), dtype=np.float32)
    check(lib.plm_scores_ex(_ptr(jij), L, q, int(conventions), _ptr(fn), _ptr(cn)))
    return fn, cn


def _canonical(hi, jij, L, q):
    """h [L][q] followed by the i<j coupling blocks [q][q]: the canonical parameter vector."""
    hi = np.ascontiguousarray(hi, dtype=np.float32).reshape(L * q)
    jij = np.ascontiguousarray(jij, dtype=np.float32).reshape(L * (L - 1) // 2 * q * q)
    return np.concatenate([hi, jij])


def _potts_model(hi, jij, q):
    """(hi, jij, L) of a model as the wrappers of the generative side take it: hi a float32 (L, q) matrix, jij float32
    with the entries of the i<j blocks; a ValueError otherwise."""
    hi = np.ascontiguousarray(hi, dtype=np.float32)
    if hi.ndim != 2 or hi.shape[1] != q or hi.shape[0] < 1:
        raise ValueError("hi must be an (L, q) matrix with q = %d" % q)
    L = hi.shape[0]
    jij = np.ascontiguousarray(jij, dtype=np.float32)
    if jij.size != L * (L - 1) // 2 * q * q:
        raise ValueError("jij has %d entries, expected the %d i<j blocks of %d x %d" % (jij.size, L * (L - 1) // 2, q, q))
    return hi, jij, L


def _chain_args(start, fixed, allowed, C_, L, q):
    """(start, fixed, allowed) as the library takes them, each None or checked in that order: C_ x L int8 states, L and q
    uint8 flags."""
    if start is not None:
        start = np.ascontiguousarray(start, dtype=np.int8)
        if start.shape != (C_, L):
            raise ValueError("start must be an (n_chains, L) = (%d, %d) matrix of states" % (C_, L))
    if fixed is not None:
        fixed = np.ascontiguousarray(np.asarray(fixed).astype(bool), dtype=np.uint8)
        if fixed.shape != (L,):
            raise ValueError("fixed must hold L = %d flags" % L)
    if allowed is not None:
        allowed = np.ascontiguousarray(np.asarray(allowed).astype(bool), dtype=np.uint8)
        if allowed.shape != (q,):
            raise ValueError("allowed must hold q = %d flags" % q)
    return start, fixed, allowed


def _progress(done, total):
    return int(done), int(total)


def _stop_callback(functype, callback, convert=_progress):
    """(cb, reraise): the ctypes callback of type functype that passes convert(the library's arguments without the user
    pointer) to callback and answers 1 (stop) for a true value, and reraise(), to be called after the library returns.
    An exception must not cross the C frames: it stops the call and reraise() raises it again.  callback None: a NULL
    function pointer."""
    failure = []

    def _cb(*args):
        try:
            return 1 if callback(*convert(*args[:-1])) else 0
        except BaseException as exc:
            failure.append(exc)
            return 1

    def reraise():
        if failure:
            raise failure[0]

    return (functype(_cb) if callback is not None else functype()), reraise


def alignment_stats(msa, gap_state=0, query=None, device=0):
    """Per-sequence gap counts, per-column gap counts and (if `query` is given) identities of every sequence to the
    query, as int32 arrays (n,), (L,), (n,) -- the raw counts behind Alignment.count(gap, axis=...) and
    identities_to_seq of evcouplings/align/alignment.py:707-747, 1157-1190."""
    lib = _lib.load()
    msa = _msa(msa)
    n, L = msa.shape
    seq_gaps, col_gaps = np.zeros(n, np.int32), np.zeros(L, np.int32)
    ident = None
    if query is not None:
        query = np.ascontiguousarray(query, dtype=np.int8).reshape(L)
        ident = np.zeros(n, np.int32)
    check(lib.plm_alignment_stats(_ptr(msa), n, L, int(gap_state), _ptr(query), _ptr(seq_gaps), _ptr(col_gaps),
                                  _ptr(ident), int(device), None))
    return seq_gaps, col_gaps, ident


def _ident_opts(threshold, gap_state, denominator, exclude_self):
    if denominator not in _lib.IDENT_DENOM:
        raise ValueError("denominator must be one of %s (got %r)" % (sorted(_lib.IDENT_DENOM), denominator))
    return _lib.PlmIdentOpts(-1 if gap_state is None else int(gap_state), _lib.IDENT_DENOM[denominator],
                             1 if exclude_self else 0, float(threshold))


def cross_identities(a, b=None, threshold=0.8, gap_state=None, denominator="columns", exclude_self=None, device=0):
    """
    For every row of `a` (n_a x L integer states 0..126) the nearest row of `b` and the number of rows of `b` within
    `threshold`; b=None compares `a` with itself, each row's own index left out (exclude_self defaults to that).
    m = matching columns (with `gap_state`, a column where either row has the gap is no match), d = the denominator:
    "columns" L, "both" the columns where neither row has the gap, "shorter" min(residues of the two rows); the last
    two need a gap state.  Similar: "columns" m >= ceil(threshold L - 1e-9) (the rule of `reweight`), otherwise d > 0
    and m >= ceil(threshold d - 1e-9).  Nearest: largest m / d compared exactly, ties to the smallest index.
    Returns a dict of int32 arrays best_index (-1 where no partner is left), best_match, best_denom, n_within, and
    identity = best_match / max(best_denom, 1) as float64.
    """
    lib = _lib.load()
    a = _msa(a)
    if exclude_self is None:
        exclude_self = b is None
    b = a if b is None else _msa(b)
    if a.shape[1] != b.shape[1]:
        raise ValueError("a has %d columns, b has %d" % (a.shape[1], b.shape[1]))
    opts = _ident_opts(threshold, gap_state, denominator, exclude_self)
    out = {k: np.zeros(a.shape[0], np.int32) for k in ("best_index", "best_match", "best_denom", "n_within")}
    check(lib.plm_cross_identities(_ptr(a), a.shape[0], _ptr(b), b.shape[0], a.shape[1], C.byref(opts),
                                   _ptr(out["best_index"]), _ptr(out["best_match"]), _ptr(out["best_denom"]),
                                   _ptr(out["n_within"]), int(device), None))
    out["identity"] = out["best_match"] / np.maximum(out["best_denom"], 1).astype(np.float64)
    return out


def redundancy_filter(msa, threshold, gap_state=None, denominator="columns", device=0):
    """
    Greedy redundancy filter in input order: row 0 is kept, row s is kept iff no kept earlier row is similar to it
    (similarity as in `cross_identities`).  Returns the boolean mask of kept rows; exactly the sequential definition.
    """
    lib = _lib.load()
    msa = _msa(msa)
    opts = _ident_opts(threshold, gap_state, denominator, False)
    keep = np.zeros(msa.shape[0], np.uint8)
    n_kept = C.c_int32(0)
    check(lib.plm_redundancy_filter(_ptr(msa), msa.shape[0], msa.shape[1], C.byref(opts), _ptr(keep), C.byref(n_kept),
                                    int(device), None))
    return keep.astype(bool)


def triplet_index(sites_or_L):
    """The (T, 3) int32 table of every i < j < k among the given sites (an ascending sequence, or L for range(L)),
    lexicographic: the order of `triplet_scan`'s outputs.  Pure numpy."""
    sites = np.arange(int(sites_or_L)) if np.ndim(sites_or_L) == 0 else np.asarray(sites_or_L)
    n = len(sites)
    i, j = np.triu_indices(n, 1)                     # the pairs in row-major order; pair (i, j) has n - 1 - j values of k
    cnt = n - 1 - j
    ii, jj = np.repeat(i, cnt), np.repeat(j, cnt)
    kk = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt) + jj + 1
    return np.stack([sites[ii], sites[jj], sites[kk]], axis=1).astype(np.int32).reshape(-1, 3)


def _triplet_args(msa, weights, skip_state, want):
    msa = _msa(msa)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
    if w is not None and w.shape != (msa.shape[0],):
        raise ValueError("weights must hold one value per sequence (%d), got shape %s" % (msa.shape[0], w.shape))
    return msa, w, _lib.PlmTripletOpts(-1 if skip_state is None else int(skip_state), int(want))


def triplet_stats(msa, q, triplets, weights=None, skip_state=None, counts=False, freq=True, connected=True, device=0):
    """
    Three-site statistics of the listed triplets (T x 3, i < j < k) of an alignment (N x L states 0..q-1): a dict with
    `total` (W, the sum of the fixed-point weights; N for weights=None), `triplets`, and as asked `counts` (T,q,q,q)
    uint64 -- exact integers --, `freq` = counts / W and `connected` = f_ijk - f_ij f_k - f_ik f_j - f_jk f_i
    + 2 f_i f_j f_k, both float64.  `weights`: N non-negative floats, quantised to integers as include/plm_hip.h states.
    """
    lib = _lib.load()
    want = (_lib.TRIPLET_COUNTS if counts else 0) | (_lib.TRIPLET_FREQ if freq else 0) | \
        (_lib.TRIPLET_CONNECTED if connected else 0)
    msa, w, opts = _triplet_args(msa, weights, skip_state, want)
    trip = np.ascontiguousarray(triplets, dtype=np.int32).reshape(-1, 3)
    shape = (len(trip), q, q, q) if 2 <= q <= 32 else (0,)
    out = {"triplets": trip,
           "counts": np.zeros(shape, np.uint64) if counts else None,
           "freq": np.zeros(shape, np.float64) if freq else None,
           "connected": np.zeros(shape, np.float64) if connected else None}
    total = C.c_uint64(0)
    check(lib.plm_triplet_stats(_ptr(msa), _ptr(w), msa.shape[0], msa.shape[1], int(q), _ptr(trip), len(trip),
                                C.byref(opts), _ptr(out["counts"]), _ptr(out["freq"]), _ptr(out["connected"]),
                                C.byref(total), int(device), None))
    out["total"] = int(total.value)
    return {k: v for k, v in out.items() if v is not None}


def triplet_scan(msa, q, weights=None, sites=None, skip_state=None, device=0, with_total=False):
    """
    Connected three-site correlations of every triplet i < j < k among `sites` (strictly ascending; None = all):
    returns (triplets (T,3) int32 in the order of `triplet_index`, norm2 (T,) = sum C^2, maxabs (T,) = max |C|,
    argmax_abc (T,3) the states of a cell that attains it), norm2 / maxabs / argmax over the cells that do not involve
    `skip_state`.  with_total: W is appended.
    """
    lib = _lib.load()
    msa, w, opts = _triplet_args(msa, weights, skip_state, 0)
    L = msa.shape[1]
    sel = None if sites is None else np.ascontiguousarray(sites, dtype=np.int32).reshape(-1)
    n_sel = L if sel is None else len(sel)
    ascending = sel is None or (len(sel) and (np.diff(sel) > 0).all() and sel[0] >= 0 and sel[-1] < L)
    T = n_sel * (n_sel - 1) * (n_sel - 2) // 6 if (ascending and 3 <= n_sel <= 2345) else 0
    norm2, maxabs, arg = np.zeros(T, np.float64), np.zeros(T, np.float64), np.zeros(T, np.int32)
    total = C.c_uint64(0)
    check(lib.plm_triplet_scan(_ptr(msa), _ptr(w), msa.shape[0], L, int(q), _ptr(sel), n_sel, C.byref(opts),
                               _ptr(norm2), _ptr(maxabs), _ptr(arg), C.byref(total), int(device), None))
    abc = np.stack([arg // (q * q), arg // q % q, arg % q], axis=1).astype(np.int32)
    out = (triplet_index(L if sel is None else sel), norm2, maxabs, abc)
    return out + (int(total.value),) if with_total else out


PCA_STATUS = {_lib.STATUS_CONVERGED: "converged", _lib.STATUS_MAXITER: "maxiter", _lib.STATUS_INTERRUPTED: "interrupted"}


def pca_fit(msa, q, k=2, weights=None, skip_state=None, oversample=8, max_iter=500, tol=1e-10, seed=0, scores=False,
            device=0, callback=None):
    """
    The k leading principal components of the centred one-hot features of an alignment (N x L states 0..q-1), by block
    subspace iteration on the GPU; the covariance is never formed (include/plm_hip.h states the definitions).  `weights`:
    N non-negative floats, quantised as for `triplet_stats`; `skip_state`: a state whose features are left out.
    Returns a dict: mean (L,q) = f_i(a), components (k,L,q) orthonormal with zeros at the skipped state, eigenvalues (k,)
    descending, explained = eigenvalues / total_variance, total_variance = trace of the covariance, residuals (k,) =
    |C v - lambda v|, iterations, converged (residuals <= tol lambda_1), status, total (W) and, with scores=True, scores
    (N,k), the projections of the rows themselves.  callback(iteration, largest relative residual) is called once per
    iteration; a true return value stops the fit ("interrupted").  Running out of iterations is a result, not an error.
    """
    lib = _lib.load()
    msa = _msa(msa)
    N, L = msa.shape
    q, k = int(q), int(k)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
    if w is not None and w.shape != (N,):
        raise ValueError("weights must hold one value per sequence (%d), got shape %s" % (N, w.shape))
    opts = _lib.PlmPcaOpts(k, int(oversample), int(max_iter), -1 if skip_state is None else int(skip_state), float(tol),
                           int(seed) & 0xFFFFFFFFFFFFFFFF)
    kk, qq = (k if 1 <= k <= 64 else 0), (q if 2 <= q <= 32 else 0)
    out = {"mean": np.zeros((L, qq)), "components": np.zeros((kk, L, qq)), "eigenvalues": np.zeros(kk),
           "residuals": np.zeros(kk), "scores": np.zeros((N, kk)) if scores else None}
    tv, total, its, conv, status = C.c_double(0), C.c_uint64(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    cb, reraise = _stop_callback(_lib.PCA_CB, callback, lambda it, worst: (int(it), float(worst)))
    check(lib.plm_pca_fit_cb(_ptr(msa), _ptr(w), N, L, q, C.byref(opts), _ptr(out["mean"]), _ptr(out["components"]),
                             _ptr(out["eigenvalues"]), _ptr(out["residuals"]), C.byref(tv), C.byref(total), C.byref(its),
                             C.byref(conv), _ptr(out["scores"]), int(device), None, cb, None, C.byref(status)))
    reraise()
    out.update(total_variance=tv.value, total=int(total.value), iterations=int(its.value), converged=bool(conv.value),
               status=PCA_STATUS[int(status.value)],
               explained=out["eigenvalues"] / tv.value if tv.value > 0 else np.zeros(kk))
    return {key: v for key, v in out.items() if v is not None}


def pca_project(seqs, q, mean, components, skip_state=None, device=0):
    """
    Projections (n,k) float64 of n sequences (n x L states 0..q-1) on the components (k,L,q) of `pca_fit` with its mean
    (L,q): t_c(x) = sum_i v_c[i, x_i] - sum_{i,a} mean[i,a] v_c[i,a]; a skipped state contributes 0.
    """
    lib = _lib.load()
    seqs = _msa(seqs)
    n, L = seqs.shape
    q = int(q)
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    components = np.ascontiguousarray(components, dtype=np.float64)
    if mean.shape != (L, q):
        raise ValueError("mean must be an (L, q) = (%d, %d) matrix, got shape %s" % (L, q, mean.shape))
    if components.ndim != 3 or components.shape[1:] != (L, q):
        raise ValueError("components must be (k, %d, %d), got shape %s" % (L, q, components.shape))
    k = components.shape[0]
    out = np.zeros((n, k if 1 <= k <= 64 else 0))
    check(lib.plm_pca_project(_ptr(seqs), n, L, q, _ptr(mean), _ptr(components), k, -1 if skip_state is None else int(skip_state),
                              _ptr(out), int(device), None))
    return out


def _atoms(coords, ranges, what):
    coords = np.ascontiguousarray(coords, dtype=np.float64)
    ranges = np.ascontiguousarray(ranges, dtype=np.int32)
    if coords.ndim != 2 or coords.shape[1] != 3:
        raise ValueError("coords_%s must be an (atoms, 3) matrix, got shape %s" % (what, coords.shape))
    if ranges.ndim != 2 or ranges.shape[1] != 2:
        raise ValueError("ranges_%s must be a (residues, 2) matrix, got shape %s" % (what, ranges.shape))
    return coords, ranges


def residue_distances(coords_i, ranges_i, coords_j=None, ranges_j=None, device=0):
    """
    Minimum atom-atom distance between every residue of axis i and every residue of axis j, float64 (N_i, N_j):
    coords (atoms, 3), ranges (residues, 2) = first and last atom of a residue, inclusive (ranges may overlap, skip
    atoms, or be empty with last < first).  d2 = (dx dx + dy dy) + dz dz with every operation rounded once, the minimum
    over the atom pairs, one correctly rounded square root, capped at 1e6 (also the value for a residue without
    atoms): reproducible to the bit.  coords_j = ranges_j = None: axis i against itself, exactly symmetric.
    """
    lib = _lib.load()
    ci, ri = _atoms(coords_i, ranges_i, "i")
    if (coords_j is None) != (ranges_j is None):
        raise ValueError("give both coords_j and ranges_j, or neither")
    cj, rj = (None, None) if coords_j is None else _atoms(coords_j, ranges_j, "j")
    n_j = len(ri) if rj is None else len(rj)
    out = np.zeros((len(ri), n_j), np.float64)
    check(lib.plm_residue_distances(_ptr(ci), len(ci), _ptr(ri), len(ri), _ptr(cj), 0 if cj is None else len(cj),
                                    _ptr(rj), 0 if rj is None else len(rj), _ptr(out), int(device), None))
    return out


def aggregate_distance_maps(coords, ranges, chain_offsets, slots_i, maps, m_i, slots_j=None, m_j=None, agg=True,
                            count=True, device=0):
    """
    The minimum of many residue distance maps on one pair of axes, without the stack of maps.  coords (atoms, 3) and
    ranges (residues, 2; atom indices into `coords`) hold every chain one after the other, chain c owning the residues
    chain_offsets[c] .. chain_offsets[c + 1] - 1.  slots_i / slots_j give every residue its row / column of the result
    (-1: none; slots_j = None: slots_i on both axes, m_j = None: m_i), maps (S, 2) lists (chain on axis i, chain on
    axis j).  Returns (agg, count): agg (m_i, m_j) float64, the minimum of `residue_distances` over the maps that cover
    a cell and NaN where none does; count (m_i, m_j) int32, the number of maps that cover it.  agg=False / count=False
    leaves that output out (None).
    """
    lib = _lib.load()
    coords, ranges = _atoms(coords, ranges, "of the chains")
    off = np.ascontiguousarray(chain_offsets, dtype=np.int32).reshape(-1)
    maps = np.ascontiguousarray(maps, dtype=np.int32).reshape(-1, 2)
    si = np.ascontiguousarray(slots_i, dtype=np.int32).reshape(-1)
    sj = None if slots_j is None else np.ascontiguousarray(slots_j, dtype=np.int32).reshape(-1)
    m_i = int(m_i)
    m_j = m_i if m_j is None else int(m_j)
    if len(off) < 2 or off[-1] != len(ranges) or len(si) != len(ranges) or (sj is not None and len(sj) != len(ranges)):
        raise ValueError("chain_offsets must end at the %d residues, and the slots hold one entry per residue" % len(ranges))
    shape = (max(m_i, 0), max(m_j, 0))
    a = np.zeros(shape, np.float64) if agg else None
    c = np.zeros(shape, np.int32) if count else None
    check(lib.plm_distance_maps_aggregate(_ptr(coords), len(coords), _ptr(ranges), _ptr(off), len(off) - 1, _ptr(si),
                                          _ptr(sj), m_i, m_j, _ptr(maps), len(maps), _ptr(a), _ptr(c), int(device), None))
    return a, c


def hamiltonians(seqs, q, hi, jij, device=0):
    """
    Statistical energies of sequences under a model: n x 3 float64 (H, H_J, H_h) with
    H_J = sum_{i<j} J_ij(x_i, x_j), H_h = sum_i h_i(x_i) -- the return value of the reference's
    `_hamiltonians(sequences, J_ij, h_i)` (couplings/model.py:25-60), computed by the forward one-hot GEMM.
    seqs: n x L integer states; hi: L x q; jij: the i<j blocks [L(L-1)/2][q][q].
    """
    lib = _lib.load()
    seqs = _msa(seqs)
    n, L = seqs.shape
    out = np.zeros((n, 3))
    check(lib.plm_hamiltonians(_ptr(seqs), n, L, q, _ptr(_canonical(hi, jij, L, q)), device, None, _ptr(out)))
    return out


def potentials(seqs, q, hi, jij, device=0):
    """HJ[s, i, a] = sum_{j != i} J_ij(a, x_sj): n x L x q float32 (coupling part of every conditional)."""
    lib = _lib.load()
    seqs = _msa(seqs)
    n, L = seqs.shape
    out = np.zeros((n, L, q), dtype=np.float32)
    check(lib.plm_potentials(_ptr(seqs), n, L, q, _ptr(_canonical(hi, jij, L, q)), device, None, _ptr(out)))
    return out


def sample(hi, jij, q, n_chains, burn_in=10, n_snapshots=1, thin=1, beta=1.0, seed=0, start=None, fixed=None,
           allowed=None, energies=True, device=0):
    """
    Draw sequences from P(x) ~ exp beta (sum_i h_i(x_i) + sum_{i<j} J_ij(x_i, x_j)) with the Gibbs sampler of the library
    (plm_sample, DESIGN_NEXT_ROWS.md section 9.6): n_chains independent chains, burn_in full sweeps (sites 0 .. L-1 in
    order), then n_snapshots snapshots of all chains, thin sweeps apart.
    hi: L x q; jij: the i<j blocks [L(L-1)/2][q][q] as for `hamiltonians`.  start: None (every chain starts from one draw
    per site of softmax beta h_i) or n_chains x L states; fixed: None or L flags of sites that are never resampled;
    allowed: None or q flags of the states that may be drawn.  The result depends on (seed, chain index, model, options)
    only, not on n_chains or the run.
    Returns (samples int8 [K, C, L], energies float64 [K, C, 3] = (H, H_J, H_h) at beta = 1, or None).
    """
    q, C_, K = int(q), int(n_chains), int(n_snapshots)
    hi, jij, L = _potts_model(hi, jij, q)
    if C_ < 1 or K < 1 or int(burn_in) < 0 or int(thin) < 1:
        raise ValueError("need n_chains >= 1, n_snapshots >= 1, burn_in >= 0 and thin >= 1")
    start, fixed, allowed = _chain_args(start, fixed, allowed, C_, L, q)
    lib = _lib.load()
    opts = _lib.PlmSampleOpts(C_, int(burn_in), K, int(thin), float(beta), int(seed) & 0xFFFFFFFFFFFFFFFF,
                              _ptr(start), _ptr(fixed), _ptr(allowed))
    samples = np.zeros((K, C_, L), dtype=np.int8)
    en = np.zeros((K, C_, 3)) if energies else None
    check(lib.plm_sample(L, q, _ptr(_canonical(hi, jij, L, q)), C.byref(opts), int(device), None, _ptr(samples), _ptr(en)))
    return samples, en


def _split_canonical(x, L, q):
    return x[:L * q].reshape(L, q), x[L * q:].reshape(L * (L - 1) // 2, q, q)


def ar_logprob(seqs, q, hi, jij, site_terms=False, device=0):
    """
    Exact log-probabilities under an autoregressive Potts model (plm_ar_logprob, DESIGN_NEXT_ROWS.md section 9.19):
    P(x) = prod_i softmax_b(h_i(b) + sum_{j<i} J_ji(x_j, b)) at b = x_i.  hi: L x q; jij: the i<j blocks, entry [a][b] of
    block (j, i) coupling state a of the earlier site j with state b of the later site i.
    Returns log P [n] (float64), with site_terms also the site terms [n, L] that sum to it.
    """
    q = int(q)
    hi, jij, L = _potts_model(hi, jij, q)
    seqs = _msa(seqs)
    if seqs.shape[1] != L:
        raise ValueError("the sequences have %d sites, the model %d" % (seqs.shape[1], L))
    n = seqs.shape[0]
    logp = np.zeros(n)
    site = np.zeros((n, L)) if site_terms else None
    check(_lib.load().plm_ar_logprob(_ptr(seqs), n, L, q, _ptr(_canonical(hi, jij, L, q)), int(device), None, _ptr(logp),
                                     _ptr(site)))
    return (logp, site) if site_terms else logp


def ar_sample(hi, jij, q, n, seed=0, beta=1.0, allowed=None, first_chain=0, device=0):
    """
    n independent exact samples of an autoregressive Potts model, one ancestral pass each (plm_ar_sample): int8 [n, L].
    Sample c of a call is chain first_chain + c of the seed, whatever n.  allowed: None or q flags of the states that may
    be drawn; beta: inverse temperature of every conditional.
    """
    q, n = int(q), int(n)
    hi, jij, L = _potts_model(hi, jij, q)
    _, _, allowed = _chain_args(None, None, allowed, n, L, q)
    opts = _lib.PlmArSampleOpts(n, int(first_chain) & 0xFFFFFFFF, int(seed) & 0xFFFFFFFFFFFFFFFF, float(beta), _ptr(allowed))
    out = np.zeros((max(n, 0), L), dtype=np.int8)
    check(_lib.load().plm_ar_sample(L, q, _ptr(_canonical(hi, jij, L, q)), C.byref(opts), int(device), None, _ptr(out)))
    return out


def ar_evaluate(msa, weights, q, lambda_h, lambda_j, hi, jij, device=0):
    """
    F = -(1/N_eff) sum_s w_s log P(x_s) + lambda_h sum h^2 + lambda_j sum J^2 of an autoregressive Potts model, its first
    term and the float64 gradient (plm_ar_eval).  Returns (F, nll, g_h [L, q], g_J [pairs, q, q]).
    """
    q = int(q)
    hi, jij, L = _potts_model(hi, jij, q)
    msa = _msa(msa)
    if msa.shape[1] != L:
        raise ValueError("the alignment has %d sites, the model %d" % (msa.shape[1], L))
    w = np.ascontiguousarray(weights, dtype=np.float32)
    if w.shape != (msa.shape[0],):
        raise ValueError("need one weight per sequence")
    g = np.zeros(n_params(L, q))
    fx, nll = C.c_double(0), C.c_double(0)
    check(_lib.load().plm_ar_eval(_ptr(msa), _ptr(w), msa.shape[0], L, q, float(lambda_h), float(lambda_j),
                                  _ptr(_canonical(hi, jij, L, q)), int(device), None, C.byref(fx), C.byref(nll), _ptr(g)))
    g_h, g_j = _split_canonical(g, L, q)
    return fx.value, nll.value, g_h, g_j


AR_STATUS = {_lib.STATUS_CONVERGED: "converged", _lib.STATUS_MAXITER: "maxiter", _lib.STATUS_LINESEARCH: "linesearch",
             _lib.STATUS_INTERRUPTED: "interrupted"}


def ar_fit(msa, weights, q, lambda_h, lambda_j, max_iter=1000, epsilon=1e-4, lbfgs_m=6, start=None, callback=None,
           device=0):
    """
    Fit an autoregressive Potts model to a weighted alignment by L-BFGS on the device (plm_ar_fit).  lambda_h, lambda_j:
    per-sequence units (F is normalised by N_eff).  start: None (zeros) or (hi, jij).  callback(iter, seconds, cond, fx,
    nll, |h|, |J|) is called after every iteration; a true return value stops the fit ("interrupted").
    Returns a dict: hi [L, q], jij [pairs, q, q] (float32), status (one of AR_STATUS's values), iterations, evaluations,
    ls_reason, fx, nll, gnorm, xnorm.
    """
    q = int(q)
    msa = _msa(msa)
    n, L = msa.shape
    w = np.ascontiguousarray(weights, dtype=np.float32)
    if w.shape != (n,):
        raise ValueError("need one weight per sequence")
    x0 = None
    if start is not None:
        hi, jij, Ls = _potts_model(start[0], start[1], q)
        if Ls != L:
            raise ValueError("the start point has %d sites, the alignment %d" % (Ls, L))
        x0 = _canonical(hi, jij, L, q)
    cb, reraise = _stop_callback(_lib.ITER_CB, callback, convert=lambda *a: a)
    opts = _lib.PlmArFitOpts(float(lambda_h), float(lambda_j), int(max_iter), float(epsilon), int(lbfgs_m))
    res = _lib.PlmArFitResult()
    x = np.zeros(max(n_params(L, q), 1), dtype=np.float32)
    rc = _lib.load().plm_ar_fit(_ptr(msa), _ptr(w), n, L, q, C.byref(opts), _ptr(x0), cb, None, int(device), None, _ptr(x),
                                C.byref(res))
    reraise()
    check(rc)
    hi, jij = _split_canonical(x[:n_params(L, q)], L, q)
    return {"hi": hi, "jij": jij, "status": AR_STATUS[res.status], "iterations": res.iterations,
            "evaluations": res.evaluations, "ls_reason": res.ls_reason, "fx": res.fx, "nll": res.nll, "gnorm": res.gnorm,
            "xnorm": res.xnorm}


def rbm_n_params(L, q, M):
    return L * q + M + M * L * q


def _rbm_model(g, c, W, q):
    """(params, L, M): the RBM layout g [L][q], c [M], W [M][L][q] as one float32 vector"""
    g = np.ascontiguousarray(g, dtype=np.float32)
    if g.ndim != 2 or g.shape[1] != q:
        raise ValueError("g must be an (L, %d) matrix" % q)
    L = g.shape[0]
    c = np.ascontiguousarray(c, dtype=np.float32).ravel()
    M = c.size
    W = np.ascontiguousarray(W, dtype=np.float32)
    if W.shape != (M, L, q):
        raise ValueError("W must be an (M, L, q) = (%d, %d, %d) array" % (M, L, q))
    return np.concatenate([g.ravel(), c, W.ravel()]), L, M


def _rbm_split(x, L, q, M):
    return x[:L * q].reshape(L, q), x[L * q:L * q + M], x[L * q + M:].reshape(M, L, q)


def rbm_score(seqs, q, g, c, W, inputs=False, device=0):
    """
    score(v) = sum_i g_i(v_i) + sum_mu softplus(I_mu(v)) = log P(v) + log Z of a restricted Boltzmann machine with Potts
    visible and Bernoulli hidden units (plm_rbm_score, DESIGN_NEXT_ROWS.md section 9.22), I_mu(v) = c_mu + sum_i W_mu,i(v_i).
    g: L x q; c: M; W: M x L x q.  Returns the scores [n] (float64), with inputs also the hidden-unit inputs I [n, M].
    """
    q = int(q)
    x, L, M = _rbm_model(g, c, W, q)
    seqs = _msa(seqs)
    if seqs.shape[1] != L:
        raise ValueError("the sequences have %d sites, the model %d" % (seqs.shape[1], L))
    n = seqs.shape[0]
    score = np.zeros(n)
    I = np.zeros((n, M)) if inputs else None
    check(_lib.load().plm_rbm_score(_ptr(seqs), n, L, q, M, _ptr(x), int(device), None, _ptr(score), _ptr(I)))
    return (score, I) if inputs else score


def rbm_sample(g, c, W, q, n_chains, burn_in=10, n_snapshots=1, thin=1, seed=0, start=None, fixed=None, allowed=None,
               first_step=0, first_chain=0, hidden=False, device=0):
    """
    Block Gibbs sampling of a restricted Boltzmann machine (plm_rbm_sample): n_chains independent chains, burn_in steps
    (all hidden units given the sites, then all sites given the hidden units), then n_snapshots snapshots thin steps
    apart.  start: None (one draw per site of softmax g_i) or n_chains x L states; fixed: None or L flags; allowed: None or
    q flags.  Chain c of a call is chain first_chain + c of the seed whatever n_chains, and a run continues from its last
    states with first_step = the steps made so far.
    Returns the states int8 [K, C, L], with hidden also the hidden units int8 [K, C, M] of the step before each snapshot.
    """
    q, C_, K = int(q), int(n_chains), int(n_snapshots)
    x, L, M = _rbm_model(g, c, W, q)
    start, fixed, allowed = _chain_args(start, fixed, allowed, C_, L, q)
    opts = _lib.PlmRbmSampleOpts(C_, int(burn_in), K, int(thin), int(first_step) & 0xFFFFFFFF, int(first_chain) & 0xFFFFFFFF,
                                 int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(start), _ptr(fixed), _ptr(allowed))
    states = np.zeros((max(K, 0), max(C_, 0), L), dtype=np.int8)
    hid = np.zeros((max(K, 0), max(C_, 0), M), dtype=np.int8) if hidden else None
    check(_lib.load().plm_rbm_sample(L, q, M, _ptr(x), C.byref(opts), int(device), None, _ptr(states), _ptr(hid)))
    return (states, hid) if hidden else states


RBM_STATUS = {_lib.STATUS_MAXITER: "maxiter", _lib.STATUS_INTERRUPTED: "interrupted"}


def rbm_fit(msa, weights, q, g, c, W, n_chains, n_epochs, steps_per_epoch=2, lr=0.1, lr_decay_after=0, lambda_g=0.0,
            lambda_w=0.0, seed=0, start=None, first_epoch=0, callback=None, phase_times=False, device=0):
    """
    Persistent contrastive divergence for a restricted Boltzmann machine (plm_rbm_fit): n_epochs steps of
    theta <- theta + lr_g ((D - N) - 2 lambda theta) from the start point (g, c, W), where D are the statistics of the
    weighted alignment and N those of n_chains persistent block-Gibbs chains after steps_per_epoch steps, both with the
    hidden units summed out.  lr_decay_after = T > 0: the step of global epoch e is lr T / (e + 1) once e + 1 > T.  start:
    None (the sampler's start rule) or n_chains x L states; first_epoch: the global number of the first epoch, for a call
    that continues an earlier one from its g, c, W and chains.  callback(epoch, max_dg, max_dc, max_dw, lr, data_score)
    is called once per epoch and stops the fit by returning a true value.
    Returns a dict: g, c, W (float32), data and model (the statistics of the last epoch that ran, each a (g, c, W) triple
    of float64), chains (int8 C x L), trace (one row per epoch that ran: max |D_g - N_g|, max |D_c - N_c|,
    max |D_W - N_W|, lr_g, the weighted mean score of the alignment), epochs_done (updates applied), status ("maxiter",
    "interrupted").  The result is bitwise reproducible.  phase_times: also phase_ms, the milliseconds of (data
    statistics, chain steps, model statistics and trace row, update) summed over the epochs, by device events; the
    fit then waits for the device after every epoch.
    """
    q, C_, E = int(q), int(n_chains), int(n_epochs)
    x0, L, M = _rbm_model(g, c, W, q)
    msa = _msa(msa)
    if msa.shape[1] != L:
        raise ValueError("the alignment has %d sites, the model %d" % (msa.shape[1], L))
    w = np.ascontiguousarray(weights, dtype=np.float32)
    if w.shape != (msa.shape[0],):
        raise ValueError("need one weight per sequence")
    start = _chain_args(start, None, None, C_, L, q)[0]
    opts = _lib.PlmRbmFitOpts(C_, E, int(steps_per_epoch), int(first_epoch), int(lr_decay_after), float(lr), float(lambda_g),
                              float(lambda_w), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(start))
    n = x0.size
    x = np.zeros(n, np.float32)
    data, model = np.zeros(n), np.zeros(n)
    chains = np.zeros((max(C_, 0), L), np.int8)
    trace = np.zeros((max(E, 0), 5))
    phase = np.zeros(4) if phase_times else None
    res = _lib.PlmRbmFitResult(_ptr(x), _ptr(data), _ptr(model), _ptr(chains), _ptr(trace), _ptr(phase), 0, 0)
    cb, reraise = _stop_callback(_lib.RBM_EPOCH_CB, callback, lambda epoch, *row: (int(epoch),) + row)
    rc = _lib.load().plm_rbm_fit(_ptr(msa), _ptr(w), msa.shape[0], L, q, M, _ptr(x0), C.byref(opts), int(device), None, cb,
                                 None, C.byref(res))
    reraise()
    check(rc)
    done = int(res.epochs_done)
    rows = done if res.status == _lib.STATUS_MAXITER else done + 1
    go, co, Wo = (a.copy() for a in _rbm_split(x, L, q, M))
    out = dict(g=go, c=co, W=Wo, data=_rbm_split(data, L, q, M), model=_rbm_split(model, L, q, M), chains=chains,
               trace=trace[:rows].copy(), epochs_done=done, status=RBM_STATUS[int(res.status)])
    if phase_times:
        out["phase_ms"] = phase
    return out


def rbm_log_partition(g, c, W, q, n_chains=4096, n_temps=1000, sweeps_per_temp=1, betas=None, seed=0, steps_per_launch=0,
                      callback=None, hidden=False, device=0):
    """
    log Z of the restricted Boltzmann machine (g, c, W) by annealed importance sampling on the GPU (plm_rbm_ais,
    DESIGN_NEXT_ROWS.md section 9.25): n_chains chains are annealed from the independent-site model of g (log Z_0 in
    closed form) to the full model over n_temps steps of sweeps_per_temp block-Gibbs sweeps each, with the inverse
    temperature beta_k on the hidden layer only (c and W scaled by it).  betas, steps_per_launch and callback are those
    of `log_partition`; with betas the result is log Z of the model with c and W scaled by beta_K.
    Returns a dict: log_z, log_z0, log_z_se, ess, log_w [C], states int8 [C, L], with hidden also hidden int8 [C, M] (the
    hidden units of the last sweep), steps_done, status ("converged" or "interrupted": log_z is NaN then).  When
    beta_K = 1 and the run completed also mean_score = sum_c w_c score(v_c) over the normalised weights, the score from
    `rbm_score` on the final states, and entropy = log_z - mean_score.
    """
    q, C_ = int(q), int(n_chains)
    x, L, M = _rbm_model(g, c, W, q)
    if betas is not None:
        betas = np.ascontiguousarray(betas, dtype=np.float32).reshape(-1)
        if betas.size < 2:
            raise ValueError("betas must hold at least beta_0 and beta_1")
        K = betas.size - 1
    else:
        K = int(n_temps)
    opts = _lib.PlmAisOpts(C_, K, int(sweeps_per_temp), int(steps_per_launch), _ptr(betas), int(seed) & 0xFFFFFFFFFFFFFFFF)
    n_out = max(C_, 1)
    log_w, states = np.zeros(n_out), np.zeros((n_out, L), np.int8)
    hid = np.zeros((n_out, M), np.int8) if hidden else None
    res = _lib.PlmRbmAisResult(0.0, 0.0, 0.0, 0.0, _ptr(log_w), _ptr(states), _ptr(hid), 0, 0)
    cb, reraise = _stop_callback(_lib.AIS_CB, callback)
    check(_lib.load().plm_rbm_ais(L, q, M, _ptr(x), C.byref(opts), int(device), None, cb, None, C.byref(res)))
    reraise()
    out = dict(log_z=float(res.log_z), log_z0=float(res.log_z0), log_z_se=float(res.log_z_se), ess=float(res.ess),
               log_w=log_w, states=states, steps_done=int(res.steps_done), status=BM_STATUS[int(res.status)])
    if hidden:
        out["hidden"] = hid
    last = 1.0 if betas is None else float(betas[-1])
    if res.status == _lib.STATUS_CONVERGED and last == 1.0:
        w = np.exp(log_w - log_w.max())
        out["mean_score"] = float((w / w.sum()) @ rbm_score(states, q, g, c, W, device=device))
        out["entropy"] = out["log_z"] - out["mean_score"]
    return out


def sample_plan(L, q, n_chains, n_cu=0):
    """
    The launch plan `sample` and `bm_fit` use for L sites, q states and n_chains chains (plm_sample_plan,
    DESIGN_NEXT_ROWS.md section 9.6) on a device with n_cu compute units; n_cu = 0: the current device.  With n_cu > 0
    no device is needed.  Returns a dict: direct (bool), tile (chains per workgroup), jc (sites per staged chunk, 0 for
    the direct form), nv (ceil(q / 4)), n_workgroups, lds_bytes.  PLM_SAMPLE_FORM, PLM_SAMPLE_TILE and PLM_SAMPLE_JC
    are honoured as the sampler honours them.
    """
    info = _lib.PlmSamplePlanInfo()
    check(_lib.load().plm_sample_plan(int(L), int(q), int(n_chains), int(n_cu), C.byref(info)))
    return dict(direct=bool(info.direct), tile=int(info.tile), jc=int(info.jc), nv=int(info.nv),
                n_workgroups=int(info.n_workgroups), lds_bytes=int(info.lds_bytes))


BM_STATUS = {_lib.STATUS_CONVERGED: "converged", _lib.STATUS_MAXITER: "maxiter", _lib.STATUS_INTERRUPTED: "interrupted"}


def log_partition(hi, jij, q, n_chains=4096, n_temps=1000, sweeps_per_temp=1, betas=None, seed=0, steps_per_launch=0,
                  callback=None, device=0):
    """
    log Z of the Potts model (hi, jij) by annealed importance sampling on the GPU (plm_ais, DESIGN_NEXT_ROWS.md section
    9.8): n_chains chains are annealed from the independent-site model of the fields (log Z_0 in closed form) to the full
    model over n_temps steps of sweeps_per_temp Gibbs sweeps each, with the inverse temperature beta_k on the couplings
    only.  betas: None (beta_k = k / n_temps) or the n_temps + 1 values 0 = beta_0 <= ... <= beta_K, which then set
    n_temps; the result is log Z of the model with the couplings scaled by beta_K.  The steps run in launches of at most
    steps_per_launch steps (0: about a second each; the result does not depend on it); callback(steps_done, n_steps) is
    called between launches and stops the anneal by returning a true value.
    Returns a dict: log_z, log_z0, log_z_se (standard error of log_z from the spread of the weights), ess (effective
    sample size of the chains), log_w [C], e_j [C] (the tracked coupling energy of the final states), states int8 [C, L],
    steps_done, status ("converged" or "interrupted": log_z is NaN then).  When beta_K = 1 also mean_energy = sum_c w_c
    H(x_c) over the normalised weights, H from `hamiltonians` on the final states, and entropy = log_z - mean_energy.
    """
    q, C_ = int(q), int(n_chains)
    hi, jij, L = _potts_model(hi, jij, q)
    if betas is not None:
        betas = np.ascontiguousarray(betas, dtype=np.float32).reshape(-1)
        if betas.size < 2:
            raise ValueError("betas must hold at least beta_0 and beta_1")
        K = betas.size - 1
    else:
        K = int(n_temps)
    lib = _lib.load()
    opts = _lib.PlmAisOpts(C_, K, int(sweeps_per_temp), int(steps_per_launch), _ptr(betas), int(seed) & 0xFFFFFFFFFFFFFFFF)
    n_out = max(C_, 1)
    log_w, e_j, states = np.zeros(n_out), np.zeros(n_out), np.zeros((n_out, L), np.int8)
    res = _lib.PlmAisResult(0.0, 0.0, 0.0, 0.0, _ptr(log_w), _ptr(e_j), _ptr(states), 0, 0)
    cb, reraise = _stop_callback(_lib.AIS_CB, callback)
    check(lib.plm_ais(L, q, _ptr(_canonical(hi, jij, L, q)), C.byref(opts), int(device), None, cb, None, C.byref(res)))
    reraise()
    out = dict(log_z=float(res.log_z), log_z0=float(res.log_z0), log_z_se=float(res.log_z_se), ess=float(res.ess),
               log_w=log_w, e_j=e_j, states=states, steps_done=int(res.steps_done), status=BM_STATUS[int(res.status)])
    last = 1.0 if betas is None else float(betas[-1])
    if res.status == _lib.STATUS_CONVERGED and last == 1.0:
        if L > 1:
            H = hamiltonians(states, q, hi, jij, device=device)[:, 0]
        else:
            H = hi[0].astype(np.float64)[states[:, 0]]
        w = np.exp(log_w - log_w.max())
        out["mean_energy"] = float((w / w.sum()) @ H)
        out["entropy"] = out["log_z"] - out["mean_energy"]
    return out


def tempering_ladder(n_rungs, beta_max=1.0, kind="linear"):
    """
    A ladder of n_rungs inverse temperatures for `parallel_tempering`, float32, from beta_0 = 0 to beta_max.
    kind = "linear": beta_r = beta_max r / (R - 1).  kind = "geometric": beta_0 = 0 and the other rungs in geometric
    progression up to beta_max with the ratio 2 (beta_r = beta_max 2^(r - R + 1)): close rungs where the couplings are
    weak, wide ones near beta_max.  One rung is beta_max alone.
    """
    R, top = int(n_rungs), float(beta_max)
    if R < 1 or not (top >= 0.0 and np.isfinite(top)):
        raise ValueError("need n_rungs >= 1 and a finite beta_max >= 0")
    if R == 1:
        return np.array([top], np.float32)
    if kind == "linear":
        return np.array([top * r / (R - 1) for r in range(R)], np.float32)
    if kind == "geometric":
        return np.array([0.0] + [top * 2.0 ** (r - R + 1) for r in range(1, R)], np.float32)
    raise ValueError('kind must be "linear" or "geometric"')


def parallel_tempering(hi, jij, q, n_ladders, betas, burn_in=10, n_snapshots=1, thin=1, sweeps_per_round=1, seed=0,
                       all_rungs=False, start=None, first_round=0, callback=None, device=0):
    """
    Replica-exchange Gibbs sampling of the Potts model (hi, jij) on the GPU (plm_pt, DESIGN_NEXT_ROWS.md section 9.9):
    n_ladders independent ladders of R = len(betas) walkers sample p_beta(x) ~ exp(sum_i h_i(x_i) + beta sum_{i<j}
    J_ij(x_i, x_j)) at the inverse temperatures 0 <= beta_0 <= ... <= beta_{R-1} (see `tempering_ladder`).  A round is
    sweeps_per_round Gibbs sweeps of every walker at the beta of its rung and one exchange pass between neighbouring rungs
    (pairs (0,1), (2,3), .. in even rounds, (1,2), (3,4), .. in odd ones).  burn_in rounds, then n_snapshots snapshots
    thin rounds apart.
    start: None, or the `walkers` triple (states, rungs, e_j) of an earlier call, which this call then continues bit for
    bit when first_round is the number of rounds made so far; (states, rungs) or (states, rungs, None) has the energies
    measured, and rungs None puts slot s of every ladder at rung s.  callback(rounds_done, n_rounds) is called between
    rounds and stops the run by returning a true value.
    Returns a dict: samples int8 [K, C, L] (the walkers at the top rung) or, with all_rungs, [K, C, R, L] in rung order;
    energies float64 [..., 3] = (H, H_J, H_h) of those rows at beta = 1, what `hamiltonians` gives; e_j [...] the tracked
    coupling energy of those rows; accepts, attempts int64 [R - 1] and acceptance = accepts / attempts per pair of rungs;
    walkers = (states int8 [C R, L], rungs int32 [C R], e_j float64 [C R]); rounds_done; status ("converged" or
    "interrupted": snapshots not yet taken are zero then).
    """
    q, C_, K = int(q), int(n_ladders), int(n_snapshots)
    hi, jij, L = _potts_model(hi, jij, q)
    betas = np.ascontiguousarray(betas, dtype=np.float32).reshape(-1)
    R = betas.size
    if R < 1:
        raise ValueError("betas must hold at least one inverse temperature")
    x0 = rungs0 = e0 = None
    if start is not None:
        parts = tuple(start) + (None,) * (3 - len(start)) if 1 <= len(start) <= 3 else ()
        if len(parts) != 3 or parts[0] is None:
            raise ValueError("start must be (states, rungs, e_j), (states, rungs) or (states,)")
        x0 = np.ascontiguousarray(parts[0], dtype=np.int8)
        if x0.shape != (max(C_, 0) * R, L):
            raise ValueError("the start states must be an (n_ladders * R, L) = (%d, %d) matrix" % (C_ * R, L))
        if parts[1] is not None:
            rungs0 = np.ascontiguousarray(parts[1], dtype=np.int32).reshape(-1)
            if rungs0.size != C_ * R:
                raise ValueError("the start rungs must hold n_ladders * R = %d values" % (C_ * R))
        if parts[2] is not None:
            if rungs0 is None:
                raise ValueError("start energies need the start rungs")
            e0 = np.ascontiguousarray(parts[2], dtype=np.float64).reshape(-1)
            if e0.size != C_ * R:
                raise ValueError("the start energies must hold n_ladders * R = %d values" % (C_ * R))
    lib = _lib.load()
    opts = _lib.PlmPtOpts(C_, R, int(burn_in), K, int(thin), int(sweeps_per_round), int(first_round),
                          1 if all_rungs else 0, _ptr(betas), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(x0), _ptr(rungs0),
                          _ptr(e0))
    Cn, Kn = max(C_, 1), max(K, 1)
    shape = (Kn, Cn, R) if all_rungs else (Kn, Cn)
    samples, e_j = np.zeros(shape + (L,), np.int8), np.zeros(shape)
    accepts, attempts = np.zeros(R - 1, np.int64), np.zeros(R - 1, np.int64)
    walkers, rungs, walker_e = np.zeros((Cn * R, L), np.int8), np.zeros(Cn * R, np.int32), np.zeros(Cn * R)
    res = _lib.PlmPtResult(_ptr(samples), _ptr(e_j), _ptr(accepts) if R > 1 else None,
                           _ptr(attempts) if R > 1 else None, _ptr(walkers), _ptr(rungs), _ptr(walker_e), 0, 0)
    cb, reraise = _stop_callback(_lib.PT_CB, callback)
    check(lib.plm_pt(L, q, _ptr(_canonical(hi, jij, L, q)), C.byref(opts), int(device), None, cb, None, C.byref(res)))
    reraise()
    rows = samples.reshape(-1, L)
    if L > 1:
        en = hamiltonians(rows, q, hi, jij, device=device)
    else:
        hh = hi[0].astype(np.float64)[rows[:, 0]]
        en = np.stack([hh, np.zeros_like(hh), hh], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        acceptance = accepts / attempts.astype(np.float64)
    return dict(samples=samples, energies=en.reshape(shape + (3,)), e_j=e_j, accepts=accepts, attempts=attempts,
                acceptance=acceptance, walkers=(walkers, rungs, walker_e), rounds_done=int(res.rounds_done),
                status=BM_STATUS[int(res.status)])


def tempered_log_z(e_j, betas, log_z0):
    """
    The estimate of `log_partition_tempered` from the tracked energies e_j [K, C, R] of all rungs: (log_z, log_z_se,
    se of every step [R - 1]), all in float64.  Step r: m_r + log mean exp(d_r E_r - m_r) over the snapshots and ladders of
    rung r, d_r = beta_{r+1} - beta_r, m_r = max d_r E_r; its standard error from the spread of the per-ladder means.
    """
    e_j = np.asarray(e_j, np.float64)
    b = np.asarray(betas, np.float32).astype(np.float64)
    K, Cn, R = e_j.shape
    log_z, se = float(log_z0), np.zeros(max(R - 1, 0))
    for r in range(R - 1):
        a = (b[r + 1] - b[r]) * e_j[:, :, r]
        m = a.max()
        w = np.exp(a - m).mean(axis=0)              # one mean per ladder: ladders are independent, snapshots are not
        log_z += m + np.log(w.mean())
        se[r] = w.std(ddof=1) / (np.sqrt(Cn) * w.mean()) if Cn > 1 else 0.0
    return log_z, float(np.sqrt((se * se).sum())), se


def log_partition_tempered(hi, jij, q, n_ladders, betas, **kw):
    """
    log Z of the Potts model (hi, jij) with the couplings scaled by betas[-1], from one run of `parallel_tempering` (whose
    keyword arguments these are; all_rungs is set) on a ladder that starts at beta_0 = 0, where log Z_0 = sum_i log sum_a
    exp h_i(a) is known:
        log_z = log Z_0 + sum_r [m_r + log mean exp((beta_{r+1} - beta_r) E_r - m_r)],
    the mean over the snapshots and ladders of rung r, in float64.  log_z_se = sqrt(sum_r se_r^2), se_r the standard error
    of step r from the per-ladder means (ladders are independent, snapshots of one ladder are not).  The correlation
    between the rungs of a ladder is ignored in log_z_se; sum(se_rungs) bounds the error whatever that correlation is.
    Unlike annealed importance sampling the estimate rests on equilibrium samples of every rung, so burn_in matters and
    the weights cannot degenerate along the path.
    Returns the dict of `parallel_tempering` with log_z, log_z0, log_z_se and se_rungs [R - 1] added (log_z is NaN when
    the run was interrupted).
    """
    betas = np.ascontiguousarray(betas, dtype=np.float32).reshape(-1)
    if betas.size < 1 or betas[0] != 0.0:
        raise ValueError("the ladder must start at beta_0 = 0, where log Z is known")
    kw["all_rungs"] = True
    res = parallel_tempering(hi, jij, q, n_ladders, betas, **kw)
    h = np.asarray(hi, np.float32).astype(np.float64).reshape(-1, int(q))
    m = h.max(axis=1)
    res["log_z0"] = float(sum(m[i] + np.log(np.exp(h[i] - m[i]).sum()) for i in range(h.shape[0])))
    if res["status"] == "converged":
        res["log_z"], res["log_z_se"], res["se_rungs"] = tempered_log_z(res["e_j"], betas, res["log_z0"])
    else:
        res["log_z"], res["log_z_se"], res["se_rungs"] = float("nan"), float("nan"), np.full(betas.size - 1, np.nan)
    return res


def annealing_schedule(n_steps, beta_min=0.1, beta_max=4.0, kind="geometric"):
    """
    The n_steps inverse temperatures of a schedule for `anneal`, float32, from beta_min to beta_max.
    kind = "geometric": beta_k = beta_min (beta_max / beta_min)^(k / (K - 1)); kind = "linear": beta_k = beta_min +
    (beta_max - beta_min) (k / (K - 1)); k = 0 .. K - 1.  Every value is computed in float64 (Python floats, the
    operations in the order written) and rounded once to float32.  One step is beta_max alone, none is an empty array.
    """
    K, lo, hi_ = int(n_steps), float(beta_min), float(beta_max)
    if K < 0 or not (0.0 < lo <= hi_ and np.isfinite(hi_)):
        raise ValueError("need n_steps >= 0 and finite 0 < beta_min <= beta_max")
    if kind not in ("geometric", "linear"):
        raise ValueError('kind must be "geometric" or "linear"')
    if K <= 1:
        return np.array([hi_] * K, np.float32)
    if kind == "geometric":
        b = [lo * (hi_ / lo) ** (k / (K - 1)) for k in range(K)]
    else:
        b = [lo + (hi_ - lo) * (k / (K - 1)) for k in range(K)]
    return np.array(b, np.float64).astype(np.float32)


def anneal(hi, jij, q, n_chains, betas=None, n_steps=100, sweeps_per_step=1, max_greedy=100, seed=0, start=None, fixed=None,
           allowed=None, first_sweep=0, steps_per_launch=0, callback=None, energies=True, device=0):
    """
    Simulated annealing and greedy ascent on the Potts model (hi, jij) on the GPU (plm_anneal, DESIGN_NEXT_ROWS.md section
    9.13): the search for sequences of high statistical energy H (P(x) ~ exp H(x), higher is better).  n_chains chains make
    sweeps_per_step Gibbs sweeps of `sample` at every inverse temperature of betas (None: annealing_schedule(n_steps); an
    array sets n_steps, any positive finite values in any order), then at most max_greedy greedy sweeps, in which a site
    moves to its best allowed state only when that improves H strictly.  After every step, and after the greedy sweeps,
    a chain whose tracked gain exceeds its best so far records its states (a checkpoint).
    start, fixed, allowed: as for `sample` (start None: the start rule at beta = 1).  first_sweep: the sweep index of the
    first annealing sweep, to continue an earlier call from its `states`.  The steps run in launches of at most
    steps_per_launch steps (0: about a second each; no result depends on it); callback(steps_done, n_steps) is called
    between launches and stops the call by returning a true value (the greedy sweeps do not run then); an exception it
    raises is raised again here.  Chain c depends on (seed, c, model, options, its start) only.
    Returns a dict: states int8 [C, L], gain [C] (tracked H(states) - H(start)), best int8 [C, L], best_gain [C], best_at
    int32 [C] (checkpoint 0 .. n_steps + 1), last_move int32 [C] (the last greedy sweep, from 1, in which the chain moved;
    0: none), converged bool [C] (the chain made a greedy sweep without a move: it is a local optimum), energies and
    best_energies float64 [C, 3] = (H, H_J, H_h) as `hamiltonians` (None with energies=False), steps_done, status
    ("converged" or "interrupted").
    """
    q, C_ = int(q), int(n_chains)
    hi, jij, L = _potts_model(hi, jij, q)
    if betas is None:
        betas = annealing_schedule(int(n_steps))
    betas = np.ascontiguousarray(betas, dtype=np.float32).reshape(-1)
    K = betas.size
    if C_ < 1:
        raise ValueError("need n_chains >= 1")
    start, fixed, allowed = _chain_args(start, fixed, allowed, C_, L, q)
    lib = _lib.load()
    opts = _lib.PlmAnnealOpts(C_, K, int(sweeps_per_step), int(max_greedy), int(first_sweep) & 0xFFFFFFFF,
                              int(steps_per_launch), _ptr(betas) if K else None, int(seed) & 0xFFFFFFFFFFFFFFFF,
                              _ptr(start), _ptr(fixed), _ptr(allowed))
    out = dict(states=np.zeros((C_, L), np.int8), gain=np.zeros(C_), best=np.zeros((C_, L), np.int8),
               best_gain=np.zeros(C_), best_at=np.zeros(C_, np.int32), last_move=np.zeros(C_, np.int32),
               converged=np.zeros(C_, np.uint8), energies=np.zeros((C_, 3)) if energies else None,
               best_energies=np.zeros((C_, 3)) if energies else None)
    res = _lib.PlmAnnealResult(*[_ptr(out[k]) for k in ("states", "gain", "best", "best_gain", "best_at", "last_move",
                                                        "converged", "energies", "best_energies")], 0, 0)
    cb, reraise = _stop_callback(_lib.ANNEAL_CB, callback)
    check(lib.plm_anneal(L, q, _ptr(_canonical(hi, jij, L, q)), C.byref(opts), int(device), None, cb, None, C.byref(res)))
    reraise()
    out["converged"] = out["converged"].astype(bool)
    out["steps_done"] = int(res.steps_done)
    out["status"] = BM_STATUS[int(res.status)]
    return out


def greedy_ascent(hi, jij, q, start, max_sweeps=100, fixed=None, allowed=None, device=0):
    """
    The local optimum of H every given sequence runs into: `anneal` without annealing steps.  start: n x L states; a
    sweep moves every free site to its best allowed state when that improves H strictly (the first such state on equal
    values, no move on a tie), until a sweep moves nothing or max_sweeps sweeps are made.  Returns the dict of `anneal`:
    states are the optima where converged is set, last_move the number of sweeps that moved something.
    """
    start = np.ascontiguousarray(start, dtype=np.int8)
    if start.ndim != 2:
        raise ValueError("start must be an (n, L) matrix of states")
    return anneal(hi, jij, q, start.shape[0], n_steps=0, max_greedy=max_sweeps, start=start, fixed=fixed, allowed=allowed,
                  device=device)


def bm_fit(fi, fij, q, hi, jij, n_chains, n_epochs, sweeps_per_epoch=2, lr=0.5, lr_decay_after=0, lambda_h=0.0,
           lambda_j=0.0, tol=0.0, seed=0, start=None, first_epoch=0, callback=None, device=0):
    """
    Boltzmann-machine refinement of a Potts model (plm_bm_fit, DESIGN_NEXT_ROWS.md section 9.7): n_epochs steps of
    x <- x + lr_g ((f - p) - 2 lambda x), where p are the one- and two-site frequencies of n_chains persistent Gibbs
    chains after sweeps_per_epoch sweeps under the current x, and f = (fi, fij) are the targets.
    fi: L x q; fij, jij: the i<j blocks [L(L-1)/2][q][q]; hi: L x q (the start point together with jij).  lambda_h,
    lambda_j: per-sequence scale (the plmc value over N_eff).  lr_decay_after = T > 0: the step of global epoch g is
    lr T / (g + 1) once g + 1 > T.  start: None (the sampler's start rule at the start point) or n_chains x L states;
    first_epoch: the global number of the first epoch, for a call that continues an earlier one from its hi, jij and
    chains.  tol > 0 stops before the update of the first epoch whose two maximal errors are <= tol; callback(epoch,
    max_dfi, max_dfij, rms_dfij, lr) is called once per epoch and stops the fit by returning a true value.
    Returns a dict: hi, jij, pi, pij, chains (int8 C x L), trace (one row per epoch that ran: max |fi - pi|,
    max |fij - pij|, rms of fij - pij, lr_g), epochs_done (updates applied), status ("maxiter", "converged",
    "interrupted").  The result is bitwise reproducible.
    """
    q, C_, E = int(q), int(n_chains), int(n_epochs)
    hi, jij, L = _potts_model(hi, jij, q)
    n_j = jij.size
    fi = np.ascontiguousarray(fi, dtype=np.float32)
    if fi.shape != (L, q):
        raise ValueError("fi must be an (L, q) = (%d, %d) matrix" % (L, q))
    fij = np.ascontiguousarray(fij, dtype=np.float32)
    if fij.size != n_j:
        raise ValueError("fij has %d entries, expected the %d i<j blocks of %d x %d" % (fij.size, L * (L - 1) // 2, q, q))
    if C_ < 1 or E < 1 or int(sweeps_per_epoch) < 1 or int(first_epoch) < 0 or int(lr_decay_after) < 0:
        raise ValueError("need n_chains >= 1, n_epochs >= 1, sweeps_per_epoch >= 1, first_epoch >= 0 and lr_decay_after >= 0")
    for name, v in (("lr", lr), ("lambda_h", lambda_h), ("lambda_j", lambda_j), ("tol", tol)):
        if not (float(v) >= 0.0 and np.isfinite(float(v))):
            raise ValueError("%s must be finite and >= 0 (got %r)" % (name, v))
    start = _chain_args(start, None, None, C_, L, q)[0]
    lib = _lib.load()
    opts = _lib.PlmBmOpts(C_, E, int(sweeps_per_epoch), int(first_epoch), float(lr), int(lr_decay_after), float(lambda_h),
                          float(lambda_j), float(tol), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(start))
    x = np.zeros(L * q + n_j, np.float32)
    pi, pij = np.zeros((L, q), np.float32), np.zeros((L * (L - 1) // 2, q, q), np.float32)
    chains = np.zeros((C_, L), np.int8)
    trace = np.zeros((E, 4))
    res = _lib.PlmBmResult(_ptr(x), _ptr(pi), _ptr(pij), _ptr(chains), _ptr(trace), 0, 0)
    cb, reraise = _stop_callback(_lib.BM_EPOCH_CB, callback, lambda epoch, *errors: (int(epoch),) + errors)
    check(lib.plm_bm_fit(L, q, _ptr(fi), _ptr(fij), _ptr(_canonical(hi, jij, L, q)), C.byref(opts), int(device), None, cb,
                         None, C.byref(res)))
    reraise()
    done = int(res.epochs_done)
    rows = done if res.status == _lib.STATUS_MAXITER else done + 1
    return dict(hi=x[:L * q].reshape(L, q).copy(), jij=x[L * q:].reshape(L * (L - 1) // 2, q, q).copy(), pi=pi, pij=pij,
                chains=chains, trace=trace[:rows].copy(), epochs_done=done, status=BM_STATUS[int(res.status)])


def single_mutant_matrix(target, q, hi, jij, device=0):
    """
    Energy differences of every single substitution of `target`: L x q x 3 float64 (dH, dH_J, dH_h), the
    return value of the reference's `_single_mutant_hamiltonians` (couplings/model.py:63-109).
    """
    target = np.ascontiguousarray(target, dtype=np.int8).reshape(1, -1)
    L = target.shape[1]
    hj = potentials(target, q, hi, jij, device=device)[0].astype(np.float64)
    hi = np.asarray(hi, dtype=np.float64).reshape(L, q)
    rows = np.arange(L)
    dj = hj - hj[rows, target[0]][:, None]
    dh = hi - hi[rows, target[0]][:, None]
    return np.stack([dj + dh, dj, dh], axis=2)


def mean_field(msa, q=21, theta_id=0.8, pseudo_count=0.5, device=0, want_fij=True, want_full=True, want_di=True):
    """
    Mean-field direct coupling analysis of an alignment: the arithmetic of the reference's
    `MeanFieldDCA.fit` (couplings/mean_field.py:163-222) and `direct_information` (:842-893) on the GPU.
    Returns weights, n_eff, raw fi [L,q] / fij [pairs,q,q], fields hi [L,q] (float64), couplings as the i<j blocks
    jij [pairs,q,q] (float32) and, if want_full, the dense jij_full [L,L,q,q] (float64, diagonal blocks included,
    last row/column of every block zero), and di [L,L] (float64).
    """
    lib = _lib.load()
    msa = _msa(msa)
    N, L = msa.shape
    npair = L * (L - 1) // 2
    out = {
        "weights": np.zeros(N, np.float32), "fi": np.zeros((L, q), np.float32), "hi": np.zeros((L, q)),
        "jij": np.zeros((npair, q, q), np.float32),
    }
    if want_fij:
        out["fij"] = np.zeros((npair, q, q), np.float32)
    if want_full:
        out["jij_full"] = np.zeros((L, L, q, q))
    if want_di:
        out["di"] = np.zeros((L, L))
    res = _lib.PlmMfResult()
    for name in ("weights", "fi", "fij", "hi", "jij_full", "jij", "di"):
        if name in out:
            setattr(res, name, out[name].ctypes.data)
    check(lib.plm_meanfield(_ptr(msa), N, L, q, float(theta_id), float(pseudo_count), device, None, C.byref(res)))
    out["n_eff"] = float(res.n_eff)
    out["theta_id"], out["pseudo_count"] = theta_id, pseudo_count
    return out


def direct_information(jij_full, fi, device=0):
    """DI of every pair from dense couplings [L,L,q,q] and frequencies [L,q] (both float64): the reference's
    `direct_information(J_ij, f_i)` (couplings/mean_field.py:842-893).  Returns [L,L] float64."""
    lib = _lib.load()
    jij_full = np.ascontiguousarray(jij_full, dtype=np.float64)
    fi = np.ascontiguousarray(fi, dtype=np.float64)
    L, q = fi.shape
    assert jij_full.shape == (L, L, q, q)
    di = np.zeros((L, L))
    check(lib.plm_direct_information(_ptr(jij_full), _ptr(fi), L, q, device, None, _ptr(di)))
    return di


# ---- analysis of a fitted model (the numeric rest of the reference's CouplingsModel) ----------------------------
MODEL_FI_PRODUCT_F32 = 1


def _f64(a):
    """contiguous float64 view of `a` (no copy when it already is one)"""
    return np.ascontiguousarray(a, dtype=np.float64)


def model_pair_scores(J_ij, f_ij, f_i, device=0):
    """FN of the zero-sum-gauged couplings and mutual information of every pair: the arithmetic of
    `CouplingsModel._calculate_ecs` (couplings/model.py:777-799).  J_ij, f_ij: dense [L,L,q,q] (only the i<j blocks
    are read), f_i: [L,q].  Returns (fn, mi), symmetric [L,L] float64 with a zero diagonal; mi is +inf for a pair with
    f_ij(a,b) > 0 where f_i(a) f_j(b) = 0, as numpy gives."""
    lib = _lib.load()
    # float32 f_i (the plmc_v2 reader's): numpy's outer product f_i f_j^T is float32 then; the kernel rounds it the same way
    flags = MODEL_FI_PRODUCT_F32 if np.asarray(f_i).dtype == np.float32 else 0
    J_ij, f_ij, f_i = _f64(J_ij), _f64(f_ij), _f64(f_i)
    L, q = f_i.shape
    if J_ij.shape != (L, L, q, q) or f_ij.shape != (L, L, q, q):
        raise ValueError("J_ij and f_ij must be (%d, %d, %d, %d)" % (L, L, q, q))
    fn, mi = np.empty((L, L)), np.empty((L, L))
    check(lib.plm_model_pair_scores_ex(_ptr(J_ij), _ptr(f_ij), _ptr(f_i), L, q, flags, device, None, _ptr(fn),
                                       _ptr(mi)))
    return fn, mi


def double_mutant_matrix(J_ij, smm, target, device=0):
    """`CouplingsModel.double_mut_mat` (couplings/model.py:715-742): dense [L,L,q,q] float64 with
    D[i,j,a,b] = smm[i,a] + smm[j,b] + J_ij[a,b] - J_ij[a,t_j] - J_ij[t_i,b] + J_ij[t_i,t_j], D[j,i] = D[i,j].T and
    zero diagonal blocks.  smm: [L,q] single-mutant matrix of the target, target: L states."""
    lib = _lib.load()
    J_ij, smm = _f64(J_ij), _f64(smm)
    L, q = smm.shape
    if J_ij.shape != (L, L, q, q):
        raise ValueError("J_ij must be (%d, %d, %d, %d)" % (L, L, q, q))
    target = np.ascontiguousarray(np.asarray(target).ravel(), dtype=np.int8)
    if target.shape != (L,):
        raise ValueError("target must hold %d states" % L)
    D = np.empty((L, L, q, q))
    check(lib.plm_double_mutants(_ptr(J_ij), _ptr(smm), _ptr(target), L, q, device, None, _ptr(D)))
    return D


def independent_fields(f_i, lambda_h, n_eff, device=0):
    """Fields of the L2-regularised independent-site model, site by site
    argmin_x n_eff (logZ(x) - f_i.x) + lambda_h |x|^2 (the objective of `CouplingsModel.to_independent_model`,
    couplings/model.py:894-910), by damped Newton on the GPU.  Returns (h [L,q] float64, Newton steps [L] int32).
    lambda_h must be > 0."""
    lib = _lib.load()
    f_i = _f64(f_i)
    L, q = f_i.shape
    h, iters = np.empty((L, q)), np.empty(L, np.int32)
    check(lib.plm_independent_fields(_ptr(f_i), L, q, float(lambda_h), float(n_eff), device, None, _ptr(h),
                                     _ptr(iters)))
    return h, iters


# ---- mutation tables and combinatorial libraries (DESIGN_NEXT_ROWS.md section 9.16) ------------------------------
MUTANT_STATUS = {0: "ok", 1: "more entries than sites", 2: "position outside the model", 3: "state outside the alphabet",
                 4: "position named twice"}


def _target_model(target, q, hi, jij):
    hi, jij, L = _potts_model(hi, jij, q)
    target = np.ascontiguousarray(np.asarray(target).ravel(), dtype=np.int8)
    if target.shape != (L,):
        raise ValueError("target must hold %d states" % L)
    return target, L, _canonical(hi, jij, L, q)


def mutant_effects(target, q, hi, jij, offsets, positions, states, device=0, tables=False):
    """
    Energy differences of variants of `target`, the arithmetic of the reference's `_delta_hamiltonian`
    (couplings/model.py:112-176) for a whole table at once.  Variant v substitutes, at the 0-based sites
    positions[offsets[v]:offsets[v+1]], the states states[offsets[v]:offsets[v+1]].  Returns (out, status): out is
    n x 3 float64 (dH, dH_J, dH_h), status n uint8 (0, or a key of MUTANT_STATUS with NaN in the row: more entries than
    sites, a position or state outside the model, a position named twice).  With tables=True a third value follows:
    the L x q x 2 float64 single-mutant tables (S_J, S_h).
    """
    lib = _lib.load()
    target, L, x = _target_model(target, q, hi, jij)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).ravel()
    positions = np.ascontiguousarray(positions, dtype=np.int32).ravel()
    states = np.ascontiguousarray(states, dtype=np.int8).ravel()
    if offsets.size < 1 or positions.size != states.size:
        raise ValueError("offsets must hold n + 1 entries, positions and states one entry per substitution")
    n = offsets.size - 1
    out, status = np.empty((n, 3)), np.empty(n, np.uint8)
    tab = np.empty((L, q, 2)) if tables else None
    check(lib.plm_mutant_effects(_ptr(x), L, q, _ptr(target), n, _ptr(offsets), positions.size, _ptr(positions),
                                 _ptr(states), device, None, _ptr(out), _ptr(status), _ptr(tab)))
    return (out, status, tab) if tables else (out, status)


def _scan_letters(letters, k, q):
    """(letter_offsets int32 [k + 1], letters int8) of per-site letter lists; None: every state at every site."""
    if letters is None:
        letters = [range(q)] * k
    if len(letters) != k:
        raise ValueError("letters must hold one list per site")
    lists = [np.asarray(list(l), dtype=np.int8) for l in letters]
    lo = np.zeros(k + 1, np.int32)
    lo[1:] = np.cumsum([len(l) for l in lists])
    return lo, np.ascontiguousarray(np.concatenate(lists) if k else np.zeros(0), dtype=np.int8)


def scan_digits(index, sizes):
    """The digits (one column per site, the last site fastest) of combination indices for per-site list sizes."""
    index = np.asarray(index, dtype=np.int64)
    digits = np.empty(index.shape + (len(sizes),), np.int64)
    for s in range(len(sizes) - 1, -1, -1):
        index, digits[..., s] = np.divmod(index, int(sizes[s]))
    return digits


def mutant_scan(target, q, hi, jij, sites, letters=None, first=0, count=None, energies=False, edges=None, threshold=None,
                capacity=1 << 16, device=0):
    """
    dH of every combination of letters at up to 8 distinct `sites` (0-based) of `target`.  letters: one list of states
    per site (None: all q states).  Combinations are numbered like `itertools.product(*letters)`, the last site
    fastest; the call covers [first, first + count) (count None: to the end).  Returns a dict: `n_combinations`, `first`,
    `count`, `dh_min`, `dh_max` (exact extremes over the range); with energies=True `energies` (count x 3:
    dH, dH_J, dH_h); with edges (ascending, at most 1024) `histogram` (uint64, len(edges) + 1: bin = number of edges
    <= dH, i.e. `np.searchsorted(edges, dH, side="right")`); with threshold `n_kept` (how many have dH >= threshold) and,
    unless n_kept > capacity (then `kept_index` is None: call again with the room), `kept_index` (ascending) and
    `kept_energies`.
    """
    lib = _lib.load()
    target, L, x = _target_model(target, q, hi, jij)
    sites = np.ascontiguousarray(np.asarray(sites).ravel(), dtype=np.int32)
    k = sites.size
    lo, let = _scan_letters(letters, k, q)
    total = 1
    for s in range(k):
        total *= int(lo[s + 1] - lo[s])
    first = int(first)
    count = max(total - first, 0) if count is None else int(count)
    capacity = int(capacity) if threshold is not None else 0
    en = np.empty((count, 3)) if energies else None
    ed = hist = None
    if edges is not None:
        ed = np.ascontiguousarray(edges, dtype=np.float64).ravel()
        n_edges = ed.size
        ed = ed if n_edges else np.zeros(1)              # no edge at all: one bin; the library still wants a pointer
        hist = np.zeros(n_edges + 1, np.uint64)
    kidx = np.empty(capacity, np.int64) if capacity > 0 else None
    ken = np.empty((capacity, 3)) if capacity > 0 else None
    opts = _lib.PlmScanOpts(n_scan_sites=k, flags=0, sites=sites.ctypes.data,
                            letter_offsets=lo.ctypes.data, letters=let.ctypes.data, first=first, count=count,
                            edges=None if ed is None else ed.ctypes.data, n_edges=0 if ed is None else n_edges,
                            use_threshold=int(threshold is not None), threshold=0.0 if threshold is None else float(threshold),
                            capacity=capacity)
    res = _lib.PlmScanResult()
    for name, arr in (("energies", en), ("histogram", hist), ("kept_index", kidx), ("kept_energies", ken)):
        if arr is not None:
            setattr(res, name, arr.ctypes.data)
    check(lib.plm_mutant_scan(_ptr(x), L, q, _ptr(target), C.byref(opts), device, None, C.byref(res)))
    out = dict(n_combinations=int(res.n_combinations), first=first, count=count, dh_min=float(res.dh_min),
               dh_max=float(res.dh_max))
    if energies:
        out["energies"] = en
    if hist is not None:
        out["histogram"] = hist
    if threshold is not None:
        n_kept = int(res.n_kept)
        fits = n_kept <= capacity
        out.update(n_kept=n_kept, kept_index=kidx[:n_kept].copy() if fits and n_kept else (np.zeros(0, np.int64) if fits else None),
                   kept_energies=ken[:n_kept].copy() if fits and n_kept else (np.zeros((0, 3)) if fits else None))
    return out


def top_combinations(target, q, hi, jij, sites, letters=None, top=100, device=0, max_keep=None, chunk=1 << 24):
    """
    The `top` combinations of largest dH among all letter combinations at `sites` (as for `mutant_scan`), ordered by
    (-dH, index): (index int64 [n], energies float64 [n, 3]), n = min(top, number of combinations).  One pass for the
    extremes, then histograms over 1024 edges that narrow onto the bin holding the top-th value until a threshold keeps
    at most max_keep combinations (default max(4 top, 2^20)), then one compacting pass whose buffer holds exactly what
    the histogram counted.  Where values tie so densely that no threshold separates that few (the bin cannot be split
    further), the library is walked in ranges of `chunk` combinations and the best are merged range by range.
    """
    top = int(top)
    if top < 1:
        raise ValueError("top must be >= 1")
    kw = dict(letters=letters, device=device)
    ext = mutant_scan(target, q, hi, jij, sites, **kw)
    total = ext["n_combinations"]
    top = min(top, total)
    max_keep = max(4 * top, 1 << 20) if max_keep is None else max(int(max_keep), top)

    def best(idx, en):
        order = np.lexsort((idx, -en[:, 0]))[:top]
        return idx[order], en[order]

    def compact(thr, expect, first=0, count=None):
        res = mutant_scan(target, q, hi, jij, sites, first=first, count=count, threshold=thr, capacity=max(expect, 1), **kw)
        if res["kept_index"] is None:            # more than was counted: take what it reports, never the overflowed buffer
            res = mutant_scan(target, q, hi, jij, sites, first=first, count=count, threshold=thr, capacity=res["n_kept"], **kw)
        return res["kept_index"], res["kept_energies"]

    lo, hi_ = ext["dh_min"], ext["dh_max"]
    thr, n_kept = -np.inf, total
    while n_kept > max_keep:
        edges = np.linspace(lo, hi_, _lib.SCAN_MAX_EDGES)
        edges[0], edges[-1] = lo, hi_
        edges = np.maximum.accumulate(np.clip(edges, lo, hi_))
        counts = mutant_scan(target, q, hi, jij, sites, edges=edges, **kw)["histogram"].astype(np.int64)
        tail = counts[::-1].cumsum()[::-1]           # tail[b]: combinations in bin b or above, i.e. with dH >= edges[b - 1]
        b = int(np.nonzero(tail >= top)[0].max())
        if b == 0:                                   # cannot happen while lo is a lower bound of the top values
            break
        thr, n_kept = float(edges[b - 1]), int(tail[b])
        if n_kept <= max_keep:
            break
        if b == edges.size:                          # that many sit at the maximum itself
            break
        upper = float(edges[b])
        if not np.nextafter(thr, np.inf) < upper or (thr == lo and upper == hi_):
            break                                    # the bin is one value wide, or did not narrow: ties
        lo, hi_ = thr, upper
    if n_kept <= max_keep:
        return best(*compact(thr, n_kept))
    idx, en = np.zeros(0, np.int64), np.zeros((0, 3))
    for first in range(0, total, int(chunk)):
        count = min(int(chunk), total - first)
        ci, ce = compact(thr, min(count, max_keep), first, count)
        idx, en = best(np.concatenate([idx, ci]), np.concatenate([en, ce]))
    return idx, en


# ---- inter-protein energies of two sequence sets, and matching by them (DESIGN_NEXT_ROWS.md section 9.23) ----
CROSS_BEST = np.dtype([("index", np.int64), ("best", np.float64), ("second", np.float64)])


def inter_blocks(jij, L, q, sites_a, sites_b, gauge="zero_sum"):
    """
    The inter block of a model for `plm.cross_energies`: a (len(sites_a), len(sites_b), q, q) float32 array with
    out[k, l, a, b] = J_ij(a, b) for i = sites_a[k], j = sites_b[l], from the canonical i<j blocks jij
    [L(L-1)/2][q][q] (a block is transposed where sites_a[k] > sites_b[l]).  The site lists are arbitrary but disjoint.
    The energy of the inter block alone depends on the gauge: a gauge change moves energy between the inter block, the
    intra blocks and the fields, and only their sum is invariant.  gauge="zero_sum" (the default) therefore brings every
    block to the zero-sum gauge, J'(a,b) = J(a,b) - mean_b J(a,.) - mean_a J(.,b) + mean J, in float64 before the one
    rounding to float32, which leaves the part of the energy that no single-site term can absorb; gauge=None takes the
    values as they are.  Pure numpy.
    """
    if gauge not in ("zero_sum", None):
        raise ValueError("gauge must be 'zero_sum' or None (got %r)" % (gauge,))
    L, q = int(L), int(q)
    jij = np.asarray(jij)
    if jij.size != L * (L - 1) // 2 * q * q:
        raise ValueError("jij must hold %d blocks of %d x %d values" % (L * (L - 1) // 2, q, q))
    jij = jij.reshape(L * (L - 1) // 2, q, q)
    sa, sb = np.asarray(sites_a, dtype=np.int64).ravel(), np.asarray(sites_b, dtype=np.int64).ravel()
    if sa.size < 1 or sb.size < 1:
        raise ValueError("each side needs one site at least")
    both = np.concatenate([sa, sb])
    if both.min() < 0 or both.max() >= L:
        raise ValueError("sites must lie in 0..%d" % (L - 1))
    if np.unique(both).size != both.size:
        raise ValueError("the two site lists must be disjoint and name no site twice")
    i, j = sa[:, None], sb[None, :]
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    blocks = jij[lo * (2 * L - lo - 1) // 2 + (hi - lo - 1)]                   # (LA, LB, q, q), [state at lo][state at hi]
    out = np.where((i < j)[:, :, None, None], blocks, blocks.transpose(0, 1, 3, 2))
    if gauge == "zero_sum":
        out = out.astype(np.float64)
        out = (out - out.mean(axis=3, keepdims=True) - out.mean(axis=2, keepdims=True)
               + out.mean(axis=(2, 3), keepdims=True))
    return np.ascontiguousarray(out, dtype=np.float32)


def _group_offsets(a_offsets, b_offsets, n_a, n_b):
    if (a_offsets is None) != (b_offsets is None):
        raise ValueError("a_offsets and b_offsets go together")
    if a_offsets is None:
        return np.array([0, n_a], np.int64), np.array([0, n_b], np.int64)
    ao = np.ascontiguousarray(a_offsets, dtype=np.int64).ravel()
    bo = np.ascontiguousarray(b_offsets, dtype=np.int64).ravel()
    if ao.size != bo.size or ao.size < 1:
        raise ValueError("a_offsets and b_offsets must hold n_groups + 1 entries each")
    return ao, bo


def cross_block_offsets(a_offsets, b_offsets):
    """Where each group's n_a(g) x n_b(g) block starts in the flat matrix of `cross_energies`: int64 [n_groups + 1]."""
    ao, bo = np.asarray(a_offsets, np.int64), np.asarray(b_offsets, np.int64)
    return np.concatenate([[0], np.cumsum(np.diff(ao) * np.diff(bo))]).astype(np.int64)


def cross_energies(jab, seqs_a, seqs_b, a_offsets=None, b_offsets=None, skip_state=None, matrix=True, best=True, device=0):
    """
    Inter-protein coupling energies E(s,t) = sum_i sum_j jab[i, j, a_si, b_tj] between rows of seqs_a (n_a x L_A states)
    and rows of seqs_b (n_b x L_B states); jab is the (L_A, L_B, q, q) float32 array of `inter_blocks`.  Group g pairs the
    rows a_offsets[g]:a_offsets[g+1] of A with the rows b_offsets[g]:b_offsets[g+1] of B (no offsets: one group, the
    all-against-all table).  A term whose state on either side equals skip_state is left out.  All sums are float64 in a
    fixed order: the same input gives the same bits.  Returns a dict:
      matrix         flat float64, the groups' row-major n_a(g) x n_b(g) blocks one after the other (None with matrix=False)
      block_offsets  int64 [n_groups + 1], where each block starts
      rows_best      structured array [n_a] (index, best, second): the row of B of the same group with the largest E (ties
                     to the smallest index; -1 without partners), that E, and the largest E over the other partners (-inf
                     where there is none);  cols_best [n_b] likewise for the rows of B.  None with best=False, which with
                     matrix=False leaves nothing to compute and is refused.
    """
    lib = _lib.load()
    jab = np.ascontiguousarray(jab, dtype=np.float32)
    if jab.ndim != 4 or jab.shape[2] != jab.shape[3]:
        raise ValueError("jab must be an (L_A, L_B, q, q) array")
    LA, LB, q, _ = jab.shape
    seqs_a, seqs_b = _msa(seqs_a), _msa(seqs_b)
    if seqs_a.shape[1] != LA or seqs_b.shape[1] != LB:
        raise ValueError("seqs_a must have %d columns and seqs_b %d (got %d and %d)" % (LA, LB, seqs_a.shape[1],
                                                                                         seqs_b.shape[1]))
    n_a, n_b = seqs_a.shape[0], seqs_b.shape[0]
    ao, bo = _group_offsets(a_offsets, b_offsets, n_a, n_b)
    if not matrix and not best:
        raise ValueError("nothing to compute: matrix=False and best=False")
    block_offsets = cross_block_offsets(ao, bo)
    opts = _lib.PlmCrossOpts(-1 if skip_state is None else int(skip_state), 1 if best else 0)
    m = np.empty(max(int(block_offsets[-1]), 0)) if matrix else None
    rows = np.empty(n_a, CROSS_BEST) if best else None
    cols = np.empty(n_b, CROSS_BEST) if best else None
    check(lib.plm_cross_energies(_ptr(jab), LA, LB, q, _ptr(seqs_a), n_a, _ptr(seqs_b), n_b, ao.size - 1, _ptr(ao), _ptr(bo),
                                 C.byref(opts), int(device), None, _ptr(m), _ptr(rows), _ptr(cols)))
    return dict(matrix=m, block_offsets=block_offsets, rows_best=rows, cols_best=cols)


def group_assignment(scores, a_offsets, b_offsets, maximize=True):
    """
    The exact rectangular linear assignment of every group of a score table laid out as the matrix of `cross_energies`:
    min(n_a(g), n_b(g)) pairs per group with the largest (or, maximize=False, smallest) total score.  Host code of the
    library, no device.  Returns (partner_of_a int64 [n_a]: the global row of B or -1, totals float64 [n_groups]).
    """
    lib = _lib.load()
    scores = np.ascontiguousarray(scores, dtype=np.float64).ravel()
    ao, bo = _group_offsets(a_offsets, b_offsets, 0, 0)
    if int((np.diff(ao) * np.diff(bo)).sum()) != scores.size:
        raise ValueError("scores must hold one value per pair of every group")
    partner = np.empty(max(int(ao[-1]), 0), np.int64)
    totals = np.empty(ao.size - 1)
    check(lib.plm_group_assignment(_ptr(scores), ao.size - 1, _ptr(ao), _ptr(bo), 1 if maximize else 0, _ptr(partner),
                                   _ptr(totals)))
    return partner, totals


# ---- the L-BFGS vector kernels, test-facing (diagnostic: tests/test_gpu_lbfgs_vectors.py) ----
def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _nan(shape, dtype):
    return np.full(shape, np.nan, dtype)


def lbfgs_gram(S, Y, x, xp, g, gp, direction, end, nst, nh, dinv=None, device=0):
    """plm_lbfgs_gram: the pair and the Gram pass behind a trial point.  S, Y: (m, n) ring slots (slot `end` is
    overwritten on the device only).  Returns (s_new, y_new, md [3 (2 nst + 2) + 1], ex [3])."""
    S, Y, x, xp, g, gp, direction, dinv = (_f32(a) for a in (S, Y, x, xp, g, gp, direction, dinv))
    m, n = S.shape
    s_new, y_new = _nan(n, np.float32), _nan(n, np.float32)
    md, ex = _nan(3 * (2 * nst + 2) + 1, np.float64), _nan(3, np.float64)
    check(_lib.load().plm_lbfgs_gram(n, int(nh), m, int(end), int(nst), _ptr(S), _ptr(Y), _ptr(x), _ptr(xp), _ptr(g),
                                     _ptr(gp), _ptr(direction), _ptr(dinv), device, _ptr(s_new), _ptr(y_new), _ptr(md),
                                     _ptr(ex)))
    return s_new, y_new, md, ex


def lbfgs_direction(S, Y, g, cs, cy, cg, stored, end, dinv=None, xacc=None, stp0=0.0, device=0):
    """plm_lbfgs_direction: the fused linear combination of the live pairs and g.  xacc given: the launch that also
    writes the first trial point; returns (dir, trial), else dir alone."""
    S, Y, g, dinv, xacc = (_f32(a) for a in (S, Y, g, dinv, xacc))
    cs, cy = _f64(cs), _f64(cy)
    m, n = S.shape
    out = _nan(n, np.float32)
    trial = None if xacc is None else _nan(n, np.float32)
    check(_lib.load().plm_lbfgs_direction(n, m, int(stored), int(end), _ptr(S), _ptr(Y), _ptr(g), _ptr(cs), _ptr(cy),
                                          float(cg), _ptr(dinv), _ptr(xacc), float(stp0), device, _ptr(out), _ptr(trial)))
    return out if xacc is None else (out, trial)


def lbfgs_multidot(V, q_index, b_index, dinv=None, wq=0, wb=0, device=0):
    """plm_lbfgs_multidot: <V[q], V[b]> for every query / basis index, (len(q_index), len(b_index)) float64"""
    V, dinv, q_index, b_index = _f32(V), _f32(dinv), _i32(q_index), _i32(b_index)
    nv, n = V.shape
    out = _nan((q_index.size, b_index.size), np.float64)
    check(_lib.load().plm_lbfgs_multidot(n, nv, _ptr(V), q_index.size, _ptr(q_index), b_index.size, _ptr(b_index),
                                         _ptr(dinv), int(wq), int(wb), device, _ptr(out)))
    return out


def lbfgs_dots(V, a_index, b_index, n=None, device=0):
    """plm_lbfgs_dots: <V[a], V[b]> over the first n entries (default: all) for 1..4 index pairs"""
    V, a_index, b_index = _f32(V), _i32(a_index), _i32(b_index)
    nv, stride = V.shape
    out = _nan(a_index.size, np.float64)
    check(_lib.load().plm_lbfgs_dots(stride, nv, _ptr(V), a_index.size, _ptr(a_index), _ptr(b_index),
                                     stride if n is None else int(n), device, _ptr(out)))
    return out


def lbfgs_lincomb(ca, a, cb=0.0, b=None, device=0):
    """plm_lbfgs_lincomb: ca a + cb b in float32 (b None: ca a)"""
    a, b = _f32(a), _f32(b)
    out = _nan(a.size, np.float32)
    check(_lib.load().plm_lbfgs_lincomb(a.size, float(ca), _ptr(a), float(cb), _ptr(b), device, _ptr(out)))
    return out


# ---- line search and pair history of the optimiser, host only (diagnostic: tests/test_linesearch_host.py) ----
def linesearch_run(phi, finit, dginit, step0):
    """plm_linesearch_run: the optimiser's More'-Thuente search on phi(stp) -> (f, f').  Returns (code, n_trials, stp,
    trace (n_trials, 3) of (stp, f - f0, f')); no device is touched."""
    def cfunc(stp, dphi, user):
        f, dphi[0] = phi(stp)
        return f
    code, count, stp = C.c_int32(0), C.c_int32(0), C.c_double(0)
    trace = _nan((_lib.LS_MAX_TRIALS, 3), np.float64)
    check(_lib.load().plm_linesearch_run(_lib.PHI_CB(cfunc), None, float(finit), float(dginit), float(step0),
                                         C.byref(code), C.byref(count), C.byref(stp), _ptr(trace)))
    return code.value, count.value, stp.value, trace[:count.value]


ADMIT_STORED, ADMIT_STRADDLE, ADMIT_SKIPPED, ADMIT_RESTARTED = 0, 1, 2, 3


def lbfgs_admit(state, md, vp=False, straddle=False):
    """plm_lbfgs_admit: the Gram rows of an accepted step's pair go into the history, then the pair is admitted or
    not.  state: dict(m, stored, end, anchored, SY, YDY (m, m), Sg, YDg (m), gDg, gg); md: the Gram pass's results
    [3 (2 nst + 2) + 1].  Returns (new state, outcome, copy_anchor); no device is touched."""
    m = int(state["m"])
    SY, YDY, Sg, YDg = (_f64(state[k]).copy() for k in ("SY", "YDY", "Sg", "YDg"))
    md = _f64(md)
    stored, end, anchored = (C.c_int32(int(state[k])) for k in ("stored", "end", "anchored"))
    gDg, gg = C.c_double(state["gDg"]), C.c_double(state["gg"])
    outcome, copy_anchor = C.c_int32(-1), C.c_int32(-1)
    nst = min(m, stored.value + 1)
    if SY.shape != (m, m) or YDY.shape != (m, m) or Sg.shape != (m,) or YDg.shape != (m,) or md.size != 3 * (2 * nst + 2) + 1:
        raise ValueError("history arrays or md of the wrong shape")
    check(_lib.load().plm_lbfgs_admit(m, C.byref(stored), C.byref(end), C.byref(anchored), _ptr(SY), _ptr(YDY), _ptr(Sg),
                                      _ptr(YDg), C.byref(gDg), C.byref(gg), _ptr(md), 2 * nst + 2, nst, int(bool(vp)),
                                      int(bool(straddle)), C.byref(outcome), C.byref(copy_anchor)))
    new = dict(m=m, stored=stored.value, end=end.value, anchored=bool(anchored.value), SY=SY, YDY=YDY, Sg=Sg, YDg=YDg,
               gDg=gDg.value, gg=gg.value)
    return new, outcome.value, bool(copy_anchor.value)


FLAG_IGNORE_GAPS = 2
FLAG_SHARDED_STATE = 4
FLAG_PRECOND = 8
FLAG_JOINT_LBFGS = 16
FLAG_COMPACT_GAPS = 1024


class _IterationCallback:
    """The plm_iter_cb of one fit: collects the iteration table, forwards to the user's callback, and turns an exception
    raised while Python code runs inside the callback -- the user's own, or the SystemExit / KeyboardInterrupt of a signal
    handler (evcouplings/utils/pipeline.py:476-545 installs handlers that call sys.exit; Python runs a pending handler
    the next time the main thread executes bytecode, which during a fit is here) -- into a cancellation: the library
    stops after this iteration (status "interrupted"), and `reraise()` raises the exception where the fit was called.
    ctypes would otherwise print and swallow it, and the fit would run on."""

    def __init__(self, callback=None):
        self.table, self.callback, self.pending = [], callback, None
        self.cfunc = _lib.ITER_CB(self._call)

    def _call(self, it, secs, cond, fx, nll, nh, ne, user):
        try:
            self.table.append((it, secs, cond, fx, nll, nh, ne))
            if self.callback is not None:
                self.callback(it, secs, cond, fx, nll, nh, ne)
            return 0
        except BaseException as exc:      # incl. SystemExit / KeyboardInterrupt: never let one cross the C boundary
            self.pending = exc
            return 1

    def reraise(self):
        if self.pending is not None:
            exc, self.pending = self.pending, None
            raise exc


def _wrap_collective(collective):
    """python callable(op, send_ptr, recv_ptr, send_counts, recv_counts, n_shards, shard) -> 0  =>  C callback"""
    def _cb(op, send, recv, scounts, rcounts, n, shard, user):
        try:
            return int(collective(int(op), send, recv, [int(scounts[k]) for k in range(n)],
                                  [int(rcounts[k]) for k in range(n)] if op in (_lib.COLL_ALLTOALL, _lib.COLL_BROADCAST) else None,
                                  int(n), int(shard)))
        except Exception as exc:   # never let an exception cross the C boundary
            import sys
            print("plm collective failed: %r" % (exc,), file=sys.stderr)
            return 1
    return _lib.COLLECTIVE_CB(_cb)


def _embed_gaps(x, L, q):
    """(q-1)-state canonical vector -> q-state layout with zeros for state 0."""
    qn = q - 1
    x = np.asarray(x, dtype=np.float32)
    npair = L * (L - 1) // 2
    out_h = np.zeros((L, q), np.float32)
    out_h[:, 1:] = x[:L * qn].reshape(L, qn)
    out_j = np.zeros((npair, q, q), np.float32)
    out_j[:, 1:, 1:] = x[L * qn:].reshape(npair, qn, qn)
    return np.concatenate([out_h.ravel(), out_j.ravel()])


def _strip_gaps(x, L, q):
    """q-state canonical vector -> (q-1)-state layout (drops every entry that involves state 0)."""
    npair = L * (L - 1) // 2
    h = x[:L * q].reshape(L, q)[:, 1:]
    j = x[L * q:].reshape(npair, q, q)[:, 1:, 1:]
    return np.concatenate([h.ravel(), j.ravel()]).astype(np.float32)


def _problem(msa, q, theta_id, scale, lambda_h, lambda_j, max_iter, epsilon, lbfgs_m, n_shards, shard,
             ignore_gaps=False, sharded_state=False, precond=False, joint=False, conventions=0, lambda_group=0.0):
    N, L = msa.shape
    p = PlmProblem()
    p.n_seqs, p.n_sites, p.n_states = N, L, q
    p.msa = msa.ctypes.data
    p.theta_id, p.scale = float(theta_id), float(scale)
    p.lambda_h, p.lambda_j = float(lambda_h), float(lambda_j)
    p.lambda_group = float(lambda_group or 0.0)
    p.max_iter, p.epsilon, p.lbfgs_m = int(max_iter), float(epsilon), int(lbfgs_m)
    p.n_shards, p.shard = int(n_shards), int(shard)
    p.flags = ((FLAG_IGNORE_GAPS if ignore_gaps else 0) | (FLAG_SHARDED_STATE if sharded_state else 0) |
               (FLAG_PRECOND if precond else 0) | (FLAG_JOINT_LBFGS if joint else 0) | (int(conventions) & CONV_MASK))
    return p


def fit(msa, q=21, theta_id=0.8, scale=1.0, lambda_h=0.01, lambda_j=None, max_iter=100,
        epsilon=1e-3, lbfgs_m=6, device=0, stream=0, callback=None, n_shards=1, shard=0,
        exchange=None, want_fij=True, ignore_gaps=False, collective=None, precond=False, joint=False, conventions=0,
        rccl_id=None, lambda_group=0.0):
    """
    Whole couplings inference: reweight -> marginals -> L-BFGS -> scores.

    callback(iter, secs, cond, fx, nll, norm_h, norm_e) is called once per iteration.
    exchange(dev_ptr, bytes_per_shard, n_shards, shard) -> 0 implements the all-gather of
    the site-sharded gradient slabs (see evcouplings_amd.dist) and is required iff n_shards > 1
    in the replicated mode; pass `collective` instead to run the sharded-state mode
    (parameters, gradient and optimiser state split across the shards, see evcouplings_amd.dist), or `rccl_id`
    (the bytes of rccl_unique_id() made on rank 0) to run that mode with the collectives issued by the library
    itself over RCCL on its own stream (one process per GPU, rank = shard).
    ignore_gaps=True is plmc -g (tools.py:222-224): state 0 is excluded from the model and every
    returned array has q-1 states (fi, hi: (L, q-1); fij, jij: (pairs, q-1, q-1)).
    joint=True optimises fields and couplings jointly with L-BFGS as libLBFGS-based plmc does
    (PLM_FLAG_JOINT_LBFGS) instead of the default variable projection (fields solved by Newton for every trial
    couplings, ~10-20x fewer iterations to the same optimum); precond=True gives L-BFGS a diagonal initial Hessian
    (PLM_FLAG_PRECOND).  conventions: PLM_CONV_* bits (CONV_* above), the selectable conventions of plmc.
    lambda_group: run_plmc's lambda_g (plmc -lg), the group regulariser lambda_group * sum_{i<j} sqrt(|J_ij|^2 + 1e-8).
    Returns a dict of numpy arrays and scalars.
    """
    lib = _lib.load()
    msa = _msa(msa)
    N, L = msa.shape
    if lambda_j is None:
        lambda_j = default_lambda_j(L, q - 1 if ignore_gaps else q)
    npair = L * (L - 1) // 2
    qo = q - 1 if ignore_gaps else q       # -g: the library returns the (q-1)-state arrays (PLM_FLAG_COMPACT_GAPS)
    out = dict(
        weights=np.zeros(N, np.float32), fi=np.zeros((L, qo), np.float32),
        fij=np.zeros((npair, qo, qo), np.float32) if want_fij else None,
        hi=np.zeros((L, qo), np.float32), jij=np.zeros((npair, qo, qo), np.float32),
        fn=np.zeros((L, L), np.float32), cn=np.zeros((L, L), np.float32))
    res = PlmResult()
    for k in ("weights", "fi", "fij", "hi", "jij", "fn", "cn"):
        setattr(res, k, None if out[k] is None else out[k].ctypes.data)
    icb = _IterationCallback(callback)
    cb, table = icb.cfunc, icb.table
    if exchange is not None:
        xcb = _lib.EXCHANGE_CB(lambda buf, nbytes, ns, sh, user: int(exchange(buf, nbytes, ns, sh)))
    else:
        xcb = C.cast(None, _lib.EXCHANGE_CB)
    prob = _problem(msa, q, theta_id, scale, lambda_h, lambda_j, max_iter, epsilon, lbfgs_m,
                    n_shards, shard, ignore_gaps, sharded_state=collective is not None or rccl_id is not None,
                    precond=precond, joint=joint, conventions=conventions, lambda_group=lambda_group)
    if ignore_gaps:
        prob.flags |= FLAG_COMPACT_GAPS
    if rccl_id is not None:
        idbuf = C.create_string_buffer(bytes(rccl_id), RCCL_ID_BYTES)
        check(lib.plm_fit_sharded_rccl(C.byref(prob), C.byref(res), int(device), C.c_void_p(int(stream) or None), cb,
                                       None, idbuf))
    elif collective is not None:
        ccb = _wrap_collective(collective)
        check(lib.plm_fit_sharded(C.byref(prob), C.byref(res), int(device), C.c_void_p(int(stream) or None), cb,
                                  None, ccb, None))
    else:
        check(lib.plm_fit(C.byref(prob), C.byref(res), int(device), C.c_void_p(int(stream) or None), cb,
                          None, xcb, None))
    icb.reraise()      # an exception (or a signal handler's SystemExit) met inside the iteration callback
    out.update(
        n_eff=float(res.n_eff), iters=int(res.iters_done), n_evals=int(res.n_evals),
        status=int(res.status), status_msg=res.status_msg.decode("ascii", "replace"),
        fx=float(res.fx), table=table, lambda_j=float(lambda_j),
        seconds=dict(reweight=res.seconds_reweight, marginals=res.seconds_marginals,
                     optimize=res.seconds_optimize, total=res.seconds_total))
    return out


RCCL_ID_BYTES = 128


def rccl_unique_id():
    """plm_rccl_unique_id: the communicator id rank 0 creates and every rank attaches (128 bytes)."""
    buf = C.create_string_buffer(RCCL_ID_BYTES)
    check(_lib.load().plm_rccl_unique_id(buf))
    return buf.raw


def rccl_version():
    """NCCL version code of the RCCL the library resolved at run time (0: none found)."""
    return int(_lib.load().plm_rccl_runtime_version())


def rccl_probe(rccl_id, nranks, rank, device=0, stream=0):
    """plm_rccl_probe: every rank forms the communicator, exchanges an all-to-all and an all-reduce, destroys it; raises
    on this rank if anything failed"""
    idbuf = C.create_string_buffer(bytes(rccl_id), RCCL_ID_BYTES)
    check(_lib.load().plm_rccl_probe(idbuf, int(nranks), int(rank), int(device), C.c_void_p(int(stream) or None)))


def rccl_probe_local(nranks, device=0, stream=0):
    """plm_rccl_probe_local: the steps of the probe that can fail on one rank alone (no communicator call)"""
    check(_lib.load().plm_rccl_probe_local(int(nranks), int(device), C.c_void_p(int(stream) or None)))


def rccl_selftest(device=0, stream=0):
    """every collective of the sharded-state mode on a one-rank communicator; raises on any failure"""
    check(_lib.load().plm_rccl_selftest(int(device), C.c_void_p(int(stream) or None)))


class PlmContext:
    """Alignment resident in HBM; step-wise access for benchmarks and the multi-GPU host."""

    def __init__(self, msa, q=21, theta_id=0.8, scale=1.0, lambda_h=0.01, lambda_j=None,
                 max_iter=100, epsilon=1e-3, lbfgs_m=6, device=0, stream=0, n_shards=1, shard=0,
                 ignore_gaps=False, sharded_state=False, precond=False, joint=False, conventions=0, lambda_group=0.0):
        self.lib = _lib.load()
        msa = _msa(msa)
        self.N, self.L = msa.shape
        self.q = q
        self.ignore_gaps = bool(ignore_gaps)
        self.qm = q - 1 if ignore_gaps else q      # model states (layout of x, g, fi, fij at this API)
        self.lambda_j = default_lambda_j(self.L, self.qm) if lambda_j is None else lambda_j
        prob = _problem(msa, q, theta_id, scale, lambda_h, self.lambda_j, max_iter, epsilon, lbfgs_m,
                        n_shards, shard, ignore_gaps, sharded_state, precond, joint, conventions, lambda_group)
        self._h = C.c_void_p()
        check(self.lib.plm_ctx_create(C.byref(prob), int(device), C.c_void_p(int(stream) or None),
                                      C.byref(self._h)))
        self._keep = []

    def close(self):
        if self._h:
            self.lib.plm_ctx_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_exchange(self, exchange):
        cb = _lib.EXCHANGE_CB(lambda buf, nbytes, ns, sh, user: int(exchange(buf, nbytes, ns, sh)))
        self._keep.append(cb)
        check(self.lib.plm_ctx_set_exchange(self._h, cb, None))

    def set_collective(self, collective):
        cb = _wrap_collective(collective)
        self._keep.append(cb)
        check(self.lib.plm_ctx_set_collective(self._h, cb, None))

    def attach_rccl(self, rccl_id):
        """collectives of the sharded-state mode from the library itself (RCCL on the context's stream); a collective
        call: every rank, with the id rank 0 made (rccl_unique_id)"""
        idbuf = C.create_string_buffer(bytes(rccl_id), RCCL_ID_BYTES)
        check(self.lib.plm_ctx_attach_rccl(self._h, idbuf))

    def set_options(self, max_iter=-1, epsilon=-1.0, lbfgs_m=-1):
        check(self.lib.plm_ctx_set_options(self._h, int(max_iter), float(epsilon), int(lbfgs_m)))

    def _set_max_iter(self, k):
        self.set_options(max_iter=k)

    def native_size(self):
        return int(self.lib.plm_ctx_native_size(self._h))

    def reweight(self):
        check(self.lib.plm_ctx_reweight(self._h))
        return self.weights()

    def set_weights(self, w):
        w = np.ascontiguousarray(w, dtype=np.float32)
        assert w.size == self.N
        check(self.lib.plm_ctx_set_weights(self._h, _ptr(w)))

    def weights(self):
        w = np.zeros(self.N, np.float32)
        counts = np.zeros(self.N, np.int32)
        neff = C.c_float(0)
        check(self.lib.plm_ctx_get_weights(self._h, _ptr(w), _ptr(counts), C.byref(neff)))
        return w, counts, neff.value

    def marginals(self, pairs=True):
        fi = np.zeros((self.L, self.q), np.float32)
        fij = np.zeros((self.L * (self.L - 1) // 2, self.q, self.q), np.float32) if pairs else None
        check(self.lib.plm_ctx_marginals(self._h, _ptr(fi), _ptr(fij)))
        if self.ignore_gaps:
            fi = fi[:, 1:].copy()
            fij = None if fij is None else fij[:, 1:, 1:].copy()
        return fi, fij

    def set_x(self, x=None):
        if x is not None:
            x = np.ascontiguousarray(x, dtype=np.float32)
            assert x.size == n_params(self.L, self.qm)
            if self.ignore_gaps:
                x = _embed_gaps(x, self.L, self.q)
        check(self.lib.plm_ctx_set_x(self._h, _ptr(x)))

    def get_x(self):
        x = np.zeros(n_params(self.L, self.q), np.float32)
        check(self.lib.plm_ctx_get_x(self._h, _ptr(x)))
        return _strip_gaps(x, self.L, self.q) if self.ignore_gaps else x

    def get_g(self):
        g = np.zeros(n_params(self.L, self.q), np.float32)
        check(self.lib.plm_ctx_get_g(self._h, _ptr(g)))
        return _strip_gaps(g, self.L, self.q) if self.ignore_gaps else g

    def eval(self, sync=True):
        if not sync:
            check(self.lib.plm_ctx_eval(self._h, None, None))
            return None
        fx, nll = C.c_double(0), C.c_double(0)
        check(self.lib.plm_ctx_eval(self._h, C.byref(fx), C.byref(nll)))
        return fx.value, nll.value

    def optimize(self, callback=None):
        res = PlmResult()
        icb = _IterationCallback(callback)
        table = icb.table
        check(self.lib.plm_ctx_optimize(self._h, icb.cfunc, None, C.byref(res)))
        icb.reraise()
        return dict(iters=int(res.iters_done), n_evals=int(res.n_evals), status=int(res.status),
                    status_msg=res.status_msg.decode("ascii", "replace"), fx=float(res.fx),
                    seconds=float(res.seconds_optimize), table=table)

    def scores(self):
        fn = np.zeros((self.L, self.L), np.float32)
        cn = np.zeros((self.L, self.L), np.float32)
        check(self.lib.plm_ctx_scores(self._h, _ptr(fn), _ptr(cn)))
        return fn, cn

    def solver_stats(self):
        """field-solver statistics of the last optimize() on this context (plm_ctx_solver_stats)"""
        out = np.zeros(_lib.S_COUNT, np.float64)
        check(self.lib.plm_ctx_solver_stats(self._h, _ptr(out)))
        ev, gv = max(1.0, out[0]), max(1.0, out[4])
        return {"evaluations": int(out[0]), "field_ms_per_evaluation": out[1] / ev, "passes_per_evaluation": out[2] / ev,
                "chains_continued_by_host": int(out[3]),
                # the two GEMMs as the fit ran them (HIP events inside the fit; plain arithmetic only)
                "gemm_evaluations": int(out[4]), "forward_ms_per_evaluation": out[5] / gv, "backward_ms_per_evaluation": out[6] / gv}

    # ---- the field solver, test-facing (diagnostic: tests/test_gpu_field_solver.py) ----
    def field_dims(self):
        """Q (the instantiated alphabet), sequence tiles of 256, 16-site blocks: the shapes of the solver's raw buffers"""
        q = self.q
        Q = 4 if q <= 4 else 5 if q == 5 else 20 if q <= 20 else 21 if q == 21 else 32
        return Q, (self.N + 255) // 256, (self.L + 15) // 16

    def field_position(self, role, accurate=False, update=True, prefill=False):
        """plm_ctx_field_position: one unchained position of the field solver at the current x in the role "stats",
        "hessian" or "residual"; the device buffers as they are (arrays in the Q-state layout of field_dims)"""
        Q, T, B = self.field_dims()
        S, NH = 16 * B, Q * (Q + 1) // 2
        out = dict(gpart=np.zeros((B, T, 16, Q)), dpart=np.zeros((B, T, 16, Q)), hpart=np.zeros((B, T, 16, NH), np.float32),
                   hcnt=np.zeros((S, Q)), hinv=np.zeros((S, Q, Q)), g2_site=np.zeros(S), g2_sum=np.zeros(1),
                   h64=np.zeros((2, S, Q)), nll_part=np.zeros((B, T)))
        buf = _lib.PlmFieldBuffers()
        for k, v in out.items():
            setattr(buf, k, v.ctypes.data)
        buf.n_gpart, buf.n_hpart, buf.n_hcnt, buf.n_hinv = out["gpart"].size, out["hpart"].size, out["hcnt"].size, out["hinv"].size
        buf.n_g2_site, buf.n_h64, buf.n_nll_part = S, out["h64"].size, out["nll_part"].size
        role = {"stats": _lib.FIELD_ROLE_STATS, "hessian": _lib.FIELD_ROLE_HESSIAN, "residual": _lib.FIELD_ROLE_RESIDUAL}[role]
        check(self.lib.plm_ctx_field_position(self._h, role, int(bool(accurate)), int(bool(update)), int(bool(prefill)),
                                              C.byref(buf)))
        return out

    def field_solve(self, tol, vp_c_prev=3, invalidate=False, accurate=False):
        """plm_ctx_field_solve: the field solver's chain of one variable-projection evaluation at the current x"""
        Q, T, B = self.field_dims()
        fields = np.zeros((16 * B, Q))
        res = _lib.PlmFieldSolve()
        check(self.lib.plm_ctx_field_solve(self._h, float(tol), int(vp_c_prev), int(bool(invalidate)), int(bool(accurate)),
                                           C.byref(res), _ptr(fields), fields.size))
        return dict(gh2=res.gh2, fx=res.fx, nll=res.nll, passes=res.passes, done=bool(res.done),
                    continuations=res.continuations, final_skip=res.final_skip, want_rt=res.want_rt, cur=res.cur,
                    state_passes=res.state_passes, c_prev_next=res.c_prev_next, hist=np.array(res.hist[:]),
                    quiet=np.array(res.quiet[:], np.uint8), fields=fields)

    def precond_diagonal(self):
        """plm_ctx_precond_diagonal: the H0 diagonal of the preconditioned L-BFGS (diagnostic:
        tests/test_gpu_lbfgs_vectors.py), canonical layout over all q states -- state 0 included when gaps are ignored"""
        out = np.full(n_params(self.L, self.q), np.nan, np.float32)
        check(self.lib.plm_ctx_precond_diagonal(self._h, _ptr(out)))
        return out

    def time_field_positions(self, reps=5):
        """ms of one Hessian position and of the closing (residual-writing) position of the field solver's chain on this
        context's site blocks (plm_ctx_time_field_positions; call time_kernels first)"""
        ms = np.zeros(2, np.float32)
        check(self.lib.plm_ctx_time_field_positions(self._h, int(reps), _ptr(ms)))
        return {"hessian_position": float(ms[0]), "closing_position": float(ms[1])}

    def time_kernels(self, reps=5):
        ms = np.zeros(_lib.K_COUNT, np.float32)
        check(self.lib.plm_ctx_time_kernels(self._h, int(reps), _ptr(ms)))
        names = ["expand", "forward", "backward", "assemble", "total", "reweight", "fields", "forward_accurate", "lbfgs_vector"]
        return dict(zip(names, ms.tolist()))
