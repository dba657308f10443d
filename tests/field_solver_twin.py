"""
numpy float64 twin of the field solver of the variable-projection fit (DESIGN.md sections 2c and 4.8; kernels
k_site_counts, k_hpass, k_hsolve of csrc/plm_kernels.hip).  TEST INFRASTRUCTURE ONLY, self-contained.

Everything lives in the layout the kernels run in: Q states = the instantiated alphabet (4 / 5 / 20 / 21 / 32) that an
alphabet of q symbols is padded to with dead states, state 0 not a model state in gap mode; sequence tiles of TILE = 256,
every SAMPLE-th of which carries Hessian sums.

  potentials        HJ[s, i, a] = sum_{j != i} J_ij(a, x_sj) from the canonical parameter vector
  tile_sums         per tile: gradient sums  sum w (P - [x = a]),  diagonal sums  sum w P_a^2,  weighted counts,
                    -sum w log P_x, and on the sampled tiles the Hessian sums  sum w P P^T  (what a pass delivers);
                    dtype = float32 gives the yardstick of the GPU tests: f32 potentials and softmax, f64 accumulation
  reduce_partials   the reductions of k_hsolve over per-tile partials -- the twin's own or the GPU's raw buffers
  assemble_hessian  exact diagonal, three symmetric Sinkhorn sweeps of the off-diagonal part, + 2 lambda_h, + 1e-12 term
  gauss_jordan      the inverse as k_hsolve forms it (no pivoting)
  newton_step       the step, scaled so that no field moves by more than CAP
  solve_exact       the per-site Newton iteration with the exact Hessian: h*(J)
"""
import numpy as np

TILE = 256
SAMPLE = 32
CAP = 3.0


def q_template(q):
    return 4 if q <= 4 else 5 if q == 5 else 20 if q <= 20 else 21 if q == 21 else 32


def n_tiles(N):
    return (N + TILE - 1) // TILE


def n_sampled(T):
    return (T + SAMPLE - 1) // SAMPLE


def live_states(q, gap, Q=None):
    Q = Q or q_template(q)
    live = np.zeros(Q, bool)
    live[(1 if gap else 0):q] = True
    return live


def unpack(x, L, q, gap=False):
    """canonical [h | J_ij (i < j)] (gap mode: over the q - 1 model states) -> h (L, Q), dense J (L, L, Q, Q) in the
    padded layout: dead states, and state 0 in gap mode, hold zeros"""
    Q, qm, a0 = q_template(q), (q - 1 if gap else q), (1 if gap else 0)
    x = np.asarray(x, np.float64)
    h = np.zeros((L, Q))
    h[:, a0:q] = x[:L * qm].reshape(L, qm)
    J = np.zeros((L, L, Q, Q))
    iu, ju = np.triu_indices(L, 1)
    blocks = x[L * qm:].reshape(L * (L - 1) // 2, qm, qm)
    J[iu, ju, a0:q, a0:q] = blocks
    J[ju, iu, a0:q, a0:q] = blocks.transpose(0, 2, 1)
    return h, J


def potentials(msa, x, q, gap=False):
    """-> (HJ (N, L, Q), h (L, Q)).  A gapped neighbour (gap mode, x_sj = 0) contributes nothing: its row of J is zero."""
    msa = np.asarray(msa)
    N, L = msa.shape
    h, J = unpack(x, L, q, gap)
    HJ = np.zeros((N, L, J.shape[2]))
    for j in range(L):
        # J[i, j, a, x_sj] for every i: (L, Q, N) -> (N, L, Q); J[j, j] = 0
        HJ += J[:, j][:, :, msa[:, j]].transpose(2, 0, 1)
    return HJ, h


def _softmax(HJ, h, live, dtype):
    H = HJ.astype(dtype) + h.astype(dtype)[None]
    H = np.where(live, H, dtype(-np.inf))
    H = H - H.max(axis=2, keepdims=True)
    E = np.exp(H)
    Z = E.sum(axis=2, keepdims=True, dtype=dtype)
    return E / Z, H - np.log(Z)


def tile_sums(HJ, h, msa, w, q, gap=False, dtype=np.float64):
    """What the passes deliver, per sequence tile.  -> dict of float64 arrays
         g, d, cnt (T, L, Q); nll (T, L); M (n_sampled, L, Q, Q): the Hessian sums of tiles 0, SAMPLE, 2 SAMPLE, ... -- above
         21 states over the first 64 sequences of the tile only (two of its eight waves; k_hsolve scales by 4)."""
    msa = np.asarray(msa)
    N, L = msa.shape
    Q = HJ.shape[2]
    live = live_states(q, gap, Q)
    dtype = np.dtype(dtype).type
    P, logP = _softmax(HJ, h, live, dtype)
    ws = np.asarray(w, np.float32).astype(np.float64)[:, None] * np.ones((1, L))
    if gap:
        ws = ws * (msa != 0)
    sidx, iidx = np.arange(N)[:, None], np.arange(L)[None, :]
    starts = np.arange(0, N, TILE)
    R = P.copy()
    R[sidx, iidx, msa] -= dtype(1)                    # P - [x = a], in the working precision
    out = {"g": np.add.reduceat(ws[:, :, None] * R.astype(np.float64), starts, axis=0)}
    del R
    out["d"] = np.add.reduceat(ws[:, :, None] * (P * P).astype(np.float64), starts, axis=0)
    X = np.zeros((N, L, Q))
    X[sidx, iidx, msa] = 1.0
    out["cnt"] = np.add.reduceat(ws[:, :, None] * X, starts, axis=0)
    del X
    lpx = logP[sidx, iidx, msa].astype(np.float64)     # (a gapped site of gap mode has no observed model state: weight 0)
    out["nll"] = -np.add.reduceat(np.where(ws > 0, ws * np.where(ws > 0, lpx, 0.0), 0.0), starts, axis=0)
    T = len(starts)
    M = np.zeros((n_sampled(T), L, Q, Q))
    for k in range(n_sampled(T)):
        lo = k * SAMPLE * TILE
        hi = min(N, lo + (64 if Q > 21 else TILE))
        Pt = P[lo:hi].astype(np.float64)
        M[k] = np.einsum("si,sia,sib->iab", ws[lo:hi], Pt, Pt)
    out["M"] = M
    out["wsum"] = np.add.reduceat(np.asarray(w, np.float32).astype(np.float64), starts)
    return out


def field_gradient(sums, h, lam, live):
    """d f / d h (L, Q) from per-tile gradient sums"""
    return np.where(live, sums["g"].sum(axis=0) + 2.0 * lam * h, 0.0)


def exact_hessian(HJ, h, msa, w, q, lam, gap=False):
    """diag(m) - M + 2 lambda I per site (L, Q, Q), every sequence in M; dead states: 2 lambda on the diagonal"""
    msa = np.asarray(msa)
    Q = HJ.shape[2]
    P, _ = _softmax(HJ, h, live_states(q, gap, Q), np.float64)
    ws = np.asarray(w, np.float32).astype(np.float64)[:, None] * np.ones((1, msa.shape[1]))
    if gap:
        ws = ws * (msa != 0)
    m = np.einsum("si,sia->ia", ws, P)
    M = np.einsum("si,sia,sib->iab", ws, P, P)
    H = -M
    idx = np.arange(Q)
    H[:, idx, idx] += m + 2.0 * lam
    return H


# ---- layouts of the GPU's raw buffers ------------------------------------------------------------------------------
def sites_of(part):
    """[block][tile][16][X] -> [site = 16 block + r][tile][X]"""
    B, T, _, X = part.shape
    return part.transpose(0, 2, 1, 3).reshape(B * 16, T, X)


def tri_to_full(tri, Q):
    """row-major upper triangle (..., Q (Q + 1) / 2) -> symmetric (..., Q, Q)"""
    iu, ju = np.triu_indices(Q)
    full = np.zeros(tri.shape[:-1] + (Q, Q), tri.dtype)
    full[..., iu, ju] = tri
    full[..., ju, iu] = tri
    return full


def full_to_tri(full):
    Q = full.shape[-1]
    iu, ju = np.triu_indices(Q)
    return full[..., iu, ju]


def partials_from_sums(sums, Q):
    """the twin's own per-tile sums in the shapes reduce_partials takes: gp, dp (L, T, Q), hp (L, T, NH) with the
    Hessian sums on the sampled tiles and, as the passes leave them, the diagonal sums only where k_hsolve reads them"""
    T, L = sums["g"].shape[:2]
    gp = sums["g"].transpose(1, 0, 2).copy()
    dp = sums["d"].transpose(1, 0, 2).copy()
    hp = np.zeros((L, T, Q * (Q + 1) // 2))
    hp[:, ::SAMPLE] = full_to_tri(sums["M"]).transpose(1, 0, 2)
    return gp, dp, hp


# ---- the reductions of k_hsolve --------------------------------------------------------------------------------------
def _lane_sum(v):
    """v (S, T, Q): lane l adds tiles l, l + 64, ... in order, then the 64 lane sums meet in an xor butterfly (32 ... 1)"""
    S, T, Q = v.shape
    lanes = np.zeros((S, 64, Q))
    for t0 in range(0, T, 64):
        n = min(64, T - t0)
        lanes[:, :n] += v[:, t0:t0 + n]
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, idx ^ o]
    return lanes[:, 0]


def reduce_partials(gp, dp, hp, Q):
    """gp, dp (S, T, Q) f64, hp (S, T, NH) -> st (S, Q) gradient sums, Mt (S, Q, Q) scaled sampled Hessian sums, Md (S, Q)
    exact diagonal sums -- up to 21 states taken from the triangle on the sampled tiles, from dp on the others"""
    S, T, _ = gp.shape
    nsamp = n_sampled(T)
    st = _lane_sum(gp)
    v = np.zeros((S, hp.shape[2]))
    for k in range(nsamp):
        v = v + hp[:, k * SAMPLE].astype(np.float64)
    Mt = tri_to_full(v * (float(T) / nsamp) * (4.0 if Q > 21 else 1.0), Q)
    src = np.array(dp, np.float64)
    if Q <= 21:
        diag = np.array([k * Q - k * (k - 1) // 2 for k in range(Q)])
        src[:, ::SAMPLE] = hp[:, ::SAMPLE][:, :, diag].astype(np.float64)
    Md = _lane_sum(src)
    return st, Mt, Md


def assemble_hessian(st, Mt, Md, cnt, lam):
    """(S, Q, Q): off-diagonal -X with X = D Mt D after three Sinkhorn sweeps to the row sums m_a - M_aa, diagonal
    rowsum(X) + 2 lambda + 1e-12 (1 + rowsum(X))"""
    S, Q = st.shape
    Hm = -np.array(Mt, np.float64)
    idx = np.arange(Q)
    mv = np.maximum(0.0, np.maximum(0.0, st + cnt) - Md)
    Hm[:, idx, idx] = 0.0
    Dv = np.ones((S, Q))
    for _ in range(3):
        rs = -np.einsum("sab,sb->sa", Hm, Dv) * Dv
        with np.errstate(divide="ignore", invalid="ignore"):
            Dv = np.where(rs > 0.0, Dv * np.sqrt(mv / np.where(rs > 0.0, rs, 1.0)), 0.0)
    Hm = Hm * Dv[:, :, None] * Dv[:, None, :]
    rowsum = -Hm.sum(axis=2)
    Hm[:, idx, idx] += rowsum + 2.0 * lam + 1e-12 * (1.0 + rowsum)
    return Hm


def gauss_jordan(H):
    """inverse of (S, Q, Q) by Gauss-Jordan without pivoting on [H | I], the operations of k_hsolve"""
    S, Q, _ = H.shape
    A = np.concatenate([np.array(H, np.float64), np.broadcast_to(np.eye(Q), (S, Q, Q))], axis=2)
    for p in range(Q):
        A[:, p] *= (1.0 / A[:, p, p])[:, None]
        f = A[:, :, p].copy()
        f[:, p] = 0.0
        A -= f[:, :, None] * A[:, p][:, None, :]
    return A[:, :, Q:].copy()


def inverse_gap(H, inv=None):
    """per site: how far Gauss-Jordan and numpy.linalg.inv of the same matrix are apart (largest entry), never below one
    rounding of the largest entry of the inverse"""
    inv = gauss_jordan(H) if inv is None else inv
    ref = np.linalg.inv(H)
    gap = np.abs(inv - ref).max(axis=(1, 2))
    return np.maximum(gap, 2.0 ** -52 * np.abs(ref).max(axis=(1, 2)))


def newton_step(h, gr, inv, a0):
    """-> (h_new, cap): h - cap H^-1 g with cap = min(1, CAP / max |dh|) per site"""
    dh = np.einsum("sab,sb->sa", inv, gr)
    dh[:, :a0] = 0.0
    mxs = np.abs(dh).max(axis=1)
    cap = np.where(mxs > CAP, CAP / np.where(mxs > 0, mxs, 1.0), 1.0)
    return h - cap[:, None] * dh, cap


def predict_solve(gp, dp, hp, cnt, h, lam, a0, full, inv_prev=None, update=True):
    """what k_hsolve (no chain state) makes of a pass's partials at the fields h (S, Q): dict with gr, g2_site, g2_sum,
    H / inv (fresh when full, else inv_prev), h_new, cap"""
    S, Q = h.shape
    st, Mt, Md = reduce_partials(gp, dp, hp, Q)
    gr = st + 2.0 * lam * h
    gr[:, :a0] = 0.0
    out = {"gr": gr, "g2_site": (gr * gr).sum(axis=1)}
    out["g2_sum"] = out["g2_site"].sum()
    if full:
        out["H"] = assemble_hessian(st, Mt, Md, cnt, lam)
        out["inv"] = gauss_jordan(out["H"])
    else:
        out["inv"] = inv_prev
    if update:
        out["h_new"], out["cap"] = newton_step(h, gr, out["inv"], a0)
    else:
        out["h_new"], out["cap"] = h.copy(), np.ones(S)
    return out


def solve_exact(HJ, h0, msa, w, q, lam, gap=False, tol=1e-10, max_steps=200):
    """per-site Newton iteration (exact Hessian, capped step) from h0 (L, Q) until |g_h| < tol -> (h*, |g_h|, steps)"""
    Q = HJ.shape[2]
    live = live_states(q, gap, Q)
    a0 = 1 if gap else 0
    h = np.where(live, np.array(h0, np.float64), 0.0)
    for step in range(max_steps):
        g = field_gradient(tile_sums(HJ, h, msa, w, q, gap), h, lam, live)
        norm = float(np.sqrt((g * g).sum()))
        if norm < tol:
            return h, norm, step
        H = exact_hessian(HJ, h, msa, w, q, lam, gap)
        h, _ = newton_step(h, g, np.linalg.inv(H), a0)
        h = np.where(live, h, 0.0)
    raise RuntimeError("field solve did not converge: |g_h| = %.3e" % norm)
