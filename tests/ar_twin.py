"""numpy float64 twin of the autoregressive Potts model (plm_ar_*, DESIGN_NEXT_ROWS.md section 9.19):
    P(x) = prod_i softmax_b( h_i(b) + sum_{j<i} J_ji(x_j, b) ) at b = x_i
with block (j, i), j < i, of the canonical layout coupling state a of the earlier site j (rows) with state b of the later
site i (columns).  The ancestral pass with the margins of sampler_twin.draw, log P, F and its gradient, the repack "by
later site" and its inverse, and enumeration helpers.  Not a test module."""
import numpy as np

import sampler_twin as st


def n_params(L, q):
    return L * q + L * (L - 1) // 2 * q * q


def pair_index(j, i, L):
    """canonical index of block (j, i), j < i"""
    return j * L - j * (j + 1) // 2 + (i - j - 1)


def random_model(L, q, seed=None, sd_h=1.0, sd_j=0.15):
    """h ~ N(0, sd_h), J ~ N(0, sd_j) from default_rng(7000 + L) unless a seed is given, rounded to float32."""
    rng = np.random.default_rng(7000 + L if seed is None else seed)
    h = rng.normal(0.0, sd_h, (L, q)).astype(np.float32)
    J = rng.normal(0.0, sd_j, (L * (L - 1) // 2, q, q)).astype(np.float32)
    return h, J


def dense(J, L, q):
    """i<j blocks -> D[j, i, a, b] for j < i (zero elsewhere), float64"""
    D = np.zeros((L, L, q, q))
    if L > 1:
        ju, iu = np.triu_indices(L, 1)
        D[ju, iu] = np.asarray(J, np.float64).reshape(len(ju), q, q)
    return D


def logits(x, h, J):
    """U[s, i, b] = h_i(b) + sum_{j<i} J_ji(x_sj, b), float64.  x: (n, L) states."""
    x = np.asarray(x, np.int64)
    n, L = x.shape
    q = h.shape[1]
    D = dense(J, L, q)
    U = np.tile(np.asarray(h, np.float64)[None], (n, 1, 1))
    for i in range(1, L):
        # D[j, i, x_sj, :] for j < i
        U[:, i] += D[np.arange(i)[None, :], i, x[:, :i]].sum(axis=1)
    return U


def site_logp(x, h, J, U=None):
    """log P(x_si | x_s,<i): the logit of the observed state minus the maximum minus the log of the sum of exp"""
    x = np.asarray(x, np.int64)
    U = logits(x, h, J) if U is None else U
    m = U.max(axis=2)
    S = np.exp(U - m[:, :, None]).sum(axis=2)
    ux = np.take_along_axis(U, x[:, :, None], axis=2)[:, :, 0]
    return (ux - m) - np.log(S)


def logp(x, h, J):
    return site_logp(x, h, J).sum(axis=1)


def probabilities(U):
    e = np.exp(U - U.max(axis=2, keepdims=True))
    return e / e.sum(axis=2, keepdims=True)


def objective(x, w, h, J, lambda_h, lambda_j, gradient=True):
    """(F, nll, g_h, g_J) in float64; the division by N_eff follows the sums"""
    x = np.asarray(x, np.int64)
    n, L = x.shape
    q = h.shape[1]
    h64, J64 = np.asarray(h, np.float64), np.asarray(J, np.float64).reshape(-1, q, q)
    w = np.asarray(w, np.float64)
    neff = w.sum()
    U = logits(x, h, J)
    nll = -(w * site_logp(x, h, J, U).sum(axis=1)).sum() / neff
    F = nll + lambda_h * (h64 ** 2).sum() + lambda_j * (J64 ** 2).sum()
    if not gradient:
        return F, nll, None, None
    onehot = np.zeros((n, L, q))
    np.put_along_axis(onehot, x[:, :, None], 1.0, axis=2)
    R = w[:, None, None] * (onehot - probabilities(U))            # [n][L][q]
    g_h = -R.sum(axis=0) / neff + 2.0 * lambda_h * h64
    g_J = np.zeros_like(J64)
    for j in range(L - 1):
        # sum_s onehot[s, j, a] R[s, i, b] for every i > j
        blk = (onehot[:, j].T @ R[:, j + 1:].reshape(n, -1)).reshape(q, L - 1 - j, q).transpose(1, 0, 2)
        p0 = pair_index(j, j + 1, L)
        g_J[p0:p0 + L - 1 - j] = -blk / neff
    g_J += 2.0 * lambda_j * J64
    return F, nll, g_h, g_J


def pack(h, J):
    return np.concatenate([np.asarray(h, np.float64).ravel(), np.asarray(J, np.float64).ravel()])


def unpack(x, L, q):
    return x[:L * q].reshape(L, q), x[L * q:].reshape(L * (L - 1) // 2, q, q)


def repack(J, L, q):
    """canonical blocks -> the kernels' order "by later site": for site i the rows [j < i][a][QP], QP = q rounded up to
    four, table i behind table i - 1"""
    QP = (q + 3) // 4 * 4
    J = np.asarray(J).reshape(L * (L - 1) // 2, q, q)
    T = np.zeros((L * (L - 1) // 2, q, QP), J.dtype)
    for i in range(1, L):
        for j in range(i):
            T[i * (i - 1) // 2 + j, :, :q] = J[pair_index(j, i, L)]
    return T


def unrepack(T, L, q):
    J = np.zeros((L * (L - 1) // 2, q, q), T.dtype)
    for i in range(1, L):
        for j in range(i):
            J[pair_index(j, i, L)] = T[i * (i - 1) // 2 + j, :, :q]
    return J


def sample(h, J, n, seed=0, beta=1.0, allowed=None, first_chain=0):
    """The ancestral pass in float64 with the draw and the uniforms of the sampler's contract, counter
    (first_chain + c, 0, 0, i).  Returns (states [n][L], margin [n][L], max|beta U| [n][L])."""
    L, q = h.shape
    D = dense(J, L, q)
    h64 = np.asarray(h, np.float64)
    x = np.zeros((n, L), np.int64)
    margin, maxbu = np.ones((n, L)), np.zeros((n, L))
    chains = np.arange(n) + first_chain
    for i in range(L):
        U = np.tile(h64[i], (n, 1))
        if i:
            U += D[np.arange(i)[None, :], i, x[:, :i]].sum(axis=1)
        x[:, i], margin[:, i], maxbu[:, i] = st.draw(U, st.uniform(seed, chains, 0, i), beta, allowed)
    return x, margin, maxbu


def explained(name, gpu, twin, margin, maxbu, L, q, cap=0.01):
    """The condition of the draw-for-draw tests of the samplers (test_gpu_sampler._explained) for one pass: a chain may
    differ only if at its first differing site the twin's u lies within 2^-24 (L + 4q)(1 + max|beta U|) of a step of the
    twin's normalised CDF, and at most `cap` of the chains may differ at all."""
    differs = gpu != twin
    bad = np.nonzero(differs.any(axis=1))[0]
    unexplained = []
    for c in bad:
        i = int(np.argmax(differs[c]))
        delta = 2.0 ** -24 * (L + 4 * q) * (1.0 + maxbu[c, i])
        if not margin[c, i] <= delta:
            unexplained.append((int(c), i, float(margin[c, i]), float(delta)))
    print("%s: %d of %d chains differ from the twin, %d unexplained" % (name, len(bad), len(twin), len(unexplained)))
    assert not unexplained, unexplained[:5]
    assert len(bad) <= cap * len(twin), (len(bad), len(twin))


def enumerate_p(h, J, beta=1.0, allowed=None):
    """P(x) of every state of sampler_twin.all_states(L, q), each conditional taken at beta over the allowed states"""
    L, q = h.shape
    xs = st.all_states(L, q)
    U = beta * logits(xs, h, J)
    ok = np.ones(q, bool) if allowed is None else np.asarray(allowed, bool)
    e = np.where(ok[None, None, :], np.exp(U - U[:, :, ok].max(axis=2, keepdims=True)), 0.0)
    p = e / e.sum(axis=2, keepdims=True)
    return np.take_along_axis(p, xs[:, :, None], axis=2)[:, :, 0].prod(axis=1)
