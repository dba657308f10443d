"""numpy float64 twin of the Gibbs sampler (plm_sample, DESIGN_NEXT_ROWS.md section 9.6): the Philox4x32-10 block, the
uniform of a (seed, chain, sweep, site), the systematic-scan sweep with masks, the start rule, and exact enumeration
helpers for small models (Boltzmann distribution, transition matrix of one sweep).  Not a test module."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
START_SWEEP = 0xFFFFFFFF


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """The four output words (uint64 arrays holding 32-bit values) of the block function."""
    c0, c1, c2, c3 = [np.asarray(c, np.uint64) & MASK for c in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = M0 * c0
        p1 = M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0 = (k0 + W0) & MASK
        k1 = (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniform(seed, chain, sweep, site):
    """u = ((word0 >> 8) + 0.5) 2^-24 of counter (chain, 0, sweep, site), key (seed low, seed high)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w0 = philox4x32_10(chain, 0, sweep, site, seed & 0xFFFFFFFF, seed >> 32)[0]
    return ((w0 >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def dense(J_pairs, L, q):
    """i<j blocks [P][q][q] -> W[i, j, a, b] = J_ij(a, b) for every ordered pair, zero diagonal blocks."""
    W = np.zeros((L, L, q, q))
    if L > 1:
        iu, ju = np.triu_indices(L, 1)
        J_pairs = np.asarray(J_pairs, np.float64).reshape(len(iu), q, q)
        W[iu, ju] = J_pairs
        W[ju, iu] = J_pairs.transpose(0, 2, 1)
    return W


def _mask(allowed, q):
    return np.ones(q, bool) if allowed is None else np.asarray(allowed).astype(bool).reshape(q)


def draw(U, u, beta=1.0, allowed=None):
    """One draw per row of U (C, q): e_a = exp(beta U_a - max) over the allowed states in state order, running sum S_a,
    first allowed a with S_a > u S_last (the last allowed state if none).  Returns (states, margin, max |beta U|) where
    margin = the distance of u from the nearest step of the normalised running sum."""
    q = U.shape[1]
    ok = _mask(allowed, q)
    bu = beta * U[:, ok]
    e = np.exp(bu - bu.max(axis=1, keepdims=True))
    cdf = np.cumsum(e, axis=1)
    t = u * cdf[:, -1]
    k = np.minimum((cdf <= t[:, None]).sum(axis=1), ok.sum() - 1)
    states = np.nonzero(ok)[0][k]
    if cdf.shape[1] > 1:
        margin = np.abs(cdf[:, :-1] / cdf[:, -1:] - u[:, None]).min(axis=1)
    else:
        margin = np.ones(len(u))
    return states, margin, np.abs(bu).max(axis=1)


def _one_hot(x, q):
    C, L = x.shape
    X = np.zeros((C, L * q))
    X[np.arange(C)[:, None], np.arange(L)[None, :] * q + x] = 1.0
    return X


def conditional_energies(x, h, W, i, X=None):
    """U[c, a] = h_i(a) + sum_{j != i} J_ij(a, x_cj), as a one-hot product (X = _one_hot(x, q), if the caller has it)."""
    C, L = x.shape
    q = h.shape[1]
    U = np.tile(h[i], (C, 1)).astype(np.float64)
    if L > 1:
        if X is None:
            X = _one_hot(x, q)
        # W[j, i, b, a] = J_ij(a, b): rows (j, b), columns a; the diagonal block is zero
        U += X @ W[:, i].reshape(L * q, q)
    return U


def sweep(x, h, W, seed, sweep_no, beta=1.0, fixed=None, allowed=None, chain0=0, margin=None, maxbu=None):
    """One systematic-scan sweep (sites 0 .. L-1) in place on x (C, L) integer states.  Fixed sites are skipped (their
    counter is simply not used).  margin / maxbu: optional (C, L) arrays filled with draw()'s diagnostics."""
    C, L = x.shape
    q = h.shape[1]
    chains = np.arange(C) + chain0
    X = _one_hot(x, q)
    for i in range(L):
        if fixed is not None and fixed[i]:
            continue
        a, mg, mb = draw(conditional_energies(x, h, W, i, X), uniform(seed, chains, sweep_no, i), beta, allowed)
        x[:, i] = a
        X[:, i * q:(i + 1) * q] = 0.0
        X[np.arange(C), i * q + a] = 1.0
        if margin is not None:
            margin[:, i] = mg
        if maxbu is not None:
            maxbu[:, i] = mb
    return x


def start_states(h, n_chains, seed, beta=1.0, allowed=None, margin=None, maxbu=None):
    """The start rule: one draw per site of softmax beta h_i over the allowed states, sweep index 0xFFFFFFFF."""
    L, q = h.shape
    x = np.zeros((n_chains, L), np.int64)
    chains = np.arange(n_chains)
    for i in range(L):
        a, mg, mb = draw(np.tile(h[i], (n_chains, 1)).astype(np.float64), uniform(seed, chains, START_SWEEP, i), beta,
                         allowed)
        x[:, i] = a
        if margin is not None:
            margin[:, i] = mg
        if maxbu is not None:
            maxbu[:, i] = mb
    return x


def hamiltonians(x, h, W):
    """(H, H_J, H_h) per row, as plm.hamiltonians."""
    C, L = x.shape
    hh = h[np.arange(L)[None, :], x].sum(axis=1)
    hj = np.zeros(C)
    if L > 1:
        iu, ju = np.triu_indices(L, 1)
        hj = W[iu[None, :], ju[None, :], x[:, iu], x[:, ju]].sum(axis=1)
    return np.stack([hh + hj, hj, hh], axis=1)


def sample(hi, jij, q, n_chains, burn_in=10, n_snapshots=1, thin=1, beta=1.0, seed=0, start=None, fixed=None,
           allowed=None, energies=True, device=0):
    """Twin of evcouplings_amd.plm.sample (same arguments, same return value)."""
    h = np.asarray(hi, np.float32).astype(np.float64).reshape(-1, q)
    L = h.shape[0]
    W = dense(np.asarray(jij, np.float32).astype(np.float64), L, q)
    if start is None:
        x = start_states(h, n_chains, seed, beta, allowed)
    else:
        x = np.array(start, np.int64).reshape(n_chains, L)
    out = np.zeros((n_snapshots, n_chains, L), np.int8)
    s = 0
    for k in range(n_snapshots):
        for _ in range(burn_in if k == 0 else thin):
            sweep(x, h, W, seed, s, beta, fixed, allowed)
            s += 1
        out[k] = x
    en = None
    if energies:
        en = np.stack([hamiltonians(out[k].astype(np.int64), h, W) for k in range(n_snapshots)])
    return out, en


# ---- exact enumeration (q^L up to ~10^4) -------------------------------------------------------------------------

def all_states(L, q):
    return np.array(np.unravel_index(np.arange(q ** L), (q,) * L)).T


def state_index(x, q):
    x = np.asarray(x, np.int64)
    return np.ravel_multi_index(x.T, (q,) * x.shape[1])


def boltzmann(h, W, beta=1.0):
    """P(x) of every state of all_states(L, q)."""
    L, q = h.shape
    st = all_states(L, q)
    E = beta * hamiltonians(st, h, W)[:, 0]
    p = np.exp(E - E.max())
    return p / p.sum()


def conditioned(p, L, q, allowed=None, fixed=None):
    """p restricted to the states whose non-fixed sites are allowed and whose fixed sites hold fixed[i] (a dict
    site -> state), renormalised."""
    st = all_states(L, q)
    keep = np.ones(len(st), bool)
    ok = _mask(allowed, q)
    fixed = fixed or {}
    for i in range(L):
        keep &= (st[:, i] == fixed[i]) if i in fixed else ok[st[:, i]]
    p = np.where(keep, p, 0.0)
    return p / p.sum()


def transition_matrix(h, W, beta=1.0, allowed=None, fixed=None):
    """Row-stochastic matrix of one sweep (sites 0 .. L-1, without the sites flagged in `fixed`, draws over the allowed
    states) over all_states(L, q)."""
    L, q = h.shape
    st = all_states(L, q)
    K = len(st)
    ok = _mask(allowed, q)
    P = np.eye(K)
    for i in range(L):
        if fixed is not None and fixed[i]:
            continue
        U = beta * conditional_energies(st, h, W, i)
        pc = np.where(ok[None, :], np.exp(U - U[:, ok].max(axis=1, keepdims=True)), 0.0)
        pc /= pc.sum(axis=1, keepdims=True)
        Ti = np.zeros((K, K))
        for a in range(q):
            tgt = st.copy()
            tgt[:, i] = a
            Ti[np.arange(K), state_index(tgt, q)] += pc[:, a]
        P = P @ Ti
    return P


def start_distribution(h, beta=1.0, allowed=None):
    """Distribution of the start rule over all_states(L, q): the product of softmax beta h_i over the allowed states."""
    L, q = h.shape
    ok = _mask(allowed, q)
    st = all_states(L, q)
    pi = np.where(ok[None, :], np.exp(beta * (h - h[:, ok].max(axis=1, keepdims=True))), 0.0)
    pi /= pi.sum(axis=1, keepdims=True)
    return pi[np.arange(L)[None, :], st].prod(axis=1)


def sweeps_to_mix(mu0, P, target, tv=1e-6, cap=500):
    """The smallest B with total variation |mu0 P^B - target| / 2 <= tv."""
    mu = np.asarray(mu0, np.float64)
    for B in range(1, cap + 1):
        mu = mu @ P
        if 0.5 * np.abs(mu - target).sum() <= tv:
            return B
    raise AssertionError("no mixing to %g within %d sweeps" % (tv, cap))


def chi2_counts(counts, p, n, min_expected=5.0):
    """Pearson chi-square of observed counts against n p over the cells with p > 0, cells with an expected count below
    min_expected pooled into one; returns (chi2, degrees of freedom).  A count in a cell with p == 0 gives inf."""
    counts = np.asarray(counts, np.float64).ravel()
    p = np.asarray(p, np.float64).ravel()
    if counts[p == 0].sum() > 0:
        return np.inf, int((p > 0).sum()) - 1
    exp = n * p[p > 0]
    obs = counts[p > 0]
    small = exp < min_expected
    if small.any():
        exp = np.concatenate([exp[~small], [exp[small].sum()]])
        obs = np.concatenate([obs[~small], [obs[small].sum()]])
    return float(((obs - exp) ** 2 / exp).sum()), len(exp) - 1
