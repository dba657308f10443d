"""numpy twin of the Boltzmann-machine refinement (plm_bm_fit, DESIGN_NEXT_ROWS.md section 9.7) on top of the sampler twin:
the counts, the step schedule, the update in float32 and the loop with its stopping rules; and the exact marginals of a
small model by enumeration.  Not a test module."""
import numpy as np

import sampler_twin as tw


def counts(x, q):
    """Exact counts of chain states x (C, L): n_i [L][q] and n_ij [L(L-1)/2][q][q] in the canonical pair order."""
    x = np.asarray(x, np.int64)
    C, L = x.shape
    ni = np.zeros((L, q), np.int64)
    for i in range(L):
        ni[i] = np.bincount(x[:, i], minlength=q)
    nij = np.zeros((L * (L - 1) // 2, q, q), np.int64)
    if L > 1:
        X = np.zeros((C, L * q), np.float32)          # one-hot Gram: exact in float32 below 2^24 chains
        X[np.arange(C)[:, None], np.arange(L)[None, :] * q + x] = 1.0
        G = (X.T @ X).reshape(L, q, L, q).transpose(0, 2, 1, 3)
        iu, ju = np.triu_indices(L, 1)
        nij = np.rint(G[iu, ju]).astype(np.int64)
    return ni, nij


def frequencies(x, q):
    """p = (float)n / (float)C in float32."""
    ni, nij = counts(x, q)
    c = np.float32(x.shape[0])
    return ni.astype(np.float32) / c, nij.astype(np.float32) / c


def step_size(lr, T, g):
    """lr_g of global epoch g."""
    if T == 0 or g + 1 <= T:
        return np.float32(lr)
    return np.float32(np.float64(np.float32(lr)) * T / (g + 1))


def update(x, f, p, lr_g, lam):
    """x + lr_g ((f - p) - 2 lambda x), every operation rounded to float32."""
    x, f, p = (np.asarray(a, np.float32) for a in (x, f, p))
    if lr_g == 0:
        return x.copy()
    g = (f - p) - (np.float32(2) * np.float32(lam)) * x
    return x + np.float32(lr_g) * g


def trace_row(fi, fij, pi, pij, lr_g):
    di = np.abs(np.asarray(fi, np.float32) - pi)
    dij = np.abs(np.asarray(fij, np.float32).reshape(pij.shape) - pij).astype(np.float64)
    rms = np.sqrt((dij ** 2).sum() / dij.size) if dij.size else 0.0
    return [float(di.max()), float(dij.max()) if dij.size else 0.0, float(rms), float(lr_g)]


def bm_fit(fi, fij, q, hi, jij, n_chains, n_epochs, sweeps_per_epoch=2, lr=0.5, lr_decay_after=0, lambda_h=0.0,
           lambda_j=0.0, tol=0.0, seed=0, start=None, first_epoch=0, callback=None, device=0):
    """Twin of evcouplings_amd.plm.bm_fit (same arguments, same return value)."""
    hi = np.array(hi, np.float32).reshape(-1, q)
    L = hi.shape[0]
    jij = np.array(jij, np.float32).reshape(L * (L - 1) // 2, q, q)
    fi = np.asarray(fi, np.float32).reshape(L, q)
    fij = np.asarray(fij, np.float32).reshape(jij.shape)
    if start is None:
        x = tw.start_states(hi.astype(np.float64), n_chains, seed)
    else:
        x = np.array(start, np.int64).reshape(n_chains, L)
    trace, done, status = [], 0, "maxiter"
    pi = pij = None
    for e in range(n_epochs):
        g = first_epoch + e
        W = tw.dense(jij.astype(np.float64), L, q)
        for s in range(sweeps_per_epoch):
            tw.sweep(x, hi.astype(np.float64), W, seed, g * sweeps_per_epoch + s)
        pi, pij = frequencies(x, q)
        lr_g = step_size(lr, lr_decay_after, g)
        trace.append(trace_row(fi, fij, pi, pij, lr_g))
        if tol > 0 and trace[-1][0] <= tol and trace[-1][1] <= tol:
            status = "converged"
            break
        if callback is not None and callback(g, *trace[-1]):
            status = "interrupted"
            break
        hi = update(hi, fi, pi, lr_g, lambda_h)
        jij = update(jij, fij, pij, lr_g, lambda_j)
        done = e + 1
    return dict(hi=hi, jij=jij, pi=pi, pij=pij, chains=x.astype(np.int8), trace=np.array(trace), epochs_done=done,
                status=status)


def exact_marginals(h, J, q):
    """(fi [L][q], fij [L(L-1)/2][q][q]) of the Boltzmann distribution of a small model, by enumeration."""
    h = np.asarray(h, np.float64).reshape(-1, q)
    L = h.shape[0]
    p = tw.boltzmann(h, tw.dense(np.asarray(J, np.float64), L, q))
    st = tw.all_states(L, q)
    fi = np.zeros((L, q))
    for i in range(L):
        fi[i] = np.bincount(st[:, i], weights=p, minlength=q)
    iu, ju = np.triu_indices(L, 1)
    fij = np.zeros((len(iu), q, q))
    for k, (i, j) in enumerate(zip(iu, ju)):
        fij[k] = np.bincount(st[:, i] * q + st[:, j], weights=p, minlength=q * q).reshape(q, q)
    return fi, fij


def enumerable_case():
    """The model, targets and start point of the exact-enumeration check (L = 5, q = 4)."""
    rng = np.random.default_rng(11)
    h = rng.normal(0, 0.7, (5, 4)).astype(np.float32)
    J = rng.normal(0, 0.6, (10, 4, 4)).astype(np.float32)
    fi, fij = exact_marginals(h, J, 4)
    h0 = np.log(fi)
    h0 = (h0 - h0.mean(axis=1, keepdims=True)).astype(np.float32)
    J0 = np.zeros((10, 4, 4), np.float32)
    return dict(h=h, J=J, fi=fi, fij=fij, h0=h0, J0=J0)


ENUM_SCHEDULE = dict(n_chains=16384, sweeps_per_epoch=4, n_epochs=300, lr=1.0, lr_decay_after=100, lambda_h=0.0,
                     lambda_j=0.0, seed=5)


def max_pair_error(h, J, fij, q):
    return float(np.abs(exact_marginals(h, J, q)[1] - fij).max())
