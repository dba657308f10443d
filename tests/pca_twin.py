"""numpy twin of the principal components of an alignment (include/plm_hip.h, "principal components of an alignment"):
the weight quantisation of the three-site twin, the dense one-hot matrix, the covariance, numpy.linalg.eigh, the
sign rule and the projection formula, all in float64.  The oracle of tests/test_pca_host.py and tests/test_gpu_pca.py;
written from the definitions, not from the kernels."""
import numpy as np

from triplet_twin import quantise


def kept(L, q, skip_state=None):
    """Boolean mask [L q] of the kept features, feature (i, a) at i q + a."""
    m = np.ones((L, q), bool)
    if skip_state is not None and skip_state >= 0:
        m[:, skip_state] = False
    return m.reshape(-1)


def frequencies(msa, q, wq, W):
    """f [L, q] = count / W from exact integer counts."""
    msa = np.asarray(msa).astype(np.int64)
    N, L = msa.shape
    cnt = np.zeros((L, q), np.int64)
    for i in range(L):
        np.add.at(cnt[i], msa[:, i], wq)
    return cnt.astype(np.float64) / float(W)


def features(seqs, q, f, skip_state=None):
    """The centred one-hot matrix [n, L q]; zero columns at the skipped state."""
    seqs = np.asarray(seqs).astype(np.int64)
    n, L = seqs.shape
    onehot = np.zeros((n, L, q))
    onehot[np.arange(n)[:, None], np.arange(L)[None, :], seqs] = 1.0
    phi = (onehot - f[None]).reshape(n, L * q)
    phi[:, ~kept(L, q, skip_state)] = 0.0
    return phi


def covariance(msa, q, weights=None, skip_state=None):
    """-> (C [L q, L q], f [L, q], wq, W).  C = (1/W) sum_n wq_n phi_n phi_n^T = count_ij(a,b) / W - f_i(a) f_j(b): the
    pair counts are exact integers (a float64 product of integer matrices whose sums stay below 2^53), the quotient,
    the product and the difference are taken in extended precision and rounded once, so every entry of C is correct
    to its last bit or two whatever the number of sequences."""
    msa = np.asarray(msa)
    N, L = msa.shape
    wq, W = quantise(weights, N)
    assert W < 2 ** 53
    f = frequencies(msa, q, wq, W)
    onehot = np.zeros((N, L, q))
    onehot[np.arange(N)[:, None], np.arange(L)[None, :], msa.astype(np.int64)] = 1.0
    onehot = onehot.reshape(N, L * q)
    counts = (onehot * wq.astype(np.float64)[:, None]).T @ onehot                # exact
    single = np.diag(counts).astype(np.longdouble) / np.longdouble(W)
    C = (counts.astype(np.longdouble) / np.longdouble(W) - single[:, None] * single[None, :]).astype(np.float64)
    drop = ~kept(L, q, skip_state)
    C[drop, :] = 0.0
    C[:, drop] = 0.0
    return C, f, wq, W


def total_variance(f, skip_state=None):
    L, q = f.shape
    return float((f * (1.0 - f)).reshape(-1)[kept(L, q, skip_state)].sum())


def sign_rule(v):
    """The entry with the largest magnitude positive; the smallest index of a tie decides."""
    v = np.asarray(v, np.float64)
    return -v if v[int(np.argmax(np.abs(v)))] < 0 else v


def fit(msa, q, k, weights=None, skip_state=None):
    """The twin of plm.pca_fit: every eigenvalue of C in descending order ("spectrum") and the k leading ones with
    their eigenvectors."""
    msa = np.asarray(msa)
    L = msa.shape[1]
    C, f, wq, W = covariance(msa, q, weights, skip_state)
    keep = kept(L, q, skip_state)
    lam, vec = np.linalg.eigh(C[np.ix_(keep, keep)])
    lam, vec = lam[::-1], vec[:, ::-1]
    comp = np.zeros((k, L * q))
    for c in range(k):
        comp[c, keep] = sign_rule(vec[:, c])
    return {"mean": f, "components": comp.reshape(k, L, q), "eigenvalues": lam[:k].copy(), "spectrum": lam,
            "total_variance": total_variance(f, skip_state), "total": W, "wq": wq, "C": C}


def project(seqs, q, mean, components, skip_state=None):
    """t_c(x) = sum_i v_c[(i, x_i)] - sum_{i,a} f_i(a) v_c[(i,a)], a skipped state contributing 0: [n, k]."""
    seqs = np.asarray(seqs).astype(np.int64)
    n, L = seqs.shape
    comp = np.array(components, np.float64).reshape(-1, L, q)
    if skip_state is not None and skip_state >= 0:
        comp[:, :, skip_state] = 0.0
    gathered = comp[:, np.arange(L)[None, :], seqs].sum(axis=2).T            # [n, k]
    return gathered - (comp * np.asarray(mean, np.float64)[None]).sum(axis=(1, 2))[None, :]


def weighted_moments(t, wq):
    """Weighted mean and variance about zero of every column of the scores."""
    w = np.asarray(wq, np.float64)
    t = np.asarray(t, np.float64)
    return (w[:, None] * t).sum(axis=0) / w.sum(), (w[:, None] * t * t).sum(axis=0) / w.sum()


def sin_angle(u, v):
    """|sin| of the angle between two vectors."""
    u, v = np.asarray(u, np.float64).ravel(), np.asarray(v, np.float64).ravel()
    u, v = u / np.linalg.norm(u), v / np.linalg.norm(v)
    return float(np.linalg.norm(u - (u @ v) * v))
