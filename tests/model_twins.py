"""
Vectorised float64 numpy twins of plm.model_pair_scores, plm.double_mutant_matrix and plm.independent_fields
(the arithmetic of the reference's CouplingsModel._calculate_ecs, .double_mut_mat and .to_independent_model,
couplings/model.py:715-742, 777-827, 882-927).  Test code only: the CPU tests put them in place of the library calls,
the GPU tests compare the kernels with them at sizes the golden fixture does not reach.
"""
import numpy as np


def pair_scores(J_ij, f_ij, f_i):
    """(fn, mi) [L,L]: zero-sum gauge over all q states, Frobenius norm; MI over f_ij > 0 (numpy IEEE rules: +inf where
    f_ij > 0 meets f_i f_j = 0).  A float32 f_i keeps numpy's float32 outer product, as in the reference."""
    L = f_i.shape[0]
    iu, ju = np.triu_indices(L, 1)
    Jb = np.asarray(J_ij, np.float64)[iu, ju]
    J0 = Jb - Jb.mean(axis=2, keepdims=True) - Jb.mean(axis=1, keepdims=True) + Jb.mean(axis=(1, 2), keepdims=True)
    fn_p = np.sqrt((J0 ** 2).sum(axis=(1, 2)))
    p = np.asarray(f_ij, np.float64)[iu, ju]
    m = f_i[iu][:, :, None] * f_i[ju][:, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = np.where(p > 0, p * np.log(p / m), 0.0)
    mi_p = terms.sum(axis=(1, 2))
    fn, mi = np.zeros((L, L)), np.zeros((L, L))
    fn[iu, ju] = fn[ju, iu] = fn_p
    mi[iu, ju] = mi[ju, iu] = mi_p
    return fn, mi


def double_mutants(J_ij, smm, target):
    """dense [L,L,q,q]: D[i,j,a,b] = smm[i,a] + smm[j,b] + J[a,b] - J[a,t_j] - J[t_i,b] + J[t_i,t_j], D[j,i] = D[i,j].T"""
    smm = np.asarray(smm, np.float64)
    L, q = smm.shape
    t = np.asarray(target).ravel().astype(np.int64)
    iu, ju = np.triu_indices(L, 1)
    Jb = np.asarray(J_ij, np.float64)[iu, ju]
    k = np.arange(len(iu))
    Dp = (smm[iu][:, :, None] + smm[ju][:, None, :] + Jb - Jb[k, :, t[ju]][:, :, None] - Jb[k, t[iu], :][:, None, :]
          + Jb[k, t[iu], t[ju]][:, None, None])
    D = np.zeros((L, L, q, q))
    D[iu, ju] = Dp
    D[ju, iu] = Dp.transpose(0, 2, 1)
    return D


def objective(x, f_i, lambda_h, n_eff):
    """per-site objective and gradient of the independent-site model (rows of x)"""
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    Z = e.sum(axis=1, keepdims=True)
    P = e / Z
    F = n_eff * ((m[:, 0] + np.log(Z[:, 0])) - (f_i * x).sum(axis=1)) + lambda_h * (x ** 2).sum(axis=1)
    g = n_eff * (P - f_i) + lambda_h * 2 * x
    return F, g, P


def independent_fields(f_i, lambda_h, n_eff, cap=100):
    """damped Newton (Sherman-Morrison on the diagonal-plus-rank-one Hessian, Armijo backtracking), all sites at once;
    returns (h, Newton steps per site)"""
    f_i = np.asarray(f_i, np.float64)
    L, q = f_i.shape
    x = np.zeros((L, q))
    F, g, P = objective(x, f_i, lambda_h, n_eff)
    tol = 1e-12 * max(1.0, n_eff)
    iters = np.zeros(L, np.int32)
    for _ in range(cap):
        gmax = np.abs(g).max(axis=1)
        act = gmax > tol
        if not act.any():
            break
        dinv = 1.0 / (n_eff * P + 2 * lambda_h)
        ptdg = (P * dinv * g).sum(axis=1, keepdims=True)
        ptdp = (P * dinv * P).sum(axis=1, keepdims=True)
        d = -(dinv * g + n_eff * dinv * P * ptdg / (1.0 - n_eff * ptdp))
        gd = (g * d).sum(axis=1)
        act &= gd < 0
        t = np.ones(L)
        todo = act.copy()
        for _ in range(60):
            if not todo.any():
                break
            xn = x + t[:, None] * d
            Fn, gn, Pn = objective(xn, f_i, lambda_h, n_eff)
            ok = todo & ((Fn <= F + 1e-4 * t * gd) |
                         ((Fn <= F + 8 * np.finfo(float).eps * np.abs(F)) & (np.abs(gn).max(axis=1) < gmax)))
            x[ok], F[ok], g[ok], P[ok] = xn[ok], Fn[ok], gn[ok], Pn[ok]
            iters[ok] += 1
            todo &= ~ok
            t[todo] *= 0.5
        if todo.all() and todo.any():
            break
    return x, iters


def apc(matrix):
    """average product correction (the reference's CouplingsModel.apc, couplings/model.py:744-775)"""
    L = matrix.shape[0]
    col_means = np.mean(matrix, axis=0) * L / (L - 1)
    matrix_mean = np.mean(matrix) * L / (L - 1)
    corrected = matrix - np.outer(col_means, col_means) / matrix_mean
    corrected[np.diag_indices(L)] = 0
    return corrected


def dense_from_pairs(blocks, L):
    """i<j pair blocks [L(L-1)/2,q,q] (the .model order) -> dense symmetric [L,L,q,q] float64, zero diagonal blocks"""
    q = blocks.shape[-1]
    iu, ju = np.triu_indices(L, 1)
    dense = np.zeros((L, L, q, q))
    dense[iu, ju] = blocks
    dense[ju, iu] = np.asarray(blocks, np.float64).transpose(0, 2, 1)
    return dense
