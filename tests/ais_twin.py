"""numpy twin of annealed importance sampling (plm_ais, DESIGN_NEXT_ROWS.md section 9.8) on top of tests/sampler_twin.py:
the coupling sums U in float32 in the order j = 0 .. L-1, the argument of the draw fadd(h, fmul(beta, U)) in float32, the
draw itself in float64 (tw.draw), the tracked coupling energy and the log weights in float64.  Not a test module."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_twin as tw  # noqa: E402


def linear_schedule(K):
    return np.array([np.float32(k / K) for k in range(K + 1)], np.float32)


def log_z0(h):
    """sum_i log sum_a exp h_i(a) in float64."""
    h = np.asarray(h, np.float32).astype(np.float64)
    m = h.max(axis=1)
    return float(sum(m[i] + np.log(np.exp(h[i] - m[i]).sum()) for i in range(h.shape[0])))


def coupling_sums(x, Wf, i):
    """U[c, a] = sum_{j != i} J_ij(a, x_cj) in float32, from zero, j = 0 .. L-1.  Wf: float32 [L, L, q, q] (tw.dense)."""
    C, L = x.shape
    U = np.zeros((C, Wf.shape[2]), np.float32)
    for j in range(L):
        if j != i:
            U = U + Wf[i, j][:, x[:, j]].T
    return U


def summary(logw, lz0):
    """(log_z, log_z_se, ess) of the definition, sums in chain order in float64."""
    logw = np.asarray(logw, np.float64)
    C = len(logw)
    m = logw.max()
    w = np.exp(logw - m)
    s1 = s2 = 0.0
    for v in w:
        s1 += v
        s2 += v * v
    mean = s1 / C
    se = float(np.sqrt(((w - mean) ** 2).sum() / (C - 1)) / (np.sqrt(C) * mean)) if C > 1 else 0.0
    return float(lz0 + m + np.log(mean)), se, float(s1 * s1 / s2)


def ais(hi, jij, q, n_chains, n_temps=None, sweeps_per_temp=1, betas=None, seed=0, trace=False):
    """Twin of plm.log_partition without the energies of the final states.  trace=True adds `steps`: per step the states
    after it, and the twin's diagnostics (margin, max |arg|) per (sweep, chain, site) with the start rule first."""
    hf = np.asarray(hi, np.float32).reshape(-1, q)
    L = hf.shape[0]
    h = hf.astype(np.float64)
    Wf = tw.dense(np.asarray(jij, np.float32).astype(np.float64), L, q).astype(np.float32)
    b = linear_schedule(int(n_temps)) if betas is None else np.asarray(betas, np.float32)
    K, n, C = len(b) - 1, int(sweeps_per_temp), int(n_chains)
    chains = np.arange(C)
    margin0, maxarg0 = np.ones((C, L)), np.zeros((C, L))
    x = tw.start_states(h, C, seed, margin=margin0, maxbu=maxarg0)
    E = np.zeros(C)
    for i in range(L):
        E = E + coupling_sums(x, Wf, i)[chains, x[:, i]].astype(np.float64)
    E = 0.5 * E
    logw = np.zeros(C)
    steps = dict(states=[x.copy()], margin=[margin0], maxarg=[maxarg0], log_w=[logw.copy()], e_j=[E.copy()])
    for k in range(1, K + 1):
        logw = logw + (np.float64(b[k]) - np.float64(b[k - 1])) * E
        margin, maxarg = np.ones((C, L)), np.zeros((C, L))
        for s in range(n):
            for i in range(L):
                U = coupling_sums(x, Wf, i)
                arg = hf[i][None, :] + b[k] * U                         # float32: one rounding per operation
                assert arg.dtype == np.float32
                a, mg, mb = tw.draw(arg.astype(np.float64), tw.uniform(seed, chains, (k - 1) * n + s, i))
                E = E + (U[chains, a].astype(np.float64) - U[chains, x[:, i]].astype(np.float64))
                x[:, i] = a
                margin[:, i] = np.minimum(margin[:, i], mg)
                maxarg[:, i] = np.maximum(maxarg[:, i], mb)
        if trace:
            steps["states"].append(x.copy())
            steps["margin"].append(margin)
            steps["maxarg"].append(maxarg)
            steps["log_w"].append(logw.copy())
            steps["e_j"].append(E.copy())
    lz0 = log_z0(hf)
    lz, se, ess = summary(logw, lz0)
    out = dict(log_z=lz, log_z0=lz0, log_z_se=se, ess=ess, log_w=logw, e_j=E, states=x.astype(np.int8), steps_done=K,
               status="converged")
    if trace:
        out["steps"] = {k: np.array(v) for k, v in steps.items()}
    return out


def exact_log_z(hi, jij, q, beta=1.0):
    """log sum_x exp(H_h(x) + beta H_J(x)) over all q^L states."""
    h = np.asarray(hi, np.float32).astype(np.float64).reshape(-1, q)
    L = h.shape[0]
    en = tw.hamiltonians(tw.all_states(L, q), h, tw.dense(np.asarray(jij, np.float32).astype(np.float64), L, q))
    e = en[:, 2] + beta * en[:, 1]
    return float(e.max() + np.log(np.exp(e - e.max()).sum()))


def log_partition(hi, jij, q, n_chains=4096, n_temps=1000, sweeps_per_temp=1, betas=None, seed=0, steps_per_launch=0,
                  callback=None, device=0):
    """Twin of evcouplings_amd.plm.log_partition (same arguments, same return value; no launches, so no callback)."""
    res = ais(hi, jij, q, n_chains, n_temps, sweeps_per_temp, betas, seed)
    if betas is None or float(np.asarray(betas, np.float32)[-1]) == 1.0:
        h = np.asarray(hi, np.float32).astype(np.float64).reshape(-1, q)
        W = tw.dense(np.asarray(jij, np.float32).astype(np.float64), h.shape[0], q)
        H = tw.hamiltonians(res["states"].astype(np.int64), h, W)[:, 0]
        w = np.exp(res["log_w"] - res["log_w"].max())
        res["mean_energy"] = float((w / w.sum()) @ H)
        res["entropy"] = res["log_z"] - res["mean_energy"]
    return res


# the two enumerable models of the tests against exact log Z: (L, q, standard deviation of J, seed of the model)
ENUMERABLE = ((5, 4, 0.5, 11), (4, 7, 0.7, 12))
ENUMERABLE_K, ENUMERABLE_C, ENUMERABLE_SEEDS = 16, 4096, (1, 2, 3)


def enumerable_model(L, q, j_scale, model_seed):
    """h ~ N(0, 1), J ~ N(0, j_scale^2), rounded to float32."""
    rng = np.random.default_rng(model_seed)
    h = rng.normal(size=(L, q)).astype(np.float32)
    J = rng.normal(scale=j_scale, size=(L * (L - 1) // 2, q, q)).astype(np.float32)
    return h, J
