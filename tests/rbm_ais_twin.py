"""numpy twin of annealed importance sampling for the restricted Boltzmann machine (plm_rbm_ais, DESIGN_NEXT_ROWS.md section
9.25) on top of tests/rbm_twin.py and tests/sampler_twin.py.  The inputs I and the weight in float64 in the contract's
order (one add per site; the softplus differences summed from 0.0 inside each chunk of 8 hidden units, the chunk sums
from 0.0 in chunk order); the argument of the visible draw in float32, one numpy float32 operation at a time; the draw
itself is the sampler twin's.  Every draw's margin and max |x| are kept for the near-tie rule.  Not a test module."""
import numpy as np

import rbm_twin as tw
import sampler_twin as st

F32 = np.float32
HB = 8          # RBM_HB: hidden units per chunk of the weight sum


def linear_schedule(K):
    return np.array([np.float32(k / K) for k in range(K + 1)], np.float32)


def log_z0(g, M):
    """M log 2 + sum_i log sum_a exp g_i(a) in float64"""
    g = np.asarray(g, F32).astype(np.float64)
    m = g.max(axis=1)
    return float(M * np.log(2.0) + sum(m[i] + np.log(np.exp(g[i] - m[i]).sum()) for i in range(g.shape[0])))


def summary(logw, lz0):
    """(log_z, log_z_se, ess) as plm_ais forms them: sums in chain order in float64"""
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


def inputs(x, c, W):
    """I [C][M]: (double) c_mu, then one float64 add per site i = 0 .. L-1"""
    W64 = np.asarray(W, F32).astype(np.float64)
    I = np.tile(np.asarray(c, F32).astype(np.float64), (x.shape[0], 1))
    for i in range(x.shape[1]):
        I = I + W64[:, i, x[:, i]].T
    return I


def weight_step(I, b1, b0):
    """sum_mu sp(b1 I) - sp(b0 I) in the contract's order"""
    term = tw.softplus(np.float64(b1) * I) - tw.softplus(np.float64(b0) * I)
    total = np.zeros(I.shape[0])
    for m0 in range(0, I.shape[1], HB):
        chunk = np.zeros(I.shape[0])
        for mu in range(m0, min(m0 + HB, I.shape[1])):
            chunk = chunk + term[:, mu]
        total = total + chunk
    return total


def ais(g, c, W, n_chains, n_temps=None, sweeps_per_temp=1, betas=None, seed=0, trace=False, f64_arg=False):
    """Twin of plm.rbm_log_partition(hidden=True) without mean_score and entropy.  trace=True adds `steps`, per step k = 0
    (the start) .. K: states, hidden (of the step's last sweep), log_w, and the diagnostics of every sweep of the step
    stacked as [n][C][.]: hm = |u - p| and hx = |x| of the hidden draws, vm and va = the margin and max |arg| of the
    visible draws.  f64_arg: the argument of the visible draw in float64 instead (the condition of the device test)."""
    g32, c32, W32 = np.asarray(g, F32), np.asarray(c, F32), np.asarray(W, F32)
    L, q = g32.shape
    M = c32.size
    b = linear_schedule(int(n_temps)) if betas is None else np.asarray(betas, F32)
    K, n, C = len(b) - 1, int(sweeps_per_temp), int(n_chains)
    chains, mus = np.arange(C), np.arange(M)
    x, margin0, maxu0 = tw.start_states(g32, C, seed, diagnostics=True)
    logw, h = np.zeros(C), np.zeros((C, M), np.int64)
    steps = dict(states=[x.copy()], hidden=[h.copy()], log_w=[logw.copy()], hm=[], hx=[], vm=[], va=[])
    max_x = 0.0
    for k in range(1, K + 1):
        rec = dict(hm=[], hx=[], vm=[], va=[])
        for s in range(n):
            sweep = (k - 1) * n + s
            I = inputs(x, c32, W32)
            if s == 0:
                logw = logw + weight_step(I, b[k], b[k - 1])
            xk = np.float64(b[k]) * I
            max_x = max(max_x, float(np.abs(xk).max()), float(np.abs(np.float64(b[k - 1]) * I).max()))
            p = tw.sigmoid(xk)
            u = tw.uniform24(tw._word0(seed, chains[:, None], 2, sweep, mus[None, :])).astype(np.float64)
            hb = u < p
            h = hb.astype(np.int64)
            if f64_arg:
                S = np.tensordot(hb.astype(np.float64), W32.astype(np.float64), axes=(1, 0))
                arg = g32.astype(np.float64)[None] + np.float64(b[k]) * S
            else:
                S = np.zeros((C, L, q), F32)
                for mu in range(M):
                    S = np.where(hb[:, mu][:, None, None], S + W32[mu][None], S)
                prod = b[k] * S                                     # float32: one rounding per operation
                arg = g32[None] + prod
                assert S.dtype == prod.dtype == arg.dtype == F32
            vm, va = np.ones((C, L)), np.zeros((C, L))
            for i in range(L):
                x[:, i], vm[:, i], va[:, i] = st.draw(arg[:, i].astype(np.float64), st.uniform(seed, chains, sweep, i))
            rec["hm"].append(np.abs(u - p))
            rec["hx"].append(np.abs(xk))
            rec["vm"].append(vm)
            rec["va"].append(va)
        if trace:
            steps["states"].append(x.copy())
            steps["hidden"].append(h.copy())
            steps["log_w"].append(logw.copy())
            for key in rec:
                steps[key].append(np.stack(rec[key]))
    lz0 = log_z0(g32, M)
    lz, se, ess = summary(logw, lz0)
    out = dict(log_z=lz, log_z0=lz0, log_z_se=se, ess=ess, log_w=logw, states=x.astype(np.int8), hidden=h.astype(np.int8),
               steps_done=K, status="converged", max_x=max_x, start_margin=margin0, start_maxu=maxu0)
    if trace:
        out["steps"] = {key: np.array(v) for key, v in steps.items()}
    return out


def delta_hidden(absx):
    """the near-tie bound of a hidden draw: sigma in float64 from an x that carries a few ulp"""
    return 2.0 ** -49 * (1.0 + absx)


def log_w_bound(K, M, max_x):
    """each of the 2 K M softplus values carries a few ulp of 1 + |x| from exp and log1p, and the sums add as many
    roundings; the factor 8 over 2^-52 is the margin"""
    return 2.0 ** -49 * K * M * (1.0 + max_x)


def first_difference_explained(step, states, hidden, q):
    """The near-tie rule for one chain's step.  step: the twin's diagnostics of that step and chain, hm, hx [n][M], vm,
    va [n][L], and its states [L] and hidden [M] after it; states, hidden: the device's.  The draws of a step are ordered
    (sweep; hidden units 0 .. M-1; sites 0 .. L-1), and only the last sweep's are seen.  A difference is explained if the
    first differing draw that is seen has a margin within its bound (rbm_twin.delta_visible with max |arg| for a visible
    draw, delta_hidden for a hidden one), or if a draw of an earlier sweep of the step, which nobody sees, has."""
    n, M = step["hm"].shape
    for s in range(n - 1):
        if (step["hm"][s] <= delta_hidden(step["hx"][s])).any() or \
                (step["vm"][s] <= tw.delta_visible(M, q, step["va"][s])).any():
            return True
    dh = np.asarray(hidden) != step["hidden"]
    if dh.any():
        mu = int(np.argmax(dh))
        return bool(step["hm"][n - 1, mu] <= delta_hidden(step["hx"][n - 1, mu]))
    dv = np.asarray(states) != step["states"]
    i = int(np.argmax(dv))
    return bool(step["vm"][n - 1, i] <= tw.delta_visible(M, q, step["va"][n - 1, i]))


def log_partition(g, c, W, q, n_chains=4096, n_temps=1000, sweeps_per_temp=1, betas=None, seed=0, steps_per_launch=0,
                  callback=None, hidden=False, device=0):
    """Twin of evcouplings_amd.plm.rbm_log_partition (same arguments, same return value; no launches, so no callback)."""
    res = ais(g, c, W, n_chains, n_temps, sweeps_per_temp, betas, seed)
    for key in ("max_x", "start_margin", "start_maxu"):
        res.pop(key)
    if not hidden:
        res.pop("hidden")
    if betas is None or float(np.asarray(betas, F32)[-1]) == 1.0:
        w = np.exp(res["log_w"] - res["log_w"].max())
        res["mean_score"] = float((w / w.sum()) @ tw.score(res["states"], g, c, W))
        res["entropy"] = res["log_z"] - res["mean_score"]
    return res
