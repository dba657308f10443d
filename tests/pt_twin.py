"""numpy twin of parallel tempering (plm_pt, DESIGN_NEXT_ROWS.md section 9.9) on top of tests/sampler_twin.py and
tests/ais_twin.py: the coupling sums U in float32 in the order j = 0 .. L-1, the argument of the draw fadd(h, fmul(beta,
U)) in float32 with the walker's own beta, the draw in float64 (tw.draw), the tracked coupling energy, the exchange
difference and the decision in float64.  It records, per draw and per exchange decision, the margin the comparisons with
the GPU need.  Not a test module."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ais_twin as at  # noqa: E402
import sampler_twin as tw  # noqa: E402


def uniform_f32(seed, c0, c1, c2, c3):
    """The sampler's uniform in float32, u = min(((word0 >> 8) + 0.5) 2^-24, largest float32 below 1), of the Philox
    counter (c0, c1, c2, c3), widened to float64."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w0 = tw.philox4x32_10(c0, c1, c2, c3, seed & 0xFFFFFFFF, seed >> 32)[0]
    u = ((w0 >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    return np.minimum(u, np.float32(0.99999994)).astype(np.float64)


def exchange_rule(delta, u):
    """Accept iff delta >= 0 or u < exp(delta), in float64."""
    with np.errstate(over="ignore"):
        return (delta >= 0.0) | (u < np.exp(delta))


def measure(x, Wf):
    """E = 1/2 sum_i (double)U_i[x_i], summed in site order."""
    Cn, L = x.shape
    rows = np.arange(Cn)
    E = np.zeros(Cn)
    for i in range(L):
        E = E + at.coupling_sums(x, Wf, i)[rows, x[:, i]].astype(np.float64)
    return 0.5 * E


class State:
    """The walkers of C ladders of R rungs: x [C R, L] int64, rung_of_slot and slot_of_rung [C, R], E [C R]."""

    def __init__(self, x, ros, E):
        self.x, self.ros, self.E = x, ros, E
        self.sor = np.argsort(ros, axis=1)

    def in_rung_order(self):
        """(states [C, R, L], E [C, R]) of the walker at every rung."""
        C, R = self.ros.shape
        w = (np.arange(C)[:, None] * R + self.sor).ravel()
        return self.x[w].reshape(C, R, -1), self.E[w].reshape(C, R)


def start_state(hf, Wf, C, R, seed, start=None):
    """The start of the definition: None, or (states, rungs or None, e_j or None)."""
    if start is None:
        x = tw.start_states(hf.astype(np.float64), C * R, seed)
        return State(x, np.tile(np.arange(R), (C, 1)), measure(x, Wf))
    parts = tuple(start) + (None,) * (3 - len(start))
    x = np.array(parts[0], np.int64).reshape(C * R, -1)
    ros = np.tile(np.arange(R), (C, 1)) if parts[1] is None else np.array(parts[1], np.int64).reshape(C, R)
    assert (np.sort(ros, axis=1) == np.arange(R)[None, :]).all(), "rungs must be a permutation within each ladder"
    E = measure(x, Wf) if parts[2] is None else np.array(parts[2], np.float64).reshape(C * R)
    return State(x, ros, E)


def one_round(st, hf, Wf, b, g, n, seed, rule=exchange_rule):
    """Round g in place on st.  Returns the diagnostics: margin and maxarg [C R, L] of the draws (the worst of the n
    sweeps), and decision [C, R - 1] = |u - exp(delta)| of every exchange that was attempted (inf where none was, and
    where delta >= 0 decides alone), accepted [C, R - 1] bool."""
    CR, L = st.x.shape
    C, R = st.ros.shape
    walkers = np.arange(CR)
    beta = b[st.ros.ravel()][:, None]                                   # float32, one per walker
    margin, maxarg = np.ones((CR, L)), np.zeros((CR, L))
    for s in range(n):
        for i in range(L):
            U = at.coupling_sums(st.x, Wf, i)
            arg = hf[i][None, :] + beta * U                             # float32: one rounding per operation
            assert arg.dtype == np.float32
            a, mg, mb = tw.draw(arg.astype(np.float64), tw.uniform(seed, walkers, g * n + s, i))
            st.E = st.E + (U[walkers, a].astype(np.float64) - U[walkers, st.x[:, i]].astype(np.float64))
            st.x[:, i] = a
            margin[:, i] = np.minimum(margin[:, i], mg)
            maxarg[:, i] = np.maximum(maxarg[:, i], mb)
    decision, accepted = np.full((C, max(R - 1, 0)), np.inf), np.zeros((C, max(R - 1, 0)), bool)
    ladders = np.arange(C)
    for r in range(g % 2, R - 1, 2):
        sa, sb = st.sor[:, r].copy(), st.sor[:, r + 1].copy()
        delta = (np.float64(b[r + 1]) - np.float64(b[r])) * (st.E[ladders * R + sa] - st.E[ladders * R + sb])
        u = uniform_f32(seed, ladders, 1, g, r)
        acc = rule(delta, u)
        with np.errstate(over="ignore"):
            decision[:, r] = np.where(delta >= 0.0, np.inf, np.abs(u - np.exp(delta)))
        accepted[:, r] = acc
        st.sor[acc, r], st.sor[acc, r + 1] = sb[acc], sa[acc]
        st.ros[ladders[acc], sa[acc]] = r + 1
        st.ros[ladders[acc], sb[acc]] = r
    return dict(margin=margin, maxarg=maxarg, decision=decision, accepted=accepted)


def pt(hi, jij, q, n_ladders, betas, rounds, sweeps_per_round=1, seed=0, start=None, first_round=0, rule=exchange_rule,
       trace=False):
    """`rounds` rounds from the start.  Returns the State reached, accepts and attempts [R - 1]; trace=True adds, per
    round (the start first, with the diagnostics of the start rule): walkers [rounds + 1, C R, L], rungs, e_j, margin,
    maxarg, and per round decision and accepted [rounds, C, R - 1]."""
    hf = np.asarray(hi, np.float32).reshape(-1, q)
    L = hf.shape[0]
    Wf = tw.dense(np.asarray(jij, np.float32).astype(np.float64), L, q).astype(np.float32)
    b = np.asarray(betas, np.float32).reshape(-1)
    C, R, n = int(n_ladders), len(b), int(sweeps_per_round)
    st = start_state(hf, Wf, C, R, seed, start)
    accepts, attempts = np.zeros(max(R - 1, 0), np.int64), np.zeros(max(R - 1, 0), np.int64)
    tr = None
    if trace:
        m0, a0 = np.ones((C * R, L)), np.zeros((C * R, L))
        if start is None:
            tw.start_states(hf.astype(np.float64), C * R, seed, margin=m0, maxbu=a0)
        tr = dict(walkers=[st.x.copy()], rungs=[st.ros.copy()], e_j=[st.E.copy()], margin=[m0], maxarg=[a0], decision=[],
                  accepted=[])
    for k in range(int(rounds)):
        g = int(first_round) + k
        d = one_round(st, hf, Wf, b, g, n, seed, rule)
        accepts += d["accepted"].sum(axis=0)
        attempts[g % 2::2] += C
        if trace:
            tr["walkers"].append(st.x.copy())
            tr["rungs"].append(st.ros.copy())
            tr["e_j"].append(st.E.copy())
            for f in ("margin", "maxarg", "decision", "accepted"):
                tr[f].append(d[f])
    out = dict(state=st, accepts=accepts, attempts=attempts)
    if trace:
        out["trace"] = {k: np.array(v) for k, v in tr.items()}
    return out


def parallel_tempering(hi, jij, q, n_ladders, betas, burn_in=10, n_snapshots=1, thin=1, sweeps_per_round=1, seed=0,
                       all_rungs=False, start=None, first_round=0, callback=None, device=0):
    """Twin of evcouplings_amd.plm.parallel_tempering (same arguments, same return value; no callback)."""
    hf = np.asarray(hi, np.float32).reshape(-1, q)
    L = hf.shape[0]
    h = hf.astype(np.float64)
    Wd = tw.dense(np.asarray(jij, np.float32).astype(np.float64), L, q)
    Wf = Wd.astype(np.float32)
    b = np.asarray(betas, np.float32).reshape(-1)
    C, R, K, n = int(n_ladders), len(b), int(n_snapshots), int(sweeps_per_round)
    st = start_state(hf, Wf, C, R, seed, start)
    accepts, attempts = np.zeros(R - 1, np.int64), np.zeros(R - 1, np.int64)
    xs, es = [], []
    g = int(first_round)
    for k in range(K):
        for _ in range(burn_in if k == 0 else thin):
            accepts += one_round(st, hf, Wf, b, g, n, seed)["accepted"].sum(axis=0)
            attempts[g % 2::2] += C
            g += 1
        x, e = st.in_rung_order()
        xs.append(x if all_rungs else x[:, -1])
        es.append(e if all_rungs else e[:, -1])
    samples, e_j = np.array(xs).astype(np.int8), np.array(es)
    en = tw.hamiltonians(samples.reshape(-1, L).astype(np.int64), h, Wd).reshape(samples.shape[:-1] + (3,))
    with np.errstate(divide="ignore", invalid="ignore"):
        acceptance = accepts / attempts.astype(np.float64)
    return dict(samples=samples, energies=en, e_j=e_j, accepts=accepts, attempts=attempts, acceptance=acceptance,
                walkers=(st.x.astype(np.int8), st.ros.ravel().astype(np.int32), st.E.copy()), rounds_done=g - int(first_round),
                status="converged")


# ---- stationary starts on the enumerable models of ais_twin -----------------------------------------------------------

STATIONARY_BETAS = (0.0, 0.5, 1.0, 2.0)
STATIONARY_C, STATIONARY_ROUNDS = 16384, 12


def rung_distributions(h, J, q, betas):
    """p_beta over tw.all_states(L, q) for every beta of the ladder, [R, q^L], by enumeration in float64."""
    h = np.asarray(h, np.float32).astype(np.float64).reshape(-1, q)
    L = h.shape[0]
    en = tw.hamiltonians(tw.all_states(L, q), h, tw.dense(np.asarray(J, np.float32).astype(np.float64), L, q))
    out = []
    for beta in np.asarray(betas, np.float32).astype(np.float64):
        e = en[:, 2] + beta * en[:, 1]
        p = np.exp(e - e.max())
        out.append(p / p.sum())
    return np.array(out)


def stationary_start(h, J, q, betas, n_ladders, rng_seed):
    """Walker states [C R, L] int8 with slot r of every ladder an exact draw of p_{beta_r} (numpy's generator), rung = slot."""
    L = np.asarray(h).reshape(-1, q).shape[0]
    p = rung_distributions(h, J, q, betas)
    st = tw.all_states(L, q)
    rng = np.random.default_rng(rng_seed)
    x = np.zeros((n_ladders, len(p), L), np.int8)
    for r in range(len(p)):
        x[:, r] = st[rng.choice(len(st), size=n_ladders, p=p[r])]
    return x.reshape(n_ladders * len(p), L)


def rung_chi2(samples, p, q):
    """[(chi2, dof)] of the rows samples[:, r] against p[r], for every rung."""
    out = []
    for r in range(p.shape[0]):
        counts = np.bincount(tw.state_index(samples[:, r].astype(np.int64), q), minlength=p.shape[1])
        out.append(tw.chi2_counts(counts, p[r], samples.shape[0]))
    return out
