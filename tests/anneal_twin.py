"""numpy twin of simulated annealing and greedy ascent (plm_anneal, DESIGN_NEXT_ROWS.md section 9.13) on top of
tests/sampler_twin.py: the conditional energies U in float32 from the field over j = 0 .. L-1, the annealing draw in
float64 (tw.draw) on the Philox uniform of (seed, chain, sweep, site), the greedy rule and the tracked gain exactly as the
contract states them (float32 comparisons, float64 differences), the checkpoints.  Not a test module."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_twin as tw  # noqa: E402


def site_energies(x, hf, Wf, i):
    """U[c, a] = h_i(a) + sum_{j != i} J_ij(a, x_cj) in float32, from the field, j = 0 .. L-1 (compare
    ais_twin.coupling_sums, which starts from zero).  hf: float32 [L, q]; Wf: float32 [L, L, q, q] (tw.dense)."""
    C, L = x.shape
    U = np.tile(hf[i], (C, 1))
    for j in range(L):
        if j != i:
            U = U + Wf[i, j][:, x[:, j]].T
    assert U.dtype == np.float32
    return U


def greedy_update(U, x_i, ok):
    """(new states, moved) of one greedy site update: a* = the first allowed state with the largest U; the chain moves
    iff U[a*] > U[x_i] in float32."""
    chains = np.arange(U.shape[0])
    a_star = np.argmax(np.where(ok[None, :], U, -np.inf), axis=1)        # argmax returns the first maximum
    moved = U[chains, a_star] > U[chains, x_i]
    return np.where(moved, a_star, x_i), moved


def anneal(hi, jij, q, n_chains, betas=None, n_steps=100, sweeps_per_step=1, max_greedy=100, seed=0, start=None, fixed=None,
           allowed=None, first_sweep=0, steps_per_launch=0, callback=None, energies=True, device=0, trace=False):
    """Twin of evcouplings_amd.plm.anneal (same arguments, same return value; no launches, so steps_per_launch and the
    callback do nothing).  trace=True adds `steps`: states [K + 1, C, L] at the start and after every annealing step
    (before the greedy phase), margin and maxarg [K + 1, C, L], the twin's draw diagnostics per (step, chain, site), the
    worst over the sweeps of the step, with the start rule first: what test_gpu_sampler._explained takes."""
    from evcouplings_amd import plm
    hf = np.asarray(hi, np.float32).reshape(-1, q)
    L = hf.shape[0]
    h = hf.astype(np.float64)
    W = tw.dense(np.asarray(jij, np.float32).astype(np.float64), L, q)
    Wf = W.astype(np.float32)
    b = plm.annealing_schedule(int(n_steps)) if betas is None else np.asarray(betas, np.float32).reshape(-1)
    K, n, C, G = len(b), int(sweeps_per_step), int(n_chains), int(max_greedy)
    ok = tw._mask(allowed, q)
    free = [i for i in range(L) if fixed is None or not np.asarray(fixed).reshape(L)[i]]
    chains = np.arange(C)
    margin0, maxarg0 = np.ones((C, L)), np.zeros((C, L))
    if start is None:
        x = tw.start_states(h, C, seed, 1.0, allowed, margin=margin0, maxbu=maxarg0)
    else:
        x = np.array(start, np.int64).reshape(C, L)
    gain = np.zeros(C)
    best, best_gain, best_at = x.copy(), np.zeros(C), np.zeros(C, np.int32)

    def checkpoint(no):
        up = gain > best_gain
        best[up] = x[up]
        best_gain[up] = gain[up]
        best_at[up] = no

    steps = dict(states=[x.copy()], margin=[margin0], maxarg=[maxarg0])
    for k in range(1, K + 1):
        margin, maxarg = np.ones((C, L)), np.zeros((C, L))
        for s in range(n):
            sweep = int(first_sweep) + (k - 1) * n + s
            for i in free:
                U = site_energies(x, hf, Wf, i)
                a, mg, mb = tw.draw(U.astype(np.float64), tw.uniform(seed, chains, sweep, i), float(b[k - 1]), allowed)
                gain = gain + (U[chains, a].astype(np.float64) - U[chains, x[:, i]].astype(np.float64))
                x[:, i] = a
                margin[:, i] = np.minimum(margin[:, i], mg)
                maxarg[:, i] = np.maximum(maxarg[:, i], mb)
        checkpoint(k)
        steps["states"].append(x.copy())
        steps["margin"].append(margin)
        steps["maxarg"].append(maxarg)
    last_move, converged = np.zeros(C, np.int32), np.zeros(C, bool)
    for t in range(1, G + 1):
        moved_any = np.zeros(C, bool)
        for i in free:
            U = site_energies(x, hf, Wf, i)
            a, moved = greedy_update(U, x[:, i], ok)
            gain = gain + (U[chains, a].astype(np.float64) - U[chains, x[:, i]].astype(np.float64))
            x[:, i] = a
            moved_any |= moved
        last_move[moved_any] = t
        converged |= ~moved_any
        if converged.all():                 # converged chains are fixed points: further sweeps change nothing
            break
    if G >= 1:
        checkpoint(K + 1)
    out = dict(states=x.astype(np.int8), gain=gain, best=best.astype(np.int8), best_gain=best_gain, best_at=best_at,
               last_move=last_move, converged=converged,
               energies=tw.hamiltonians(x, h, W) if energies else None,
               best_energies=tw.hamiltonians(best, h, W) if energies else None, steps_done=K, status="converged")
    if trace:
        out["steps"] = {k: np.array(v) for k, v in steps.items()}
    return out
