#!/usr/bin/env python3
"""Speed and convergence of annealed importance sampling for the restricted Boltzmann machine (plm_rbm_ais,
DESIGN_NEXT_ROWS.md section 9.25) at L = 300, q = 21, M = 128.  A probe, not a test; it reads nothing outside the tree.

  step         one AIS step (one sweep) of 65 536 chains: the difference of two plm.rbm_log_partition calls with 10 and 2
               steps in one launch each (host clock, so uploads, the expansion, the start rule and the download cancel),
               median of 10 with min and max; next to it, in the same process, one plm.rbm_sample step of as many chains
               from the start rule, measured the same way, and the ratio of the two medians
  convergence  a model fitted to N_FIT sequences for a few tens of epochs: log_z, its standard error and the effective
               sample size at K = 32, 128, 512 for C = 1024 and 4096

    python tests/probes/rbm_ais_probe.py [OUT.json]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from evcouplings_amd import plm  # noqa: E402

L, Q, M = 300, 21, 128
C_STEP, LONG, SHORT, REPS = 65536, 10, 2, 10
N_FIT, C_FIT, E_FIT = 5000, 4096, 50


def problem(seed=0):
    rng = np.random.default_rng(seed)
    fi = rng.dirichlet(np.full(Q, 0.3), size=L)                    # a few frequent letters per site, as in a family
    msa = np.stack([rng.choice(Q, size=N_FIT, p=fi[i]) for i in range(L)], axis=1).astype(np.int8)
    g = np.log(fi + 1e-3).astype(np.float32)
    c = rng.normal(0.0, 0.5, M).astype(np.float32)
    W = rng.normal(0.0, 1.0 / np.sqrt(L), (M, L, Q)).astype(np.float32)
    return msa, g, c, W


def _per_unit(call):
    """milliseconds per step from the difference of a call with LONG and one with SHORT steps"""
    call(SHORT)                                                    # warm-up: code objects, allocator
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call(SHORT)
        a = time.perf_counter() - t0
        t0 = time.perf_counter()
        call(LONG)
        b = time.perf_counter() - t0
        ts.append(1e3 * (b - a) / (LONG - SHORT))
    return dict(median_ms=float(np.median(ts)), min_ms=min(ts), max_ms=max(ts), reps=REPS)


def steps(g, c, W):
    ais = _per_unit(lambda K: plm.rbm_log_partition(g, c, W, Q, n_chains=C_STEP, n_temps=K, seed=2, steps_per_launch=K))
    print("ais: one step of %d chains: %.3f ms (min %.3f, max %.3f; %d repetitions of %d against %d steps)"
          % (C_STEP, ais["median_ms"], ais["min_ms"], ais["max_ms"], REPS, LONG, SHORT), flush=True)
    gibbs = _per_unit(lambda B: plm.rbm_sample(g, c, W, Q, C_STEP, burn_in=B, seed=2))
    print("yardstick: one plm.rbm_sample step of %d chains: %.3f ms (min %.3f, max %.3f)"
          % (C_STEP, gibbs["median_ms"], gibbs["min_ms"], gibbs["max_ms"]), flush=True)
    ratio = ais["median_ms"] / gibbs["median_ms"]
    print("ratio of the medians: %.3f" % ratio, flush=True)
    return dict(ais_step=ais, rbm_sample_step=gibbs, ratio=ratio)


def convergence(msa, g):
    rng = np.random.Generator(np.random.PCG64(0))
    W0 = rng.normal(0.0, 0.01, (M, L, Q)).astype(np.float32)
    t0 = time.perf_counter()
    fit = plm.rbm_fit(msa, np.ones(len(msa), np.float32), Q, g, np.zeros(M, np.float32), W0, C_FIT, E_FIT, lr=0.1,
                      lambda_w=1e-3, seed=1)
    print("fit: %d sequences, %d chains, %d epochs in %.2f s" % (len(msa), C_FIT, E_FIT, time.perf_counter() - t0), flush=True)
    rows = []
    for C in (1024, 4096):
        for K in (32, 128, 512):
            t0 = time.perf_counter()
            r = plm.rbm_log_partition(fit["g"], fit["c"], fit["W"], Q, n_chains=C, n_temps=K, seed=3)
            rows.append(dict(C=C, K=K, log_z=r["log_z"], log_z_se=r["log_z_se"], ess=r["ess"], entropy=r["entropy"],
                             seconds=time.perf_counter() - t0))
            print("convergence: C = %4d, K = %3d: log Z = %.4f +- %.4f, ESS = %.1f, entropy = %.3f (%.2f s)"
                  % (C, K, r["log_z"], r["log_z_se"], r["ess"], r["entropy"], rows[-1]["seconds"]), flush=True)
    return rows


if __name__ == "__main__":
    msa, g, c, W = problem()
    out = dict(shape=dict(L=L, q=Q, M=M, C_step=C_STEP, N_fit=N_FIT, C_fit=C_FIT, epochs=E_FIT), steps=steps(g, c, W),
               convergence=convergence(msa, g))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
