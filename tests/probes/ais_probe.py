#!/usr/bin/env python3
"""Cost of annealed importance sampling (plm.log_partition, DESIGN_NEXT_ROWS.md section 9.8) beside the plain sampler,
q = 21, C = 65 536, L = 300 and L = 100.  A call uploads the model, expands it, anneals and downloads; the time of an AIS
sweep is the difference of two calls with K_LONG and K_SHORT steps of one sweep each (each in one launch), divided by the
steps between them: host clock, one warm-up pair, then REPS pairs (median, min, max).  plm.sample's sweep is measured the
same way in the same run (burn_in = K_LONG and K_SHORT from the start rule).  The first launch also draws the start
states and makes the measuring pass: a one-step AIS call (ending at beta = 0.5, so that no energies of the final states
are computed) beside a plm.sample call with one sweep from the start rule.  Last, the convergence table of the fitted
L = 24 model of tests/golden: log Z, its standard error and the effective sample size over K and C.

    python tests/probes/ais_probe.py [REPS] [OUT.json]
    python tests/probes/ais_probe.py --one L C K        one AIS call, for a profiler run around it
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from evcouplings_amd import plm  # noqa: E402

Q = 21
K_SHORT, K_LONG = 2, 10


def model(L, q=Q, seed=0):
    rng = np.random.default_rng(seed + L)
    h = rng.normal(size=(L, q)).astype(np.float32)
    J = rng.normal(scale=0.05, size=(L * (L - 1) // 2, q, q)).astype(np.float32)
    return h, J


def stats(ts):
    return dict(median_ms=1e3 * float(np.median(ts)), min_ms=1e3 * min(ts), max_ms=1e3 * max(ts), reps=len(ts))


def ais_call(h, J, C, K, last=1.0):
    betas = (np.arange(K + 1) / K * last).astype(np.float32)
    t0 = time.perf_counter()
    plm.log_partition(h, J, Q, n_chains=C, betas=betas, seed=1, steps_per_launch=K)
    return time.perf_counter() - t0


def sample_call(h, J, C, sweeps):
    t0 = time.perf_counter()
    plm.sample(h, J, Q, C, burn_in=sweeps, seed=1, energies=False)
    return time.perf_counter() - t0


def speed(reps):
    rows = {}
    for L, C in ((300, 65536), (100, 65536)):
        h, J = model(L)
        ais_call(h, J, C, K_SHORT), ais_call(h, J, C, K_LONG), sample_call(h, J, C, K_SHORT), sample_call(h, J, C, K_LONG)
        ais, plain, first, one = [], [], [], []
        for _ in range(reps):
            a, b = ais_call(h, J, C, K_SHORT), ais_call(h, J, C, K_LONG)
            c, d = sample_call(h, J, C, K_SHORT), sample_call(h, J, C, K_LONG)
            ais.append((b - a) / (K_LONG - K_SHORT))
            plain.append((d - c) / (K_LONG - K_SHORT))
            first.append(ais_call(h, J, C, 1, last=0.5))
            one.append(sample_call(h, J, C, 1))
        r = dict(ais_sweep=stats(ais), sample_sweep=stats(plain), ais_call_with_1_step=stats(first),
                 sample_call_with_1_sweep=stats(one))
        r["ratio"] = r["ais_sweep"]["median_ms"] / r["sample_sweep"]["median_ms"]
        r["measuring_pass_ms"] = r["ais_call_with_1_step"]["median_ms"] - r["sample_call_with_1_sweep"]["median_ms"]
        rows["L%d_C%d" % (L, C)] = r
        print("L=%d C=%d  AIS sweep %.2f ms (min %.2f, max %.2f), plm.sample sweep %.2f ms (min %.2f, max %.2f), ratio %.3f; "
              "one-step AIS call %.1f ms, one-sweep sample call %.1f ms: start measuring pass %.1f ms (%d reps)"
              % (L, C, r["ais_sweep"]["median_ms"], r["ais_sweep"]["min_ms"], r["ais_sweep"]["max_ms"],
                 r["sample_sweep"]["median_ms"], r["sample_sweep"]["min_ms"], r["sample_sweep"]["max_ms"], r["ratio"],
                 r["ais_call_with_1_step"]["median_ms"], r["sample_call_with_1_sweep"]["median_ms"], r["measuring_pass_ms"],
                 reps), flush=True)
    return rows


def convergence():
    d = np.load(os.path.join(ROOT, "tests", "golden", "hip_fit_L24.npz"))
    h, J = d["hi"], d["jij"]
    rows = []
    for C in (1024, 4096):
        for K in (32, 128, 512):
            t0 = time.perf_counter()
            r = plm.log_partition(h, J, h.shape[1], n_chains=C, n_temps=K, seed=1)
            secs = time.perf_counter() - t0
            rows.append(dict(C=C, K=K, log_z=r["log_z"], log_z_se=r["log_z_se"], ess=r["ess"], entropy=r["entropy"],
                             log_z0=r["log_z0"], seconds=secs))
            print("hip_fit_L24  C=%d K=%d  log Z %.4f +- %.4f, ESS %.0f, entropy %.3f (log Z0 %.4f), %.3f s"
                  % (C, K, r["log_z"], r["log_z_se"], r["ess"], r["entropy"], r["log_z0"], secs), flush=True)
    return rows


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        L, C, K = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
        print("AIS call with %d steps: %.3f s" % (K, ais_call(*model(L), C, K)))
    else:
        reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
        out = dict(convergence=convergence(), speed=speed(reps))
        if len(sys.argv) > 2:
            with open(sys.argv[2], "w") as f:
                json.dump(out, f, indent=1)
