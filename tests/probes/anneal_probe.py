#!/usr/bin/env python3
"""Speed of the annealing and greedy sweeps (DESIGN_NEXT_ROWS.md section 9.13) beside the sampler's sweep, which runs the
same pipeline, at (L, C) = (300, 65 536) and (100, 65 536), q = 21, in one process.  Every call uploads the model,
expands it, sweeps and downloads; the time of a sweep is the difference of two calls that differ in the number of sweeps
only (host clock, same start states), divided by the sweeps between them: one warm-up pair, then REPS pairs (median, min,
max), the three kinds interleaved so that they meet the same state of the device.
  sampler    plm.sample with burn_in = 26 (L = 300) or 162 (L = 100) against burn_in = 2: about 0.3 s of sweeps
  annealing  plm.anneal with as many steps against 2 steps at beta = 1, one sweep each, no greedy sweeps
  greedy     plm.anneal without steps, 2 greedy sweeps against 1: from uniform random starts every chain moves in the
             first sweep, so no workgroup leaves before the second; chains converge, so the window cannot be longer and
             this figure is the roughest of the three
PLM_SAMPLE_FORM=direct in the environment measures the other form.

    python tests/probes/anneal_probe.py [REPS] [OUT.json]
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
B_SHORT, B_LONG = 2, {300: 26, 100: 162}      # about 0.3 s of sweeps between the two calls


def model(L, q=Q, seed=0):
    rng = np.random.default_rng(seed + L)
    h = rng.normal(size=(L, q)).astype(np.float32)
    J = rng.normal(scale=0.05, size=(L * (L - 1) // 2, q, q)).astype(np.float32)
    return h, J


def stats(ts):
    return dict(median_ms=1e3 * float(np.median(ts)), min_ms=1e3 * min(ts), max_ms=1e3 * max(ts), reps=len(ts))


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


def table(reps, out_path):
    rows = {}
    for L, C in ((300, 65536), (100, 65536)):
        h, J = model(L)
        x0 = np.random.default_rng(1).integers(0, Q, size=(C, L)).astype(np.int8)
        kinds = dict(
            sampler=lambda n: plm.sample(h, J, Q, C, burn_in=n, seed=1, start=x0, energies=False),
            annealing=lambda n: plm.anneal(h, J, Q, C, betas=np.ones(n, np.float32), max_greedy=0, seed=1, start=x0,
                                           energies=False),
            greedy=lambda n: plm.anneal(h, J, Q, C, n_steps=0, max_greedy=n, start=x0, energies=False))
        spans = dict(sampler=(B_SHORT, B_LONG[L]), annealing=(B_SHORT, B_LONG[L]), greedy=(1, 2))
        sweep = {k: [] for k in kinds}
        for rep in range(reps + 1):                                      # the first round is the warm-up
            for k, f in kinds.items():
                lo, hi = spans[k]
                a, _ = timed(lambda: f(lo))
                b, r = timed(lambda: f(hi))
                if k == "greedy":
                    assert r["last_move"].min() >= 1                     # every chain moved in the first sweep
                if rep:
                    sweep[k].append((b - a) / (hi - lo))
        r = {k: stats(v) for k, v in sweep.items()}
        for k in ("annealing", "greedy"):
            r[k + "_over_sampler"] = r[k]["median_ms"] / r["sampler"]["median_ms"]
        rows["L%d_C%d" % (L, C)] = r
        print("L=%d C=%d  one sweep, median (min, max) of %d: sampler %.2f (%.2f, %.2f) ms, annealing %.2f (%.2f, %.2f) ms = "
              "%.3f of the sampler's, greedy %.2f (%.2f, %.2f) ms = %.3f"
              % (L, C, reps, r["sampler"]["median_ms"], r["sampler"]["min_ms"], r["sampler"]["max_ms"],
                 r["annealing"]["median_ms"], r["annealing"]["min_ms"], r["annealing"]["max_ms"], r["annealing_over_sampler"],
                 r["greedy"]["median_ms"], r["greedy"]["min_ms"], r["greedy"]["max_ms"], r["greedy_over_sampler"]), flush=True)
        del h, J, x0
    if out_path:
        with open(out_path, "w") as f:
            json.dump(dict(form=os.environ.get("PLM_SAMPLE_FORM", "tiled"), rows=rows), f, indent=1)


if __name__ == "__main__":
    table(int(sys.argv[1]) if len(sys.argv) > 1 else 10, sys.argv[2] if len(sys.argv) > 2 else None)
