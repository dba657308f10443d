#!/usr/bin/env python3
"""Cost of parallel tempering (plm.parallel_tempering, DESIGN_NEXT_ROWS.md section 9.9) beside the plain sampler, q = 21,
C R = 65 536 walkers (R = 16, linear ladder to 1), L = 300 and L = 100.  A call uploads the model, expands it, starts the
walkers, runs its rounds and downloads; the time of a round (one sweep of every walker, one exchange pass) is the
difference of two calls with K_LONG and K_SHORT rounds, divided by the rounds between them: host clock, one warm-up pair,
then REPS pairs (median, min, max).  plm.sample's sweep at 65 536 chains is measured the same way in the same run.  Last,
the fitted L = 24 model of tests/golden: acceptance rates, log Z and the time of a round over the ladder size.

    python tests/probes/pt_probe.py [REPS] [OUT.json]
    python tests/probes/pt_probe.py --one L LADDERS ROUNDS     one call, for a profiler run around it
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from evcouplings_amd import plm  # noqa: E402

Q, R = 21, 16
K_SHORT, K_LONG = 2, 10


def model(L, q=Q, seed=0):
    rng = np.random.default_rng(seed + L)
    h = rng.normal(size=(L, q)).astype(np.float32)
    J = rng.normal(scale=0.05, size=(L * (L - 1) // 2, q, q)).astype(np.float32)
    return h, J


def stats(ts):
    return dict(median_ms=1e3 * float(np.median(ts)), min_ms=1e3 * min(ts), max_ms=1e3 * max(ts), reps=len(ts))


def pt_call(h, J, ladders, rounds, n_rungs=R):
    t0 = time.perf_counter()
    plm.parallel_tempering(h, J, h.shape[1], ladders, plm.tempering_ladder(n_rungs), burn_in=rounds, seed=1)
    return time.perf_counter() - t0


def sample_call(h, J, C, sweeps):
    t0 = time.perf_counter()
    plm.sample(h, J, h.shape[1], C, burn_in=sweeps, seed=1, energies=False)
    return time.perf_counter() - t0


def speed(reps):
    rows = {}
    for L, walkers in ((300, 65536), (100, 65536)):
        h, J = model(L)
        C = walkers // R
        pt_call(h, J, C, K_SHORT), pt_call(h, J, C, K_LONG), sample_call(h, J, walkers, K_SHORT), sample_call(h, J, walkers, K_LONG)
        rnd, plain = [], []
        for _ in range(reps):
            a, b = pt_call(h, J, C, K_SHORT), pt_call(h, J, C, K_LONG)
            c, d = sample_call(h, J, walkers, K_SHORT), sample_call(h, J, walkers, K_LONG)
            rnd.append((b - a) / (K_LONG - K_SHORT))
            plain.append((d - c) / (K_LONG - K_SHORT))
        r = dict(pt_round=stats(rnd), sample_sweep=stats(plain))
        r["ratio"] = r["pt_round"]["median_ms"] / r["sample_sweep"]["median_ms"]
        rows["L%d_W%d" % (L, walkers)] = r
        print("L=%d walkers=%d (R=%d)  round %.2f ms (min %.2f, max %.2f), plm.sample sweep %.2f ms (min %.2f, max %.2f), "
              "ratio %.3f (%d reps)" % (L, walkers, R, r["pt_round"]["median_ms"], r["pt_round"]["min_ms"],
                                        r["pt_round"]["max_ms"], r["sample_sweep"]["median_ms"], r["sample_sweep"]["min_ms"],
                                        r["sample_sweep"]["max_ms"], r["ratio"], reps), flush=True)
    return rows


def fitted(reps):
    d = np.load(os.path.join(ROOT, "tests", "golden", "hip_fit_L24.npz"))
    h, J = d["hi"], d["jij"]
    q = h.shape[1]
    rows = []
    for n_rungs, C in ((4, 512), (8, 512), (16, 512), (8, 4096)):
        r = plm.log_partition_tempered(h, J, q, C, plm.tempering_ladder(n_rungs), burn_in=20, n_snapshots=4, thin=5, seed=1)
        pt_call(h, J, C, 10, n_rungs), pt_call(h, J, C, 110, n_rungs)
        ts = [(pt_call(h, J, C, 110, n_rungs) - pt_call(h, J, C, 10, n_rungs)) / 100 for _ in range(reps)]
        rows.append(dict(R=n_rungs, C=C, log_z=r["log_z"], log_z_se=r["log_z_se"], acceptance=[float(v) for v in r["acceptance"]],
                         round=stats(ts)))
        print("hip_fit_L24  R=%d C=%d  log Z %.4f +- %.4f, acceptance %s, round %.3f ms (min %.3f, max %.3f)"
              % (n_rungs, C, r["log_z"], r["log_z_se"], " ".join("%.3f" % v for v in r["acceptance"]),
                 rows[-1]["round"]["median_ms"], rows[-1]["round"]["min_ms"], rows[-1]["round"]["max_ms"]), flush=True)
    return rows


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        L, C, K = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
        print("call with %d rounds: %.3f s" % (K, pt_call(*model(L), C, K)))
    else:
        reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
        out = dict(fitted=fitted(reps), speed=speed(reps))
        if len(sys.argv) > 2:
            with open(sys.argv[2], "w") as f:
                json.dump(out, f, indent=1)
