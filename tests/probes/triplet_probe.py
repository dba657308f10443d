#!/usr/bin/env python3
"""Cost of the three-site statistics (plm.triplet_scan, plm.triplet_stats; DESIGN_NEXT_ROWS.md section 9.12), q = 21,
N = 50 000.  A call validates and transposes the alignment on the host, uploads, runs and downloads; host clock around
the whole call, one warm-up call, then REPS calls (median, min, max).  A full scan at L = 300 is 4 455 100 triplets and
takes seconds, so the number of calls of a case is cut to what fits SECONDS of wall time per case (estimated from the
L = 100 scan, which runs first) and printed with the result; its warm-up is the L = 100 scan of the same weights.
  scan:     every triplet of L = 100 and of L = 300, with unit weights (32-bit cells) and with the weights
            1 / plm.reweight (64-bit cells);
  bound:    HBM traffic of one new column per triplet, N bytes, at HBM_TBS -- which LDS atomics do not get near;
  listed:   plm.triplet_stats of 1 000 random triplets (counts, freq and connected wanted), L = 300;
  contention: the L = 100 scan on an alignment whose columns are all constant (every lane of a wave on one cell) and on
            one with a dominant state of 90 % per column, against the random one.

    python tests/probes/triplet_probe.py [REPS] [SECONDS] [OUT.json]
    python tests/probes/triplet_probe.py --one      one L = 100 scan of each weight kind and one listed call after a
                                                    warm-up, for a profiler run around it
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from evcouplings_amd import plm  # noqa: E402

Q, N = 21, 50000
HBM_TBS = 8.0        # peak HBM bandwidth of the MI355X, TB/s


def families(n, L, seed, n_families=2500, rate=0.3):
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, Q, size=(n_families, L), dtype=np.int8)
    rows = anc[rng.integers(0, n_families, size=n)]
    mut = rng.random((n, L)) < rate
    rows[mut] = rng.integers(0, Q, size=int(mut.sum()), dtype=np.int8)
    return rows


def timed(fn, reps, warm=True):
    if warm:
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return dict(median_ms=1e3 * float(np.median(ts)), min_ms=1e3 * min(ts), max_ms=1e3 * max(ts), reps=len(ts))


def show(name, st, extra=""):
    print("%s %.1f ms (min %.1f, max %.1f, %d calls)%s" % (name, st["median_ms"], st["min_ms"], st["max_ms"], st["reps"],
                                                          extra), flush=True)


def n_triplets(L):
    return L * (L - 1) * (L - 2) // 6


def bound_ms(L):
    return 1e3 * n_triplets(L) * N / (HBM_TBS * 1e12)


def one():
    msa = families(N, 100, seed=100)
    w = (1.0 / plm.reweight(msa, 0.8)).astype(np.float32)
    trip = plm.triplet_index(100)[::162][:1000]
    for _ in range(2):
        plm.triplet_scan(msa, Q, skip_state=0)
        plm.triplet_scan(msa, Q, weights=w, skip_state=0)
        plm.triplet_stats(msa, Q, trip, weights=w, counts=True)


def main():
    args = sys.argv[1:]
    reps = int(args[0]) if args else 10
    seconds = float(args[1]) if len(args) > 1 else 120.0
    out = {}
    big = families(N, 300, seed=300)
    small = np.ascontiguousarray(big[:, :100])
    w = (1.0 / plm.reweight(big, 0.8)).astype(np.float32)
    print("N = %d, q = %d, N_eff = %.0f" % (N, Q, w.sum()), flush=True)
    per_triplet = {}
    for kind, weights in (("unit", None), ("reweight", w)):
        st = timed(lambda: plm.triplet_scan(small, Q, weights=weights, skip_state=0), reps)
        per_triplet[kind] = st["median_ms"] / n_triplets(100)
        show("scan L=100 %s (%d triplets):" % (kind, n_triplets(100)), st,
             "  %.2f us per triplet, HBM bound %.2f ms, ratio %.0f" % (1e3 * per_triplet[kind], bound_ms(100),
                                                                      st["median_ms"] / bound_ms(100)))
        out["scan_L100_" + kind] = dict(time=st, hbm_bound_ms=bound_ms(100))
    for kind, weights in (("unit", None), ("reweight", w)):
        est_s = per_triplet[kind] * n_triplets(300) / 1e3
        n_calls = int(max(1, min(reps, seconds // est_s)))
        st = timed(lambda: plm.triplet_scan(big, Q, weights=weights, skip_state=0), n_calls, warm=False)
        show("scan L=300 %s (%d triplets):" % (kind, n_triplets(300)), st,
             "  HBM bound %.1f ms, ratio %.0f (no warm-up call of its own; estimate was %.1f s)"
             % (bound_ms(300), st["median_ms"] / bound_ms(300), est_s))
        out["scan_L300_" + kind] = dict(time=st, hbm_bound_ms=bound_ms(300))
    rng = np.random.default_rng(1)
    trip = np.sort(np.array([rng.choice(300, 3, replace=False) for _ in range(1000)]), axis=1).astype(np.int32)
    for kind, weights in (("unit", None), ("reweight", w)):
        st = timed(lambda: plm.triplet_stats(big, Q, trip, weights=weights, counts=True), reps)
        show("listed T=1000 L=300 %s:" % kind, st)
        out["listed_" + kind] = dict(time=st)
    # contention: all lanes of a wave on one cell / mostly on one cell / spread
    const = np.full((N, 100), 7, np.int8)
    rng = np.random.default_rng(2)
    skew = np.where(rng.random((N, 100)) < 0.9, np.int8(3), rng.integers(0, Q, size=(N, 100), dtype=np.int8)).astype(np.int8)
    flat = rng.integers(0, Q, size=(N, 100), dtype=np.int8)
    for name, msa in (("constant columns", const), ("90 % one state", skew), ("uniform random", flat)):
        for kind, weights in (("unit", None), ("ones", np.ones(N, np.float32))):
            st = timed(lambda: plm.triplet_scan(msa, Q, weights=weights), max(1, reps // 3))
            show("contention, scan L=100, %s, %s:" % (name, kind), st)
            out["contention_%s_%s" % (name.split()[0], kind)] = dict(time=st)
    if len(args) > 2:
        with open(args[2], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    one() if "--one" in sys.argv else main()
