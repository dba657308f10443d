#!/usr/bin/env python3
"""Cost of the inter-protein energies (plm.cross_energies; DESIGN_NEXT_ROWS.md section 9.23) at L_A = L_B = 150, q = 21:
  (a) one group, 10 000 x 10 000, best-partner arrays only;
  (b) the same shape with the matrix (800 MB of float64 come back to the host);
  (c) 5 000 groups of 1..10 rows per side, matrix and best arrays.
A call uploads the inter block and the sequences, runs and downloads; host clock around the whole (synchronous) call, one
warm-up, then the best of REPS calls.  Two baselines in the same process:
  twin    the numpy twin tests/cross_twin.py on the host, at TWIN_ROWS x TWIN_ROWS rows (shapes a, b) or on the first
          TWIN_GROUPS groups (shape c), scaled to the shape by the number of pairs;
  H       plm.hamiltonians on the expanded concatenated rows at HAM_ROWS x HAM_ROWS pairs, where the expansion fits, with
          and without the time numpy takes to build the rows; plm.cross_energies at the same rows next to it.  H_J of the
          whole row holds the intra blocks too; getting E from it takes two more calls on the two sides, not timed.
Kernel times come from a separate run under a profiler's kernel trace around `--one` (each shape once after a warm-up).

    python tests/probes/cross_energy_probe.py [REPS] [OUT.json]
    python tests/probes/cross_energy_probe.py --one
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import cross_twin as tw  # noqa: E402
from evcouplings_amd import plm  # noqa: E402

LA = LB = 150
Q = 21
N_BIG = 10000
N_GROUPS = 5000
TWIN_ROWS = 1000
TWIN_GROUPS = 250
HAM_ROWS = 1000


def best_of(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, 1e3 * min(ts)


def once(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, 1e3 * (time.perf_counter() - t0)


def inputs():
    rng = np.random.default_rng(923)
    L = LA + LB
    jij = rng.normal(scale=0.05, size=(L * (L - 1) // 2, Q, Q)).astype(np.float32)
    jab = plm.inter_blocks(jij, L, Q, np.arange(LA), np.arange(LA, L), gauge=None)
    a = rng.integers(0, Q, (N_BIG, LA)).astype(np.int8)
    b = rng.integers(0, Q, (N_BIG, LB)).astype(np.int8)
    na, nb = rng.integers(1, 11, N_GROUPS), rng.integers(1, 11, N_GROUPS)
    ao, bo = np.concatenate([[0], np.cumsum(na)]), np.concatenate([[0], np.cumsum(nb)])
    ga = rng.integers(0, Q, (int(ao[-1]), LA)).astype(np.int8)
    gb = rng.integers(0, Q, (int(bo[-1]), LB)).astype(np.int8)
    return jij, jab, a, b, ga, gb, ao, bo


def one():
    _, jab, a, b, ga, gb, ao, bo = inputs()
    for _ in range(2):
        plm.cross_energies(jab, a, b, matrix=False)
        plm.cross_energies(jab, a, b)
        plm.cross_energies(jab, ga, gb, ao, bo)


def main():
    args = sys.argv[1:]
    reps = int(args[0]) if args else 3
    jij, jab, a, b, ga, gb, ao, bo = inputs()
    out = {}
    pairs_big = float(N_BIG) * N_BIG
    pairs_groups = float((np.diff(ao) * np.diff(bo)).sum())
    # the twin, once each
    _, twin_big = once(lambda: tw.cross_energies(jab, a[:TWIN_ROWS], b[:TWIN_ROWS]))
    _, twin_grp = once(lambda: tw.cross_energies(jab, ga[:ao[TWIN_GROUPS]], gb[:bo[TWIN_GROUPS]], ao[:TWIN_GROUPS + 1],
                                                 bo[:TWIN_GROUPS + 1]))
    twin_big_scaled = twin_big * pairs_big / (float(TWIN_ROWS) ** 2)
    twin_grp_scaled = twin_grp * N_GROUPS / TWIN_GROUPS
    _, ta = best_of(lambda: plm.cross_energies(jab, a, b, matrix=False), reps)
    _, tb = best_of(lambda: plm.cross_energies(jab, a, b), reps)
    _, tc = best_of(lambda: plm.cross_energies(jab, ga, gb, ao, bo), reps)
    for name, t, pairs, twin in (("a", ta, pairs_big, twin_big_scaled), ("b", tb, pairs_big, twin_big_scaled),
                                 ("c", tc, pairs_groups, twin_grp_scaled)):
        print("(%s) %.1f ms for %.3g pairs: %.2f Gpairs/s, %.2f T site-terms/s; twin (scaled) %.0f ms, twin / GPU %.0f"
              % (name, t, pairs, pairs / t / 1e6, pairs * LA / t / 1e9, twin, twin / t), flush=True)
        out[name] = dict(ms=t, pairs=pairs, twin_scaled_ms=twin, ratio_twin=twin / t)
    # plm.hamiltonians on the expanded rows
    n = HAM_ROWS
    h0 = np.zeros((LA + LB, Q), np.float32)
    expand = lambda: np.concatenate([np.repeat(a[:n], n, axis=0), np.tile(b[:n], (n, 1))], axis=1)
    rows, t_expand = once(expand)
    _, t_ham = best_of(lambda: plm.hamiltonians(rows, Q, h0, jij), reps)
    _, t_cross = best_of(lambda: plm.cross_energies(jab, a[:n], b[:n]), reps)
    _, t_cross_best = best_of(lambda: plm.cross_energies(jab, a[:n], b[:n], matrix=False), reps)
    print("%d x %d pairs: plm.hamiltonians on expanded rows %.1f ms (+ %.1f ms to build the rows); plm.cross_energies %.1f ms "
          "with the matrix, %.1f ms best arrays only: H / cross %.1f (%.1f with the expansion)"
          % (n, n, t_ham, t_expand, t_cross, t_cross_best, t_ham / t_cross, (t_ham + t_expand) / t_cross), flush=True)
    print("shape (a) at the H rate per pair: %.0f ms against %.1f ms: %.0f x"
          % (t_ham * pairs_big / n / n, ta, t_ham * pairs_big / n / n / ta), flush=True)
    out["hamiltonians"] = dict(rows=n, ham_ms=t_ham, expand_ms=t_expand, cross_ms=t_cross, cross_best_ms=t_cross_best,
                               shape_a_at_ham_rate_ms=t_ham * pairs_big / n / n)
    if len(args) > 1:
        with open(args[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    one() if "--one" in sys.argv else main()
