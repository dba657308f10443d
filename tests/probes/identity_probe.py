#!/usr/bin/env python3
"""Cost of the pairwise identities (plm.cross_identities, plm.redundancy_filter; DESIGN_NEXT_ROWS.md section 9.11),
q = 21.  A call builds the device images on the host, uploads, runs and downloads; host clock around the whole call,
one warm-up, then REPS calls (median, min, max).
  cross:    A = 65 536 x B = 50 000 rows at L = 300 and L = 100 (A: planted descendants of B's families);
  yardstick: plm.reweight on the same 50 000 x L alignment in the same run -- the same compare at the same row
            length, half the pairs by symmetry and early exits the cross kernel cannot all use; the ratio is per
            pair-site (cross: n_a n_b L, reweight: n_b^2 L counted in full, as a user sees it);
  bound:    3 VALU ops per 4 sites per lane, 256 CUs x 4 SIMDs x 16 lanes per cycle at CLOCK_GHZ;
  filter:   plm.redundancy_filter at N = 50 000, L = 300, threshold 0.9, with the rows kept.

    python tests/probes/identity_probe.py [REPS] [OUT.json]
    python tests/probes/identity_probe.py --one        one cross call (L = 300) and one filter call after a warm-up of
                                                       each, for a profiler run around it
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
CLOCK_GHZ = 2.4      # peak engine clock of the MI355X
LANES = 256 * 4 * 16


def families(n, L, n_families, seed, rates=(0.02, 0.1, 0.25, 0.5)):
    """n rows: descendants of n_families random ancestors at the given per-site mutation rates."""
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, Q, size=(n_families, L), dtype=np.int8)
    rows = anc[rng.integers(0, n_families, size=n)]
    rate = np.asarray(rates)[rng.integers(0, len(rates), size=n)]
    mut = rng.random((n, L)) < rate[:, None]
    rows[mut] = rng.integers(0, Q, size=int(mut.sum()), dtype=np.int8)
    return rows


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, dict(median_ms=1e3 * float(np.median(ts)), min_ms=1e3 * min(ts), max_ms=1e3 * max(ts), reps=len(ts))


def show(name, st, extra=""):
    print("%s %.1f ms (min %.1f, max %.1f, %d reps)%s" % (name, st["median_ms"], st["min_ms"], st["max_ms"], st["reps"],
                                                         extra), flush=True)


def one():
    b, a = families(50000, 300, 2500, seed=300), families(65536, 300, 2500, seed=300)
    msa = families(50000, 300, 2500, seed=7)
    for _ in range(2):
        plm.cross_identities(a, b, threshold=0.8)
        plm.redundancy_filter(msa, 0.9)


def main():
    args = sys.argv[1:]
    reps = int(args[0]) if args else 10
    n_a, n_b, n_f = 65536, 50000, 50000
    out = {}
    for L in (300, 100):
        b = families(n_b, L, n_b // 20, seed=L)
        a = families(n_a, L, n_b // 20, seed=L)       # the same ancestors (same seed, same first draw)
        r, cross = timed(lambda: plm.cross_identities(a, b, threshold=0.8), reps)
        _, rew = timed(lambda: plm.reweight(b, 0.8), reps)
        pair_sites, rew_sites = float(n_a) * n_b * L, float(n_b) * n_b * L
        bound_ms = 1e3 * pair_sites * 0.75 / (LANES * CLOCK_GHZ * 1e9)
        ratio = (cross["median_ms"] / pair_sites) / (rew["median_ms"] / rew_sites)
        show("L=%d cross %d x %d:" % (L, n_a, n_b), cross,
             "  %.2f Tsites/s, VALU bound %.1f ms; nearest identity mean %.3f, within 0.8: mean %.1f"
             % (pair_sites / cross["median_ms"] / 1e9, bound_ms, r["identity"].mean(), r["n_within"].mean()))
        show("L=%d reweight %d:" % (L, n_b), rew, "  cross / reweight per pair-site %.2f" % ratio)
        out["L%d" % L] = dict(cross=cross, reweight=rew, ratio_per_pair_site=ratio, valu_bound_ms=bound_ms)
    msa = families(n_f, 300, n_f // 20, seed=7)
    keep, filt = timed(lambda: plm.redundancy_filter(msa, 0.9), max(1, reps // 2))
    show("filter N=%d L=300 theta=0.9:" % n_f, filt, "  kept %d" % int(keep.sum()))
    out["filter"] = dict(time=filt, kept=int(keep.sum()), n=n_f)
    if len(args) > 1:
        with open(args[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    one() if "--one" in sys.argv else main()
