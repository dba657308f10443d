#!/usr/bin/env python3
"""Cost of the residue distance maps (plm.residue_distances, plm.aggregate_distance_maps; DESIGN_NEXT_ROWS.md section
9.18).  A call validates on the host, uploads, runs and downloads: host clock around the whole call, one warm-up, then
REPS calls (median, min, max) -- the time with the transfers.  The time without them is the kernel time of a profiler
run around `--one` (rocprofv3 --kernel-trace --stats).
  one chain:  1000 residues x 8 atoms, the symmetric call;
  aggregate:  32 chains of 300 residues x 8 atoms, every chain with itself, one residue numbering (300 x 300 result);
  context:    the vectorised numpy twin (tests/distance_twin.py) on the same inputs, once each, results compared bit
              for bit.  The twin is context, not a target: numpy runs it on one core.

    python tests/probes/distance_probe.py [REPS] [OUT.json]
    python tests/probes/distance_probe.py --one        two calls of each entry point, for a profiler run around it
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import distance_twin as twin  # noqa: E402
from evcouplings_amd import plm  # noqa: E402

ATOMS = 8


def chain(n, seed):
    """a random walk of n residue centres 3.8 apart, ATOMS atoms around each, three decimals"""
    rng = np.random.default_rng(seed)
    step = rng.normal(size=(n, 3))
    centres = np.cumsum(3.8 * step / np.linalg.norm(step, axis=1, keepdims=True), axis=0)
    xyz = np.round(np.repeat(centres, ATOMS, axis=0) + rng.normal(scale=1.2, size=(n * ATOMS, 3)), 3)
    first = ATOMS * np.arange(n)
    return xyz, np.stack((first, first + ATOMS - 1)).T.astype(np.int32)


def many_chains(n_chains, n):
    parts = [chain(n, 100 + c) for c in range(n_chains)]
    coords = np.concatenate([p[0] for p in parts])
    ranges = np.concatenate([p[1] + c * n * ATOMS for c, p in enumerate(parts)]).astype(np.int32)
    off = (n * np.arange(n_chains + 1)).astype(np.int32)
    slots = np.tile(np.arange(n, dtype=np.int32), n_chains)
    maps = np.stack((np.arange(n_chains), np.arange(n_chains))).T.astype(np.int32)
    return coords, ranges, off, slots, maps, n


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, dict(median_ms=1e3 * float(np.median(ts)), min_ms=1e3 * min(ts), max_ms=1e3 * max(ts), reps=len(ts))


def show(name, st, extra=""):
    print("%s %.2f ms (min %.2f, max %.2f, %d reps)%s" % (name, st["median_ms"], st["min_ms"], st["max_ms"], st["reps"],
                                                         extra), flush=True)


def one():
    xyz, ranges = chain(1000, 1)
    args = many_chains(32, 300)
    for _ in range(2):
        plm.residue_distances(xyz, ranges)
        plm.aggregate_distance_maps(*args)


def main():
    args = sys.argv[1:]
    reps = int(args[0]) if args else 20
    out = {}
    xyz, ranges = chain(1000, 1)
    got, st = timed(lambda: plm.residue_distances(xyz, ranges), reps)
    t0 = time.perf_counter()
    want = twin.residue_distances(xyz, ranges)
    twin_ms = 1e3 * (time.perf_counter() - t0)
    pairs = 0.5 * (1000 * ATOMS) ** 2
    show("one chain, 1000 x %d atoms, symmetric:" % ATOMS, st, "  %.1f G atom pairs/s; numpy twin %.0f ms; same bits: %s"
         % (pairs / st["median_ms"] / 1e6, twin_ms, np.array_equal(got, want)))
    out["one_chain"] = dict(time=st, twin_ms=twin_ms, same_bits=bool(np.array_equal(got, want)))
    many = many_chains(32, 300)
    (agg, count), st = timed(lambda: plm.aggregate_distance_maps(*many), reps)
    t0 = time.perf_counter()
    want_agg, want_count = twin.aggregate_distance_maps(*many)
    twin_ms = 1e3 * (time.perf_counter() - t0)
    same = bool(np.array_equal(agg, want_agg) and np.array_equal(count, want_count))
    pairs = 32 * 0.5 * (300 * ATOMS) ** 2
    show("aggregate, 32 chains of 300 x %d atoms:" % ATOMS, st, "  %.1f G atom pairs/s; numpy twin %.0f ms; same bits: %s"
         % (pairs / st["median_ms"] / 1e6, twin_ms, same))
    out["aggregate"] = dict(time=st, twin_ms=twin_ms, same_bits=same)
    if len(args) > 1:
        with open(args[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    one() if "--one" in sys.argv else main()
