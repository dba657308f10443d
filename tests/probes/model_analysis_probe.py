#!/usr/bin/env python3
"""Wall time of the three CouplingsModel analysis calls (DESIGN_NEXT_ROWS.md section 9.5) at L = 300 and L = 600, q = 21:
plm.model_pair_scores, plm.double_mutant_matrix, plm.independent_fields.  Each time is a host clock around one call,
which uploads, runs the kernel, downloads and synchronises the stream; one warm-up call per shape, then REPS repeats
(median, min, max).  Usage: python tests/probes/model_analysis_probe.py [REPS] [OUT.json]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from evcouplings_amd import plm  # noqa: E402


def dense(blocks, L):
    q = blocks.shape[-1]
    iu, ju = np.triu_indices(L, 1)
    out = np.zeros((L, L, q, q))
    out[iu, ju] = blocks
    out[ju, iu] = blocks.transpose(0, 2, 1)
    return out


def timed(fn, reps):
    fn()                                    # warm-up: code object load, first allocations of this shape
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return dict(median_ms=1e3 * float(np.median(ts)), min_ms=1e3 * min(ts), max_ms=1e3 * max(ts), reps=reps)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    rows = {}
    for L in (300, 600):
        q = 21
        rng = np.random.default_rng(L)
        n = L * (L - 1) // 2
        J = dense(rng.normal(size=(n, q, q)), L)
        Fb = rng.random(size=(n, q, q))
        F = dense(Fb / Fb.sum(axis=(1, 2), keepdims=True), L)
        fi = rng.random(size=(L, q))
        fi /= fi.sum(axis=1, keepdims=True)
        smm, target = rng.normal(size=(L, q)), rng.integers(0, q, size=L).astype(np.int8)
        rows[L] = {
            "model_pair_scores": timed(lambda: plm.model_pair_scores(J, F, fi), reps),
            "double_mutant_matrix": timed(lambda: plm.double_mutant_matrix(J, smm, target), reps),
            "independent_fields": timed(lambda: plm.independent_fields(fi, 0.01, 0.2 * 50000), reps),
        }
        for name, r in rows[L].items():
            print("L=%d %-22s median %8.2f ms  (min %.2f, max %.2f, %d reps)" % (L, name, r["median_ms"], r["min_ms"],
                                                                              r["max_ms"], r["reps"]), flush=True)
        del J, F
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
