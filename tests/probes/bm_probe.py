#!/usr/bin/env python3
"""Speed of the Boltzmann-machine refinement (plm_bm_fit, DESIGN_NEXT_ROWS.md section 9.7) at q = 21, C = 65 536 chains,
k = 5 sweeps per epoch, L = 300 and L = 100.  A plm.bm_fit call uploads, runs E epochs and downloads; the time of an epoch
is the difference of two calls with E_LONG and E_SHORT epochs (host clock, same start), divided by the epochs between
them.  Two columns: without a callback (nothing crosses to the host inside the loop) and with one (the host waits for the
trace row of every epoch).  The split of an epoch into kernels comes from a profiler run of its own.

    python tests/probes/bm_probe.py [REPS] [OUT.json]           the table
    python tests/probes/bm_probe.py --one L C K E               one call, for a profiler run around it
    python tests/probes/bm_probe.py --split L C K E OUTDIR      rocprofv3 --kernel-trace --stats around --one (a child
                                                                process), then milliseconds per epoch by group
"""
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from evcouplings_amd import plm  # noqa: E402

Q = 21
E_SHORT, E_LONG = 2, 6
GROUPS = (("sweeps", ("k_gibbs",)), ("counts", ("k_bm_transpose", "k_bm_count")),
          ("update_and_expansion", ("k_bm_stats", "k_bm_trace", "k_bm_update", "k_sample_expand")))


def problem(L, C, q=Q, seed=0):
    rng = np.random.default_rng(seed + L)
    h = rng.normal(size=(L, q)).astype(np.float32)
    J = rng.normal(scale=0.05, size=(L * (L - 1) // 2, q, q)).astype(np.float32)
    fi = rng.dirichlet(np.full(q, 0.3), size=L).astype(np.float32)       # a few frequent letters per site, as in a family
    iu, ju = np.triu_indices(L, 1)
    fij = np.empty((len(iu), q, q), np.float32)
    for s in range(0, len(iu), 4096):
        fij[s:s + 4096] = fi[iu[s:s + 4096], :, None] * fi[ju[s:s + 4096], None, :]
    x0 = np.stack([rng.choice(q, size=C, p=fi[i] / fi[i].sum()) for i in range(L)], axis=1).astype(np.int8)
    return h, J, fi, fij, x0


def call(pb, C, K, E, callback=None):
    h, J, fi, fij, x0 = pb
    t0 = time.perf_counter()
    plm.bm_fit(fi, fij, Q, h, J, C, E, sweeps_per_epoch=K, lr=0.05, seed=1, start=x0, callback=callback)
    return time.perf_counter() - t0


def table(reps, out_path, K=5, C=65536):
    rows = {}
    for L in (300, 100):
        pb = problem(L, C)
        r = {}
        for name, cb in (("no_callback", None), ("with_callback", lambda *a: False)):
            call(pb, C, K, E_SHORT, cb)                                  # warm-up
            ts = []
            for _ in range(reps):
                a, b = call(pb, C, K, E_SHORT, cb), call(pb, C, K, E_LONG, cb)
                ts.append(1e3 * (b - a) / (E_LONG - E_SHORT))
            r[name] = dict(median_ms=float(np.median(ts)), min_ms=min(ts), max_ms=max(ts), reps=reps)
        rows["L%d_C%d_k%d" % (L, C, K)] = r
        print("L=%d C=%d k=%d  epoch %.2f ms (min %.2f, max %.2f) without a callback, %.2f ms (min %.2f, max %.2f) with one; "
              "%d reps" % (L, C, K, r["no_callback"]["median_ms"], r["no_callback"]["min_ms"], r["no_callback"]["max_ms"],
                           r["with_callback"]["median_ms"], r["with_callback"]["min_ms"], r["with_callback"]["max_ms"], reps),
              flush=True)
        del pb
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


def split(L, C, K, E, outdir):
    os.makedirs(outdir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", outdir, "-o", "bm", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--one", str(L), str(C), str(K), str(E)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    sys.stdout.write(run.stdout[-2000:])
    if run.returncode != 0:
        sys.stderr.write(run.stderr[-4000:])
        return run.returncode
    wall = [float(l.split()[-2]) for l in run.stdout.splitlines() if l.startswith("bm_fit call")][0]
    files = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
    ms = {name: 0.0 for name, _ in GROUPS}
    ms["other"] = 0.0
    lines = []
    for r in csv.DictReader(open(files[0])):
        t = float(r["TotalDurationNs"]) / 1e6
        lines.append("  %-60s calls=%6s total=%10.3f ms" % (r["Name"][:60], r["Calls"], t))
        for name, keys in GROUPS:
            if any(k in r["Name"] for k in keys):
                ms[name] += t
                break
        else:
            ms["other"] += t
    kernels = sum(ms.values())                # --one makes the timed call only: every kernel in the trace is its own
    print("L=%d C=%d k=%d, %d epochs under the profiler: call %.1f ms; per epoch: sweeps %.3f ms (%.3f per sweep), counts "
          "%.3f ms, update and expansion %.3f ms, other kernels %.3f ms; call less kernels (code-object load, allocation, "
          "upload, download, host) %.1f ms"
          % (L, C, K, E, wall, ms["sweeps"] / E, ms["sweeps"] / E / K, ms["counts"] / E, ms["update_and_expansion"] / E,
             ms["other"] / E, wall - kernels))
    print("\n".join(lines))
    return 0


def one(L, C, K, E):
    pb = problem(L, C)
    print("bm_fit call with %d epochs: %.1f ms" % (E, 1e3 * call(pb, C, K, E)))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(*[int(v) for v in sys.argv[2:6]])
    elif len(sys.argv) > 1 and sys.argv[1] == "--split":
        sys.exit(split(*[int(v) for v in sys.argv[2:6]], sys.argv[6]))
    else:
        table(int(sys.argv[1]) if len(sys.argv) > 1 else 5, sys.argv[2] if len(sys.argv) > 2 else None)
