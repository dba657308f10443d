#!/usr/bin/env python3
"""Speed of the Gibbs sampler (DESIGN_NEXT_ROWS.md section 9.6) at (L, C) = (300, 65 536), (100, 65 536), (600, 16 384),
q = 21.  A plm.sample call uploads the model, expands it, sweeps and downloads; the time of a sweep is the difference of
two calls with burn_in = B_LONG and burn_in = B_SHORT (host clock, same start), divided by the sweeps between them: one
warm-up pair, then REPS pairs (median, min, max).  Beside it, as the yardstick, one plm.potentials call on the same
C x L sequences (the same C L (L - 1) q gathered adds, done in parallel by the forward GEMM; host clock, transfers in).
PLM_SAMPLE_FORM=direct in the environment measures the other form of the sweep.

    python tests/probes/sample_probe.py [REPS] [OUT.json]      the table
    python tests/probes/sample_probe.py --one L C SWEEPS       one call of each kind, for a profiler run around it
    python tests/probes/sample_probe.py --fit                  fit synthetic_msa(20 000, 100), sample 20 000 sequences
                                                               from the fit, compare frequencies (an illustration)
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
B_SHORT, B_LONG = 2, 10


def model(L, q=Q, seed=0):
    rng = np.random.default_rng(seed + L)
    h = rng.normal(size=(L, q)).astype(np.float32)
    J = rng.normal(scale=0.05, size=(L * (L - 1) // 2, q, q)).astype(np.float32)
    return h, J


def stats(ts):
    return dict(median_ms=1e3 * float(np.median(ts)), min_ms=1e3 * min(ts), max_ms=1e3 * max(ts), reps=len(ts))


def call(h, J, C, burn_in, x0):
    t0 = time.perf_counter()
    plm.sample(h, J, Q, C, burn_in=burn_in, seed=1, start=x0, energies=False)
    return time.perf_counter() - t0


def table(reps, out_path):
    rows = {}
    for L, C in ((300, 65536), (100, 65536), (600, 16384)):
        h, J = model(L)
        x0 = np.random.default_rng(1).integers(0, Q, size=(C, L)).astype(np.int8)
        call(h, J, C, B_SHORT, x0), call(h, J, C, B_LONG, x0)           # warm-up
        sweep, short = [], []
        for _ in range(reps):
            a, b = call(h, J, C, B_SHORT, x0), call(h, J, C, B_LONG, x0)
            short.append(a)
            sweep.append((b - a) / (B_LONG - B_SHORT))
        plm.potentials(x0[:256], Q, h, J)                                # warm-up of the forward path
        pot = []
        for _ in range(3):
            t0 = time.perf_counter()
            plm.potentials(x0, Q, h, J)
            pot.append(time.perf_counter() - t0)
        r = dict(sweep=stats(sweep), call_with_2_sweeps=stats(short), potentials_call=stats(pot))
        ms = r["sweep"]["median_ms"]
        r["sweeps_per_s"] = 1e3 / ms
        r["chain_sweeps_per_s"] = C * 1e3 / ms
        r["gathered_adds_per_s"] = C * L * (L - 1.0) * Q * 1e3 / ms
        r["sweep_over_potentials"] = ms / r["potentials_call"]["median_ms"]
        rows["L%d_C%d" % (L, C)] = r
        print("L=%d C=%d  sweep %.2f ms (min %.2f, max %.2f, %d reps) = %.1f sweeps/s, %.3g chain-sweeps/s, %.3g adds/s; "
              "call with %d sweeps %.0f ms; potentials call %.0f ms (min %.0f, max %.0f); sweep / potentials = %.3f"
              % (L, C, ms, r["sweep"]["min_ms"], r["sweep"]["max_ms"], reps, r["sweeps_per_s"], r["chain_sweeps_per_s"],
                 r["gathered_adds_per_s"], B_SHORT, r["call_with_2_sweeps"]["median_ms"], r["potentials_call"]["median_ms"],
                 r["potentials_call"]["min_ms"], r["potentials_call"]["max_ms"], r["sweep_over_potentials"]), flush=True)
        del h, J, x0
    if out_path:
        with open(out_path, "w") as f:
            json.dump(dict(form=os.environ.get("PLM_SAMPLE_FORM", "tiled"), rows=rows), f, indent=1)


def one(L, C, sweeps):
    h, J = model(L)
    x0 = np.random.default_rng(1).integers(0, Q, size=(C, L)).astype(np.int8)
    print("sample call with %d sweeps: %.3f s" % (sweeps, call(h, J, C, sweeps, x0)))
    t0 = time.perf_counter()
    plm.potentials(x0, Q, h, J)
    print("potentials call: %.3f s" % (time.perf_counter() - t0))


def fit_and_sample():
    from evcouplings_amd.synthetic import synthetic_msa
    N, L = 20000, 100
    msa, planted = synthetic_msa(N, L, seed=7)
    res = plm.fit(msa, Q, max_iter=100)
    w = res["weights"] / res["weights"].sum()
    t0 = time.perf_counter()
    out, _ = plm.sample(res["hi"], res["jij"], Q, N, burn_in=200, seed=1, energies=False)
    secs = time.perf_counter() - t0
    x = out[0]
    onehot = lambda m: (m[:, :, None] == np.arange(Q)[None, None, :])            # noqa: E731
    fi_a = (onehot(msa) * w[:, None, None]).sum(axis=0)
    fi_s = onehot(x).mean(axis=0)
    print("sampled %d sequences (200 sweeps) in %.2f s; single-site frequencies, correlation %.4f"
          % (N, secs, np.corrcoef(fi_a.ravel(), fi_s.ravel())[0, 1]))
    pairs = [tuple(p[:2]) for p in list(planted)[:20]]
    ca, cs = [], []
    for i, j in pairs:
        fa = np.einsum("n,na,nb->ab", w, onehot(msa)[:, i], onehot(msa)[:, j]) - np.outer(fi_a[i], fi_a[j])
        fs = np.einsum("na,nb->ab", onehot(x)[:, i], onehot(x)[:, j]) / N - np.outer(fi_s[i], fi_s[j])
        ca.append(fa.ravel())
        cs.append(fs.ravel())
    print("connected pair frequencies of %d planted pairs, correlation %.4f"
          % (len(pairs), np.corrcoef(np.concatenate(ca), np.concatenate(cs))[0, 1]))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--fit":
        fit_and_sample()
    else:
        table(int(sys.argv[1]) if len(sys.argv) > 1 else 10, sys.argv[2] if len(sys.argv) > 2 else None)
