#!/usr/bin/env python3
"""Cost of the principal components of an alignment (plm.pca_fit, plm.pca_project; DESIGN_NEXT_ROWS.md section 9.20),
q = 21, N = 50 000, k = 2, oversample = 8 (a block of 10 columns).  A call validates and transposes the alignment on the
host, uploads, runs and downloads; host clock around the whole call, one warm-up call, then REPS calls (median, min, max).
  fit:        the whole fit at L = 300 with the weights 1 / cluster size, and at L = 100;
  iteration:  the fit cut at max_iter = 21 minus the fit cut at max_iter = 1 (both with a tolerance that is never met),
              over 20: one block product with its b x b sums, synchronisation, host eigenproblems and rotation;
  project:    plm.pca_project of 65 536 sequences on the two components;
  bytes:      what each kernel of one iteration has to move, and the time that takes at HBM_TBS, to be read beside a
              kernel trace of `--one` (rocprofv3 --kernel-trace --stats -- python tests/probes/pca_probe.py --one);
  dense:      the numpy route at L = 100 on the same box: one-hot matrix, weighted covariance (one float64 GEMM), eigh.

    python tests/probes/pca_probe.py [REPS] [OUT.json]
    python tests/probes/pca_probe.py --one      one fit at L = 300 and one projection after a warm-up
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from evcouplings_amd import plm  # noqa: E402

Q, N, K, OVER, N_PROJECT = 21, 50000, 2, 8, 65536
HBM_TBS = 8.0        # peak HBM bandwidth of the MI355X, TB/s: the rate DESIGN.md prices the field-solver passes at
SLICE, ROWS = 256, 32


def families(n, L, seed, n_families=6, rate=0.3):
    """Subfamilies of unequal size (proportions 1, 1/2, 1/3, ...) around random ancestors (the same for every seed)."""
    anc = np.random.default_rng(0).integers(0, Q, size=(n_families, L), dtype=np.int8)
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, n_families + 1)
    rows = anc[rng.choice(n_families, size=n, p=p / p.sum())]
    mut = rng.random((n, L)) < rate
    rows[mut] = rng.integers(0, Q, size=int(mut.sum()), dtype=np.int8)
    return rows


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1], "reps": reps}, out


def kernel_bytes(n, L, q, b):
    """Bytes one iteration's kernels must move (reads of what does not stay in LDS or registers, plus writes)."""
    df, ns, chunks = L * q, -(-n // SLICE), -(-L * q // ROWS)
    return {
        "k_pca_meanproj": 8 * (df * b + df + 2 * L * b),
        "k_pca_phiv": n * L + 8 * n * L * b + 8 * n * b,                 # the image, one gathered row of V per site, U
        "k_pca_slices": n * L + L * (4 * n + 8 * n * b) + 8 * L * ns * q * b,   # U and wq once per site, the slice sums
        "k_pca_combine": 8 * (L * ns * q * b + df * b),
        "k_pca_gram": 8 * (2 * df * b + 3 * chunks * b * b),
        "k_pca_rotate": 8 * (5 * df * b + chunks * b),
    }


def dense_route(msa, w):
    t0 = time.perf_counter()
    n, L = msa.shape
    onehot = np.zeros((n, L * Q))
    onehot[np.arange(n)[:, None], np.arange(L)[None, :] * Q + msa] = 1.0
    w = w.astype(np.float64) / w.sum()
    phi = onehot - (w[:, None] * onehot).sum(axis=0)[None]
    t1 = time.perf_counter()
    cov = (phi * w[:, None]).T @ phi
    t2 = time.perf_counter()
    lam = np.linalg.eigh(cov)[0][::-1]
    t3 = time.perf_counter()
    return {"onehot_s": t1 - t0, "covariance_s": t2 - t1, "eigh_s": t3 - t2, "total_s": t3 - t0}, lam


def main(argv):
    one = "--one" in argv
    argv = [a for a in argv if a != "--one"]
    reps = int(argv[0]) if argv else 5
    out_path = argv[1] if len(argv) > 1 else None
    msa = families(N, 300, seed=1)
    w = (1.0 / plm.reweight(msa, 0.8)).astype(np.float32)
    other = families(N_PROJECT, 300, seed=2)
    if one:
        plm.pca_fit(msa[:, :100], Q, k=K, weights=w)
        model = plm.pca_fit(msa, Q, k=K, weights=w)
        plm.pca_project(other, Q, model["mean"], model["components"])
        return 0
    res = {"N": N, "q": Q, "k": K, "oversample": OVER, "hbm_tbs": HBM_TBS}
    for L in (300, 100):
        sub = np.ascontiguousarray(msa[:, :L])
        fit, model = timed(lambda: plm.pca_fit(sub, Q, k=K, weights=w, oversample=OVER), reps)
        never = dict(k=K, weights=w, oversample=OVER, tol=1e-300)           # a tolerance no residual meets: max_iter decides
        cut1, _ = timed(lambda: plm.pca_fit(sub, Q, max_iter=1, **never), reps)
        cut21, c21 = timed(lambda: plm.pca_fit(sub, Q, max_iter=21, **never), reps)
        assert c21["iterations"] == 21
        proj, _ = timed(lambda: plm.pca_project(other[:, :L], Q, model["mean"], model["components"]), reps)
        bytes_ = kernel_bytes(N, L, Q, K + OVER)
        res["L%d" % L] = {
            "fit": fit, "iterations": model["iterations"], "converged": model["converged"],
            "eigenvalues": model["eigenvalues"].tolist(), "explained": model["explained"].tolist(),
            "residuals": model["residuals"].tolist(),
            "iteration_s": (cut21["median_s"] - cut1["median_s"]) / 20, "fit_max_iter_1": cut1, "fit_max_iter_21": cut21,
            "project_%d" % N_PROJECT: proj,
            "kernel_bytes": bytes_, "kernel_us_at_hbm": {k: v / (HBM_TBS * 1e12) * 1e6 for k, v in bytes_.items()},
        }
        print("L = %d: fit %.1f ms (%d iterations, converged %s), one iteration %.3f ms, projection of %d sequences %.1f ms"
              % (L, 1e3 * fit["median_s"], model["iterations"], model["converged"], 1e3 * res["L%d" % L]["iteration_s"],
                 N_PROJECT, 1e3 * proj["median_s"]))
        for name, nbytes in bytes_.items():
            print("    %-16s %8.2f MB  %8.2f us at %.0f TB/s" % (name, nbytes / 1e6, nbytes / (HBM_TBS * 1e12) * 1e6, HBM_TBS))
        if L == 100:
            dense, lam = dense_route(sub, w)
            res["dense_numpy_L100"] = dense
            res["dense_eigenvalue_gap"] = float(np.abs(lam[:K] - model["eigenvalues"]).max())
            print("    dense numpy route: one-hot %.2f s, covariance %.2f s, eigh %.2f s, total %.2f s; eigenvalues differ by %.2g"
                  % (dense["onehot_s"], dense["covariance_s"], dense["eigh_s"], dense["total_s"], res["dense_eigenvalue_gap"]))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main(sys.argv[1:]))
