"""Timings of the autoregressive Potts model (DESIGN_NEXT_ROWS.md section 9.19) at L = 300, q = 21:

    python tests/probes/ar_probe.py [--n 50000] [--chains 65536] [--fit-n 5000] [--budget 120] [--no-fit] [--out FILE.json]

  * one plm_ar_eval at N sequences, plm_ar_logprob at N sequences, plm_ar_sample of C chains: host clock around the call,
    which ends in a device synchronise; the median of three after one warm-up call.  The times include the upload of
    the model and the sequences and the download of the result (the one-shot calls own their buffers).
  * a whole fit to epsilon 1e-4 on fit-n samples of a planted model (lambda_h = lambda_j = 0.01), with its iteration count,
    and one attempt at epsilon 1e-5 from that fit's end point; either stops when it has run for `budget` seconds.
Needs a gfx950 device; there is no fall-back."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ar_twin as tw  # noqa: E402
from evcouplings_amd import plm  # noqa: E402


def timed(fn, reps=3):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts))}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=300)
    ap.add_argument("--q", type=int, default=21)
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--fit-n", type=int, default=5000)
    ap.add_argument("--budget", type=float, default=120.0)
    ap.add_argument("--no-fit", action="store_true", help="the three one-shot calls only (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    L, q = a.L, a.q
    h, J = tw.random_model(L, q)
    out = {"L": L, "q": q, "n": a.n, "chains": a.chains, "fit_n": a.fit_n}
    out["sample"] = timed(lambda: plm.ar_sample(h, J, q, a.chains, seed=1))
    for form in ("tiled", "direct"):
        os.environ["PLM_AR_FORM"] = form
        out["sample_" + form] = timed(lambda: plm.ar_sample(h, J, q, a.chains, seed=1), reps=1)
    del os.environ["PLM_AR_FORM"]
    x = plm.ar_sample(h, J, q, a.n, seed=2)
    w = np.random.default_rng(1).uniform(0.2, 1.0, a.n).astype(np.float32)
    out["logprob"] = timed(lambda: plm.ar_logprob(x, q, h, J))
    out["eval"] = timed(lambda: plm.ar_evaluate(x, w, q, 0.01, 0.01, h, J))
    print(json.dumps(out), flush=True)

    xf, wf = x[:a.fit_n], w[:a.fit_n]
    for eps, start in () if a.no_fit else ((1e-4, None), (1e-5, "previous")):
        t0 = time.perf_counter()
        conds = []

        def cb(it, secs, cond, *rest):
            conds.append(cond)
            return time.perf_counter() - t0 > a.budget

        res = plm.ar_fit(xf, wf, q, 0.01, 0.01, max_iter=5000, epsilon=eps, callback=cb,
                         start=None if start is None else (prev["hi"], prev["jij"]))
        secs = time.perf_counter() - t0
        prev = res
        out["fit_eps_%g" % eps] = {"status": res["status"], "iterations": res["iterations"], "evaluations": res["evaluations"],
                                   "ls_reason": res["ls_reason"], "seconds": secs, "fx": res["fx"],
                                   "cond": res["gnorm"] / max(1.0, res["xnorm"]), "best_cond": min(conds) if conds else None}
        print(json.dumps({k: out[k] for k in out if k.startswith("fit")}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
