"""Bit-exact record of a fixed list of small fits, for refactors of the L-BFGS iteration and its two callers,
plm_ctx_optimize and plm_ar_fit: every column of every iteration table plus n_evals, status, status_msg and the final
objective; for the autoregressive fits (cases ar_*) also ls_reason, nll, the norms and the bytes of the fitted model.  A fit
is bitwise reproducible on one device (DESIGN_NEXT_ROWS.md section 9.7), so two builds that decide alike write equal files.

    python tests/probes/trajectory_dump.py dump OUT.npz [CASE ...]     (PLM_HIP_LIB selects another build)
    python tests/probes/trajectory_dump.py compare A.npz B.npz         (exit status 1 when anything differs)

The wall-clock column of the tables is kept under its own keys (*/secs) and left out of the comparison.  With PLM_DEBUG=1
the library's line-search / pair reports on stderr follow a "=== case" line each, which shows the paths a case took.
"""
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.dirname(TESTS), TESTS]      # the package, and tests/ar_twin.py

Q = 21


def _fit(N, L, seed, **kw):
    def run(plm, synthetic_msa):
        msa, _ = synthetic_msa(N, L, seed=seed)
        return [plm.fit(msa, q=Q, want_fij=False, **kw)]
    return run


def _resumed(N, L, seed, first, then):
    """a max_iter stop, then a second call on the same context (which still holds f and g of the point reached)"""
    def run(plm, synthetic_msa):
        msa, _ = synthetic_msa(N, L, seed=seed)
        with plm.PlmContext(msa, Q, max_iter=first, epsilon=1e-6) as ctx:
            ctx.reweight()
            ctx.marginals(pairs=False)
            ctx.set_x(None)
            a = ctx.optimize()
            ctx.set_options(max_iter=then)
            return [a, ctx.optimize()]
    return run


AR_LAM, AR_EPS = 0.01, 1e-4      # LAM and FIT_EPS of tests/test_gpu_ar.py


def _ar(L, q, n, restart=False, **kw):
    """one plm.ar_fit on the data of _fit_data(L, q, n) of tests/test_gpu_ar.py; restart: from the converged point"""
    def run(plm, synthetic_msa):
        import ar_twin
        h, J = ar_twin.random_model(L, q, sd_j=0.4)
        x = plm.ar_sample(h, J, q, n, seed=5)
        w = np.random.default_rng(300 + L).uniform(0.2, 1.0, n).astype(np.float32)
        opts = dict(dict(max_iter=2000, epsilon=AR_EPS), **kw)
        if restart:
            first = plm.ar_fit(x, w, q, AR_LAM, AR_LAM, **opts)
            opts["start"] = (first["hi"], first["jij"])
        table = []
        r = plm.ar_fit(x, w, q, AR_LAM, AR_LAM, callback=lambda *a: table.append(a) and False, **opts)
        status = [k for k, v in plm.AR_STATUS.items() if v == r["status"]][0]
        return [dict(r, table=table, n_evals=r["evaluations"], status=status, status_msg=r["status"])]
    return run


AR_KEYS = [("iterations", np.int64), ("ls_reason", np.int64), ("nll", np.float64), ("gnorm", np.float64),
           ("xnorm", np.float64), ("hi", np.float32), ("jij", np.float32)]
CASES = [
    ("joint", _fit(2000, 48, 12, lambda_h=0.01, max_iter=30, epsilon=1e-12, joint=True)),
    ("vp", _fit(800, 32, 5, max_iter=0, epsilon=1e-3)),
    ("precond", _fit(800, 32, 5, max_iter=0, epsilon=1e-3, precond=True)),
    ("precond_joint", _fit(800, 32, 5, max_iter=60, epsilon=1e-3, precond=True, joint=True)),
    ("gaps", _fit(800, 32, 5, max_iter=0, epsilon=1e-3, ignore_gaps=True)),
    ("m3", _fit(800, 32, 5, max_iter=80, epsilon=1e-6, lbfgs_m=3)),
    ("m20", _fit(800, 32, 5, max_iter=80, epsilon=1e-6, lbfgs_m=20)),
    ("m20_joint", _fit(800, 32, 5, max_iter=80, epsilon=1e-6, lbfgs_m=20, joint=True)),
    ("resumed", _resumed(800, 32, 5, 7, 12)),
    ("tight", _fit(600, 24, 31, max_iter=3000, epsilon=1e-12)),
    ("tight_joint", _fit(600, 24, 31, max_iter=3000, epsilon=1e-12, joint=True)),
    ("accurate_switch", _fit(6000, 120, 77, max_iter=0, epsilon=1e-3)),
    ("deep", _fit(300000, 64, 300064, max_iter=3000, epsilon=1e-3)),
    ("ar_6", _ar(6, 4, 200)),
    ("ar_12", _ar(12, 21, 300)),
    ("ar_24", _ar(24, 5, 1000)),
    ("ar_6_maxiter", _ar(6, 4, 200, max_iter=3)),
    ("ar_6_restart", _ar(6, 4, 200, restart=True)),
    ("ar_6_tight", _ar(6, 4, 200, max_iter=400, epsilon=1e-12)),
]


def dump(path, names):
    from evcouplings_amd import plm
    from evcouplings_amd.synthetic import synthetic_msa
    out = {}
    for name, run in CASES:
        if names and name not in names:
            continue
        print("=== case %s" % name, file=sys.stderr, flush=True)
        for i, r in enumerate(run(plm, synthetic_msa)):
            key = "%s/%d" % (name, i)
            table = np.array(r["table"], np.float64).reshape(-1, 7)
            out[key + "/table"] = np.delete(table, 1, axis=1)       # iter, cond, fx, nll, |h|, |e|
            out[key + "/secs"] = table[:, 1]
            out[key + "/n_evals"] = np.int64(r["n_evals"])
            out[key + "/status"] = np.int64(r["status"])
            out[key + "/status_msg"] = np.array(r["status_msg"])
            out[key + "/fx"] = np.float64(r["fx"])
            if name.startswith("ar_"):
                for field, dtype in AR_KEYS:
                    out["%s/%s" % (key, field)] = np.asarray(r[field], dtype)
            print("%-18s %4d iterations %5d evaluations  status %d  %s" % (
                key, len(table), r["n_evals"], r["status"], r["status_msg"]), flush=True)
    np.savez(path, **out)


def compare(a, b):
    A, B = np.load(a), np.load(b)
    keys = sorted(k for k in set(A.files) | set(B.files) if not k.endswith("/secs"))
    bad = 0
    for k in keys:
        if k not in A.files or k not in B.files:
            same = False
        elif A[k].dtype.kind == "U":
            same = A[k].shape == B[k].shape and bool((A[k] == B[k]).all())
        else:
            same = A[k].shape == B[k].shape and A[k].tobytes() == B[k].tobytes()
        if not same:
            bad += 1
            print("DIFFERENT: %s" % k)
    print("%d of %d entries differ" % (bad, len(keys)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3:])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
