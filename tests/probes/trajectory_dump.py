"""Bit-exact record of a fixed list of small fits, for refactors of plm_ctx_optimize: every column of every iteration
table plus n_evals, status, status_msg and the final objective.  A fit is bitwise reproducible on one device
(DESIGN_NEXT_ROWS.md section 9.7), so two builds that decide alike write equal files.

    python tests/probes/trajectory_dump.py dump OUT.npz [CASE ...]     (PLM_HIP_LIB selects another build)
    python tests/probes/trajectory_dump.py compare A.npz B.npz         (exit status 1 when anything differs)

The wall-clock column of the tables is kept under its own keys (*/secs) and left out of the comparison.  With PLM_DEBUG=1
the library's line-search / pair reports on stderr follow a "=== case" line each, which shows the paths a case took.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

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
