"""plm_pca_fit / plm_pca_project on the GPU against the numpy twin (tests/pca_twin.py).

Bounds (D = the number of kept features, lambda_1 the twin's largest eigenvalue):
  eigenvalues   |lambda_c - twin| <= residual_c + D 2^-52 lambda_1: a Ritz value lies within its residual norm of an
                eigenvalue; the second term covers the twin's dense eigh.
  eigenvectors  planted clusters, k = 2, gaps (lambda_c - lambda_{c+1}) / lambda_1 >= 1e-3 asserted from the twin:
                |sin angle| <= 2 residual_c / (lambda_c - lambda_{c+1}) + D 2^-52 (Davis-Kahan).
  invariants    eps = D 2^-50 (the rounding bound of a D-term float64 sum with a factor 4 of slack): components
                orthonormal within eps, weighted mean of the scores within eps sqrt(lambda_1) of 0, weighted variance of
                scores[:, c] within eps lambda_1 of eigenvalues[c], sum of the eigenvalues at most the total variance
                (plus eps lambda_1: with k = D the two are the same number, summed in two orders).  The weighted sums over
                the sequences are taken in extended precision, so that they add no error of their own.
  projections   (L + L q) 2^-52 max|v| absolute: L gathered terms plus the L q terms of the mean.
Every fit must converge (tol 1e-10, at most 500 iterations).

One combination is kept out of the matrix and has a test of its own: L = 1 with the 0.8-reweighting.  There a cluster is
the set of rows with the same state, so every state that occurs gets the total weight 1 up to the float32 rounding of
1 / size: C = diag(f) - f f^T with all f equal has ONE eigenvalue of multiplicity (states - 1), and the rounding spreads
it over a cluster of relative width 1e-8.  A block of k + 8 columns narrower than that cluster cannot resolve single
eigenvectors inside it to 1e-10 (the convergence factor is 1 - 1e-8), and no vector of the cluster's span has a residual
above its width: test_a_cluster_of_eigenvalues_wider_than_the_block states what the call returns then."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pca_twin as twin  # noqa: E402
from test_gpu_triplets import _msa as skewed  # noqa: E402

from evcouplings_amd import _lib, plm  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = ["unit", "reweight", "zero", "ones"]
U52 = 2.0 ** -52


def planted(N, L, q, seed):
    """4 random centres, each row a centre with 30 % of its entries redrawn."""
    rng = np.random.default_rng(seed)
    centres = rng.integers(0, q, size=(4, L))
    rows = centres[rng.integers(0, 4, size=N)]
    redo = rng.random(rows.shape) < 0.3
    rows[redo] = rng.integers(0, q, size=int(redo.sum()))
    return rows.astype(np.int8)


def _weights(kind, msa):
    N = len(msa)
    if kind == "unit":
        return None
    if kind == "ones":
        return np.ones(N, np.float32)
    same = np.stack([(msa[s][None, :] == msa).sum(axis=1) for s in range(N)])
    w = (1.0 / (same >= np.ceil(0.8 * msa.shape[1] - 1e-9)).sum(axis=1)).astype(np.float32)      # 1 / cluster size at 0.8
    if kind == "zero":
        w[N // 2] = 0.0
    return w


def _dim(L, q, skip):
    return L * (q - 1 if skip is not None else q)


def _long_moments(t, wq):
    w = np.asarray(wq).astype(np.longdouble)[:, None]
    t = np.asarray(t).astype(np.longdouble)
    return ((w * t).sum(axis=0) / w.sum()).astype(np.float64), ((w * t * t).sum(axis=0) / w.sum()).astype(np.float64)


def _check_fit(msa, q, k, w, skip, got, want, what):
    """Eigenvalues against the twin, the invariants, and scores == plm_pca_project of the same rows.  Every figure is
    printed, every miss collected; one assertion at the end."""
    N, L = msa.shape
    D = _dim(L, q, skip)
    lam1 = max(float(want["eigenvalues"][0]), 0.0)
    eps = D * 2.0 ** -50
    bad = []

    def need(ok, *info):
        if not ok:
            bad.append(info)

    need(got["converged"] and got["status"] == "converged" and 1 <= got["iterations"] <= 500, "converged", got["iterations"])
    need(got["total"] == want["total"], "total")
    need(np.array_equal(got["mean"], want["mean"]), "mean")
    need(abs(got["total_variance"] - want["total_variance"]) <= D * U52, "total_variance")
    for key in ("components", "eigenvalues", "residuals", "scores", "explained"):
        need(np.isfinite(got[key]).all(), "finite", key)
    err = np.abs(got["eigenvalues"] - want["eigenvalues"])
    bound = got["residuals"] + D * U52 * lam1
    need((err <= bound).all(), "eigenvalues", err, bound)
    need((np.diff(got["eigenvalues"]) <= 0).all(), "descending")
    need((got["residuals"] <= 1e-10 * max(got["eigenvalues"][0], 0.0)).all(), "residuals", got["residuals"])
    comp = got["components"].reshape(k, -1)
    orth = np.abs(comp @ comp.T - np.eye(k)).max()
    need(orth <= eps, "orthonormal", orth, eps)
    if skip is not None:
        need((got["components"][:, :, skip] == 0).all(), "zeros at the skipped state")
    for c in range(k):
        need(comp[c][int(np.argmax(np.abs(comp[c])))] > 0, "sign", c)
    mean, var = _long_moments(got["scores"], want["wq"])
    need(np.abs(mean).max() <= eps * np.sqrt(lam1), "mean of the scores", mean, eps * np.sqrt(lam1))
    need(np.abs(var - got["eigenvalues"]).max() <= eps * lam1, "variance of the scores", var - got["eigenvalues"], eps * lam1)
    need(got["eigenvalues"].sum() <= got["total_variance"] + eps * lam1, "sum of the eigenvalues")
    again = plm.pca_project(msa, q, got["mean"], got["components"], skip_state=skip)
    need(again.tobytes() == got["scores"].tobytes(), "scores against plm_pca_project")
    print("%s: %d iterations; eigenvalue errors %s (bounds %s); orthonormal %.3g, mean %.3g, variance %.3g (eps %.3g, lambda %.3g)%s"
          % (what, got["iterations"], err, bound, orth, np.abs(mean).max(), np.abs(var - got["eigenvalues"]).max(), eps, lam1,
             "  MISSED: %s" % bad if bad else ""))
    assert not bad, (what, bad)


def _matrix():
    """A subset of N x L x q that meets every value of each, cycling through the weight kinds, skip states and k."""
    cases, n = [], 0
    for N in (1, 5, 63, 64, 65, 257, 1000):
        for L in (1, 3, 4, 37):
            for q in (2, 3, 21, 26, 32):
                n += 1
                if n % 4 != 1 and not (N == 1000 and L == 37 and q == 21):
                    continue
                kind = KINDS[(n // 4) % 4]
                if kind == "zero" and N == 1:
                    kind = "ones"
                if L == 1 and kind in ("reweight", "zero"):          # see the module docstring
                    kind = "ones" if kind == "reweight" else "unit"
                skip = 0 if (n // 4) % 2 else None
                k = min((1, 2, 4)[(n // 4) % 3], _dim(L, q, skip))
                cases.append((N, L, q, kind, skip, k))
    return cases


MATRIX = _matrix()


@pytest.mark.parametrize("gen", [skewed, planted], ids=["skewed", "planted"])
def test_shape_matrix(gen):
    seen = {"N": set(), "L": set(), "q": set(), "kind": set(), "skip": set(), "k": set()}
    missed = []
    for N, L, q, kind, skip, k in MATRIX:
        msa = gen(N, L, q, seed=1000 * q + 10 * N + L)
        w = _weights(kind, msa)
        want = twin.fit(msa, q, k, w, skip)
        got = plm.pca_fit(msa, q, k=k, weights=w, skip_state=skip, scores=True)
        try:
            _check_fit(msa, q, k, w, skip, got, want, "%s N=%d L=%d q=%d %s skip=%s k=%d" % (gen.__name__, N, L, q, kind, skip, k))
        except AssertionError as miss:
            missed.append(miss.args[0])
        for key, v in zip(("N", "L", "q", "kind", "skip", "k"), (N, L, q, kind, skip, k)):
            seen[key].add(v)
    assert not missed, missed
    assert seen["N"] == {1, 5, 63, 64, 65, 257, 1000} and seen["L"] == {1, 3, 4, 37} and seen["q"] == {2, 3, 21, 26, 32}
    assert seen["kind"] == set(KINDS) and seen["skip"] == {None, 0} and seen["k"] == {1, 2, 4}


def _gapped(N, L, q, w_kind):
    """The first seed whose planted alignment has both compared gaps >= 1e-3 in the twin: (msa, weights, twin fit)."""
    for seed in range(50):
        msa = planted(N, L, q, seed)
        w = _weights(w_kind, msa)
        want = twin.fit(msa, q, 2, w)
        gaps = -np.diff(want["spectrum"][:3]) / want["spectrum"][0]
        if (gaps >= 1e-3).all():
            return msa, w, want, gaps
    raise AssertionError("no seed below 50 gives gaps of 1e-3")


@pytest.mark.parametrize("N,L,q,kind", [(65, 37, 21, "unit"), (257, 37, 3, "reweight"), (1000, 37, 21, "zero"),
                                        (65, 4, 26, "ones"), (1000, 4, 26, "unit")])
def test_eigenvectors_of_planted_clusters(N, L, q, kind):
    msa, w, want, gaps = _gapped(N, L, q, kind)
    assert (gaps >= 1e-3).all()
    D = L * q
    got = plm.pca_fit(msa, q, k=2, weights=w, scores=True)
    _check_fit(msa, q, 2, w, None, got, want, "planted N=%d L=%d q=%d %s" % (N, L, q, kind))
    for c in range(2):
        sin = twin.sin_angle(got["components"][c], want["components"][c])
        bound = 2 * got["residuals"][c] / (gaps[c] * want["spectrum"][0]) + D * U52
        print("component %d: |sin| %.3g, bound %.3g (gap %.3g)" % (c + 1, sin, bound, gaps[c]))
        assert sin <= bound, (c, sin, bound)


@pytest.mark.parametrize("skip", [None, 0])
def test_a_block_wider_than_the_rank(skip):
    """N = 5, L = 3, q = 2: rank C <= 3 < b.  k = 2 as it is used, and k = D, where components lie beyond the rank."""
    msa = skewed(5, 3, 2, seed=77)
    D = _dim(3, 2, skip)
    for k in (2, D):
        want = twin.fit(msa, 2, k, None, skip)
        got = plm.pca_fit(msa, 2, k=k, skip_state=skip, scores=True)
        _check_fit(msa, 2, k, None, skip, got, want, "N=5 L=3 q=2 skip=%s k=%d" % (skip, k))
        beyond = want["eigenvalues"] <= D * U52 * want["total_variance"]
        assert k < D or beyond.any()
        assert (got["eigenvalues"][beyond] <= D * U52 * got["total_variance"]).all() and (got["residuals"][beyond] == 0).all()


@pytest.mark.parametrize("L,q,k,skip", [(3, 2, 2, None), (4, 21, 4, 0), (1, 2, 2, None)])
def test_a_single_sequence_has_no_variance(L, q, k, skip):
    msa = skewed(1, L, q, seed=5)
    got = plm.pca_fit(msa, q, k=k, skip_state=skip, scores=True)
    D = _dim(L, q, skip)
    assert (got["eigenvalues"] <= D * U52 * got["total_variance"]).all() and (got["residuals"] == 0).all()
    assert got["total_variance"] == 0.0 and got["converged"]
    _check_fit(msa, q, k, None, skip, got, twin.fit(msa, q, k, None, skip), "N=1 L=%d q=%d" % (L, q))


@pytest.mark.parametrize("kind", ["unit", "reweight"])
def test_a_conserved_alignment(kind):
    msa = np.tile(np.array([[2, 0, 1, 2, 2]], np.int8), (70, 1))
    w = None if kind == "unit" else np.linspace(0.1, 1.0, 70).astype(np.float32)
    for skip in (None, 2):
        got = plm.pca_fit(msa, 3, k=3, weights=w, skip_state=skip, scores=True)
        assert (got["eigenvalues"] == 0).all() and (got["residuals"] == 0).all() and got["total_variance"] == 0.0
        assert got["converged"] and (got["scores"] == 0).all() and (got["explained"] == 0).all()
        comp = got["components"].reshape(3, -1)
        assert np.isfinite(comp).all() and np.abs(comp @ comp.T - np.eye(3)).max() <= 15 * 2.0 ** -50


@pytest.mark.parametrize("skip", [None, 0])
def test_projection_of_another_set(skip):
    N, L, q, k = 257, 37, 21, 4
    msa = planted(N, L, q, seed=3)
    got = plm.pca_fit(msa, q, k=k, weights=_weights("reweight", msa), skip_state=skip)
    assert "scores" not in got
    other = np.concatenate([skewed(1000, L, q, seed=9), planted(65, L, q, seed=4)])
    t = plm.pca_project(other, q, got["mean"], got["components"], skip_state=skip)
    want = twin.project(other, q, got["mean"], got["components"], skip)
    bound = (L + L * q) * U52 * np.abs(got["components"]).max()
    assert t.shape == (1065, k) and np.abs(t - want).max() <= bound, (np.abs(t - want).max(), bound)
    one = plm.pca_project(other[:1], q, got["mean"], got["components"][:1], skip_state=skip)
    assert one.tobytes() == t[:1, :1].tobytes()
    # a component that is not zero at the skipped state: the state still contributes 0
    if skip is not None:
        comp = got["components"].copy()
        comp[:, :, skip] = 0.25
        assert plm.pca_project(other, q, got["mean"], comp, skip_state=skip).tobytes() == t.tobytes()


ARRAYS = ("mean", "components", "eigenvalues", "residuals", "scores", "explained")
PLANS = [None, "g1", "g2", "g3", "g4", "g9", "s1", "s7", "s64", "s100000", "r1", "r2", "r5", "r1000", "g2,s64,r3", "r7,g4,s5"]


@pytest.mark.parametrize("N,L,q,kind,skip", [(1000, 37, 21, "reweight", None), (65, 4, 32, "ones", 0)])
def test_the_plan_changes_no_output_bit(monkeypatch, N, L, q, kind, skip):
    """g2 .. g9 put several workgroups on one site (N = 1000 has four slices of 256 sequences); s64 leaves the last
    sequence of N = 65 alone in the second workgroup of the Phi V kernel, s1 gives every sequence its own; r changes how
    many 32-row chunks a workgroup of the b x b products and of the rotation takes."""
    msa = planted(N, L, q, seed=11)
    w = _weights(kind, msa)
    other = skewed(129, L, q, seed=12)
    runs = []
    for plan in PLANS:
        if plan is None:
            monkeypatch.delenv("PLM_PCA_PLAN", raising=False)
        else:
            monkeypatch.setenv("PLM_PCA_PLAN", plan)
        r = plm.pca_fit(msa, q, k=2, weights=w, skip_state=skip, scores=True, seed=5)
        r["projected"] = plm.pca_project(other, q, r["mean"], r["components"], skip_state=skip)
        runs.append(r)
    monkeypatch.delenv("PLM_PCA_PLAN", raising=False)
    _check_fit(msa, q, 2, w, skip, {k: v for k, v in runs[0].items() if k != "projected"}, twin.fit(msa, q, 2, w, skip),
               "plan sweep N=%d" % N)
    for plan, r in zip(PLANS[1:], runs[1:]):
        for key in ARRAYS + ("projected",):
            assert r[key].tobytes() == runs[0][key].tobytes(), (plan, key)
        assert (r["iterations"], r["converged"], r["total"], r["total_variance"]) == \
            (runs[0]["iterations"], runs[0]["converged"], runs[0]["total"], runs[0]["total_variance"]), plan


def test_seeds():
    N, L, q = 257, 37, 21
    msa = planted(N, L, q, seed=21)
    want = twin.fit(msa, q, 2)
    a = plm.pca_fit(msa, q, k=2, scores=True, seed=1)
    b = plm.pca_fit(msa, q, k=2, scores=True, seed=1)
    c = plm.pca_fit(msa, q, k=2, scores=True, seed=2)
    for key in ARRAYS:
        assert a[key].tobytes() == b[key].tobytes(), key
    assert a["iterations"] == b["iterations"]
    assert any(a[key].tobytes() != c[key].tobytes() for key in ARRAYS)
    _check_fit(msa, q, 2, None, None, a, want, "seed 1")
    _check_fit(msa, q, 2, None, None, c, want, "seed 2")


def test_running_out_of_iterations_is_a_result():
    msa = skewed(257, 37, 21, seed=31)
    got = plm.pca_fit(msa, 21, k=2, max_iter=3, scores=True)
    assert not got["converged"] and got["status"] == "maxiter" and got["iterations"] == 3
    assert np.isfinite(got["components"]).all() and (got["residuals"] > 1e-10 * got["eigenvalues"][0]).any()
    comp = got["components"].reshape(2, -1)
    assert np.abs(comp @ comp.T - np.eye(2)).max() <= 777 * 2.0 ** -50
    want = twin.fit(msa, 21, 2)
    nearest = np.abs(got["eigenvalues"][:, None] - want["spectrum"][None, :]).min(axis=1)      # of any eigenvalue: not yet sorted out
    assert (nearest <= got["residuals"] + 777 * U52 * want["eigenvalues"][0]).all()


def test_a_cluster_of_eigenvalues_wider_than_the_block():
    """N = 257, L = 1, q = 32, reweighted: 31 equal eigenvalues up to 1e-8 (module docstring) and a block of 9 columns.
    The call runs out of iterations and says so; what it returns is still right: orthonormal vectors of the cluster's
    span, each Rayleigh quotient within its residual of an eigenvalue, residuals no larger than the cluster is wide.
    With a block that holds the whole cluster (oversample 30) the same alignment converges at once."""
    msa = skewed(257, 1, 32, seed=1000 * 32 + 10 * 257 + 1)
    w = _weights("reweight", msa)
    want = twin.fit(msa, 32, 1, w, 0)
    live = want["spectrum"][want["spectrum"] > (1 - 1e-6) * want["spectrum"][0]]       # the cluster at the top
    width = live[0] - live[-1]
    assert len(live) > 9 and 0 < width                                  # the premise, from the twin alone
    got = plm.pca_fit(msa, 32, k=1, weights=w, skip_state=0, max_iter=40, scores=True)
    print("cluster of %d eigenvalues, width %.3g; residual %.3g after %d iterations" % (len(live), width, got["residuals"][0],
                                                                                    got["iterations"]))
    assert got["status"] in ("maxiter", "converged") and got["converged"] == (got["status"] == "converged")
    assert got["residuals"][0] <= width + 31 * U52 * live[0]
    assert np.abs(got["eigenvalues"][0] - want["spectrum"]).min() <= got["residuals"][0] + 31 * U52 * live[0]
    assert abs(np.linalg.norm(got["components"][0]) - 1.0) <= 31 * 2.0 ** -50
    wide = plm.pca_fit(msa, 32, k=1, weights=w, skip_state=0, oversample=30, scores=True)
    _check_fit(msa, 32, 1, w, 0, wide, want, "the whole cluster in the block")
    assert wide["iterations"] <= 4


def _free_bytes():
    lib = _lib.load()                     # the HIP runtime is among its dependencies
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert lib.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_the_callback_reports_and_cancels():
    msa = planted(257, 37, 21, seed=41)
    seen = []
    whole = plm.pca_fit(msa, 21, k=2, scores=True, callback=lambda it, worst: seen.append((it, worst)))
    plain = plm.pca_fit(msa, 21, k=2, scores=True)
    assert whole["status"] == "converged" and [s[0] for s in seen] == list(range(1, whole["iterations"]))
    assert seen[0][1] == float("inf") and seen[-1][1] < 1e-8
    for key in ARRAYS:
        assert whole[key].tobytes() == plain[key].tobytes(), key
    stop = plm.pca_fit(msa, 21, k=2, scores=True, callback=lambda it, worst: it == 2)
    assert stop["status"] == "interrupted" and stop["iterations"] == 2 and not stop["converged"]
    same = plm.pca_fit(msa, 21, k=2, scores=True, max_iter=2)
    for key in ARRAYS:
        assert stop[key].tobytes() == same[key].tobytes(), key          # the vectors reached at the cancellation
    with pytest.raises(ZeroDivisionError):
        plm.pca_fit(msa, 21, k=2, callback=lambda it, worst: 1 // 0)
    # no device memory is left behind.  The runtime reports free memory in granules of 2 MB and may take one for itself
    # at any call; a cancelled call at this shape holds 1.9 MB of slice sums alone, so sixteen leaking calls would take
    # 30 MB: the bound of two granules tells the two apart
    big = planted(1000, 37, 32, seed=42)
    plm.pca_fit(big, 32, k=2, callback=lambda it, worst: True)
    before = _free_bytes()
    for _ in range(16):
        assert plm.pca_fit(big, 32, k=2, callback=lambda it, worst: True)["status"] == "interrupted"
    lost = before - _free_bytes()
    print("free device memory fell by %d bytes over 16 cancelled calls" % lost)
    assert lost <= 2 * 2097152
