"""plm_triplet_stats / plm_triplet_scan on the GPU against the numpy twin (tests/triplet_twin.py): counts and totals
equal as integers, freq within 1 ulp, connected within 4e-15 (fewer than 16 roundings of quantities of magnitude <= 2:
16 * 2 * 2^-53 = 3.6e-15), norm2 within q^3 2^-52 relative + 1e-28 (summation order of q^3 non-negative terms).

Which launch a case takes (csrc/plm_triplets.hip, `plan_of` below):
  listed call   k_trip_count<u32> ("count32") while W < 2^32 -- every unweighted call, and weighted ones of a handful
                of sequences --, k_trip_count<u64> in one pass ("count64") for W >= 2^32 and q <= 25, in c-range passes
                ("count64-cpass", q >= 26: 64-bit cells of q^3 pass the 128 KB of a histogram); k_trip_close follows.
                The sequence split (more than one workgroup per triplet) starts above 4096 sequences or under the knob.
  scan          the fused k_trip_scan<u32> / <u64> ("scan32" / "scan64") where the listed call takes one pass, else the
                kernels of the listed call over chunks of the table ("scan-unfused").
PLM_TRIPLET_PLAN forces each of these; test_the_plan_changes_no_output_* sweep it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import triplet_twin as twin  # noqa: E402

from evcouplings_amd import correlations, plm  # noqa: E402
from evcouplings_amd.synthetic import msa_to_a2m  # noqa: E402

pytestmark = pytest.mark.gpu

ALPHABETS = [2, 3, 21, 25, 26, 32]          # 25 | 26: the last alphabet whose 64-bit histogram takes one pass, the first that does not
SIZES = [1, 63, 64, 65, 257, 1000]
LENGTHS = [3, 4, 37]
KINDS = ["unit", "reweight", "zero", "ones"]
C_ATOL = 4e-15


def plan_of(q, W, scan=False):
    if W < 2 ** 32:
        return "scan32" if scan else "count32"
    if q <= 25:
        return "scan64" if scan else "count64"
    return "scan-unfused" if scan else "count64-cpass"


def _msa(N, L, q, seed):
    """Skewed states (a dominant one per column) with repeated rows, so that clusters and contention both occur."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, q, size=(max(1, N // 3 + 1), L))
    base[rng.random(base.shape) < 0.4] = int(rng.integers(0, q))
    rows = base[rng.integers(0, len(base), size=N)]
    flip = rng.random(rows.shape) < 0.15
    rows[flip] = rng.integers(0, q, size=int(flip.sum()))
    return rows.astype(np.int8)


_WEIGHTS = {}


def _weights(kind, msa, key):
    """unit: None; reweight: 1 / cluster size at 0.8 (computed once per alignment); zero: the same with one weight exactly
    0; ones: [1] * N (W = N 2^30)."""
    N = len(msa)
    if kind == "unit":
        return None
    if kind == "ones":
        return np.ones(N, np.float32)
    if key not in _WEIGHTS:
        _WEIGHTS[key] = (1.0 / plm.reweight(msa, 0.8)).astype(np.float32)
    w = _WEIGHTS[key].copy()
    if kind == "zero":
        w[N // 2] = 0.0
    return w


def _triplets(L):
    t = [(0, 1, 2), (L - 3, L - 2, L - 1), (0, 1, L - 1), (0, 1, 2)]       # the first one listed twice
    if L > 30:
        t.append((5, 17, 30))
    return np.array(t, np.int32)


def _assert_listed(got, want, what):
    assert got["total"] == want["total"], what
    assert got["counts"].dtype == np.uint64
    np.testing.assert_array_equal(got["counts"].astype(np.int64), want["counts"], err_msg=what + ": counts")    # < 2^63
    err = np.abs(got["freq"] - want["freq"])
    assert (err <= np.spacing(want["freq"])).all(), "%s: freq off by %g" % (what, err.max())
    np.testing.assert_allclose(got["connected"], want["connected"], rtol=0, atol=C_ATOL, err_msg=what + ": connected")


def _cases(q):
    for N in SIZES:
        for L in LENGTHS:
            for kind in KINDS:
                if kind == "zero" and N == 1:
                    continue                    # the only weight zero: W = 0, refused (test_triplet_host.py)
                yield N, L, kind


@pytest.mark.parametrize("q", ALPHABETS)
def test_listed_shape_matrix(q):
    """Every alphabet with every N, L and weight kind: counts, total, freq and connected against the twin."""
    for N, L, kind in _cases(q):
        msa = _msa(N, L, q, seed=1000 * q + 10 * N + L)
        w = _weights(kind, msa, (q, N, L))
        trip = _triplets(L)
        want = twin.triplet_stats(msa, q, trip, w)
        got = plm.triplet_stats(msa, q, trip, weights=w, counts=True)
        _assert_listed(got, want, "q=%d N=%d L=%d %s (%s)" % (q, N, L, kind, plan_of(q, want["total"])))
        np.testing.assert_array_equal(got["counts"][0], got["counts"][3])          # the repeated triplet


def test_the_matrix_meets_every_plan_with_every_weight_kind():
    seen = set()
    for q in ALPHABETS:
        for N, L, kind in _cases(q):
            if kind == "unit":
                W = N
            elif kind == "ones":
                W = N * 2 ** 30
            else:
                W = twin.quantise(_weights(kind, _msa(N, L, q, seed=1000 * q + 10 * N + L), (q, N, L)), N)[1]
            seen.add((plan_of(q, W), kind))
    assert {(p, k) for p, k in seen if k == "unit"} == {("count32", "unit")}        # N < 2^32: always narrow
    for kind in ("reweight", "zero", "ones"):
        for plan in ("count64", "count64-cpass"):
            assert (plan, kind) in seen, (plan, kind)
    assert ("count32", "reweight") in seen and ("count32", "ones") in seen          # N = 1: W = 2^30


def test_only_some_outputs_and_the_skip_state_leaves_them_alone():
    msa = _msa(65, 4, 21, seed=3)
    trip = _triplets(4)
    full = plm.triplet_stats(msa, 21, trip, counts=True)
    only_c = plm.triplet_stats(msa, 21, trip, counts=False, freq=False, connected=True, skip_state=0)
    assert sorted(only_c) == ["connected", "total", "triplets"]
    np.testing.assert_array_equal(only_c["connected"], full["connected"])
    only_n = plm.triplet_stats(msa, 21, trip, counts=True, freq=False, connected=False)
    assert sorted(only_n) == ["counts", "total", "triplets"]
    np.testing.assert_array_equal(only_n["counts"], full["counts"])


@pytest.mark.parametrize("kind", ["unit", "ones"])
def test_contention_conserved_columns(kind):
    """All 64 lanes of every wave on one counter (three constant columns), and on q of them (two constant columns)."""
    N, q = 1000, 21
    rng = np.random.default_rng(7)
    msa = np.empty((N, 4), np.int8)
    msa[:, 0], msa[:, 1], msa[:, 2] = 5, 20, 0
    msa[:, 3] = rng.integers(0, q, N)
    w = _weights(kind, msa, None)
    trip = np.array([(0, 1, 2), (0, 1, 3)], np.int32)
    want = twin.triplet_stats(msa, q, trip, w)
    got = plm.triplet_stats(msa, q, trip, weights=w, counts=True)
    _assert_listed(got, want, "conserved " + kind)
    assert int(got["counts"][0][5, 20, 0]) == want["total"] and int(got["counts"][0].sum()) == want["total"]
    assert (got["connected"][0] == 0).all()                # every frequency is 0 or 1: C = 1 - 3 + 2, exactly
    _, norm2, maxabs, _ = plm.triplet_scan(msa, q, weights=w, sites=[0, 1, 2])
    assert norm2[0] == 0 and maxabs[0] == 0


LISTED_PLANS = {"unit": [None, "w32", "w64", "n4", "n64,c5", "w64,n100,c1", "n1000,c32", "w64,c16"],
                "ones": [None, "w64", "n4", "n64,c5", "n100,c1", "n1000", "c16", "c25"]}


@pytest.mark.parametrize("kind,q", [("unit", 32), ("ones", 32), ("ones", 21), ("zero", 26)])
def test_the_plan_changes_no_output_of_the_listed_call(monkeypatch, kind, q):
    """Counter width, sequence split and c-range passes: every output identical bit for bit."""
    msa = _msa(1000, 4, q, seed=q)
    w = _weights(kind, msa, ("plans", q))
    trip = _triplets(4)
    monkeypatch.delenv("PLM_TRIPLET_PLAN", raising=False)
    ref = plm.triplet_stats(msa, q, trip, weights=w, counts=True)
    _assert_listed(ref, twin.triplet_stats(msa, q, trip, w), "default plan")
    for plan in LISTED_PLANS["unit" if kind == "unit" else "ones"][1:]:
        monkeypatch.setenv("PLM_TRIPLET_PLAN", plan)
        got = plm.triplet_stats(msa, q, trip, weights=w, counts=True)
        assert got["total"] == ref["total"]
        for key in ("counts", "freq", "connected"):
            assert got[key].tobytes() == ref[key].tobytes(), "PLM_TRIPLET_PLAN=%s: %s" % (plan, key)


@pytest.mark.parametrize("kind,q", [("unit", 21), ("reweight", 21), ("unit", 32), ("reweight", 32)])
def test_the_plan_changes_no_output_of_the_scan(monkeypatch, kind, q):
    """Fused and unfused, narrow and wide, any split of the k range: norm2, maxabs and argmax identical bit for bit."""
    msa = _msa(257, 6, q, seed=q + 1)
    w = _weights(kind, msa, ("scan-plans", q))
    monkeypatch.delenv("PLM_TRIPLET_PLAN", raising=False)
    ref = plm.triplet_scan(msa, q, weights=w, skip_state=0)
    plans = ["k1", "k2", "k4", "u", "u,n64,c7", "w64", "w64,k3", "w64,u,c4,n100"]
    for plan in plans:
        monkeypatch.setenv("PLM_TRIPLET_PLAN", plan)
        got = plm.triplet_scan(msa, q, weights=w, skip_state=0)
        for a, b, name in zip(got, ref, ("triplets", "norm2", "maxabs", "argmax")):
            assert a.tobytes() == b.tobytes(), "PLM_TRIPLET_PLAN=%s: %s" % (plan, name)


def _check_scan(msa, q, w, sites, skips, what, against_listed):
    got = {s: plm.triplet_scan(msa, q, weights=w, sites=sites, skip_state=s, with_total=True) for s in skips}
    flat = {s: (got[s][3].astype(np.int64) * [q * q, q, 1]).sum(axis=1) for s in skips}
    trip, want = twin.triplet_scan_multi(msa, q, w, sites, skips, probes=flat)
    for s in skips:
        t, norm2, maxabs, abc, total = got[s]
        name = "%s skip=%s (%s)" % (what, s, plan_of(q, total, scan=True))
        np.testing.assert_array_equal(t, trip, err_msg=name)
        w_norm2, w_maxabs, _, probed = want[s]
        np.testing.assert_allclose(maxabs, w_maxabs, rtol=0, atol=C_ATOL, err_msg=name + ": maxabs")
        np.testing.assert_allclose(norm2, w_norm2, rtol=q ** 3 * 2.0 ** -52, atol=1e-28, err_msg=name + ": norm2")
        assert (probed >= w_maxabs - 8e-15).all(), name + ": argmax"
        if s >= 0:
            assert (abc != s).all(), name + ": argmax names a skipped state"
        assert ((abc >= 0) & (abc < q)).all()
        if against_listed:
            C = plm.triplet_stats(msa, q, t, weights=w, freq=False)["connected"]
            keep = twin.admissible(q, s)
            np.testing.assert_allclose(maxabs, np.abs(C[:, keep]).max(axis=1), rtol=0, atol=C_ATOL, err_msg=name)
            np.testing.assert_allclose(norm2, (C[:, keep] ** 2).sum(axis=1), rtol=q ** 3 * 2.0 ** -52, atol=1e-28,
                                       err_msg=name)


@pytest.mark.parametrize("L,q,N", [(3, 2, 1), (4, 21, 65), (5, 32, 257)])
@pytest.mark.parametrize("kind", ["unit", "reweight"])
def test_scan_of_every_site(L, q, N, kind):
    msa = _msa(N, L, q, seed=L + q + N)
    _check_scan(msa, q, _weights(kind, msa, ("scan", L, q, N)), None, (-1, 0, q - 1), "L=%d q=%d N=%d %s" % (L, q, N, kind),
                against_listed=True)


@pytest.mark.parametrize("kind", ["unit", "reweight"])
def test_scan_of_many_triplets(kind):
    """L = 37: 7770 triplets, 630 (i, j) workgroups with k ranges of every length from 1 to 35."""
    msa = _msa(257, 37, 21, seed=37)
    _check_scan(msa, 21, _weights(kind, msa, ("scan", 37)), None, (0,), "L=37 " + kind, against_listed=False)


@pytest.mark.parametrize("sites", [[4, 20, 36], [0, 3, 4, 11, 19, 30, 36]])
def test_scan_of_a_selection(sites):
    msa = _msa(257, 37, 21, seed=37)
    for kind in ("unit", "reweight"):
        _check_scan(msa, 21, _weights(kind, msa, ("scan", 37)), sites, (-1, 0, 20), "sites=%s %s" % (sites, kind),
                    against_listed=True)


def test_frequencies_sum_to_the_marginals_of_the_fit_path():
    """Summing freq over c gives plm.marginals' f_ij, over b and c its f_i, within the 2e-6 test_gpu_parity.py holds
    plm.marginals to (float32 there; the new path is exact to about 2^-31 per weight)."""
    q, N, L = 21, 1000, 6
    msa = _msa(N, L, q, seed=11)
    w = _weights("reweight", msa, ("marg",))
    fi, fij = plm.marginals(msa, w, q)
    trip = plm.triplet_index(L)
    freq = plm.triplet_stats(msa, q, trip, weights=w, connected=False)["freq"]
    pair = {p: n for n, p in enumerate(zip(*np.triu_indices(L, 1)))}
    for t, (i, j, k) in enumerate(trip):
        np.testing.assert_allclose(freq[t].sum(axis=2), fij[pair[(i, j)]], rtol=0, atol=2e-6)
        np.testing.assert_allclose(freq[t].sum(axis=1), fij[pair[(i, k)]], rtol=0, atol=2e-6)
        np.testing.assert_allclose(freq[t].sum(axis=0), fij[pair[(j, k)]], rtol=0, atol=2e-6)
        np.testing.assert_allclose(freq[t].sum(axis=(1, 2)), fi[i], rtol=0, atol=2e-6)
        np.testing.assert_allclose(freq[t].sum(axis=(0, 1)), fi[k], rtol=0, atol=2e-6)


def _planted_model(L=12, q=4, seed=5):
    rng = np.random.default_rng(seed)
    hi = (0.3 * rng.normal(size=(L, q))).astype(np.float32)
    jij = np.zeros((L * (L - 1) // 2, q, q), np.float32)
    pairs = list(zip(*np.triu_indices(L, 1)))
    for i, j in ((0, 5), (5, 9), (2, 3), (3, 11)):
        jij[pairs.index((i, j))] = 1.5 * np.eye(q, dtype=np.float32)
    return hi, jij


def test_two_samples_of_one_model_end_to_end(tmp_path):
    """No statistical threshold: how closely two finite samples agree has not been measured and is not this test's
    business.  The numbers of the comparison equal the twin's on the same inputs."""
    L, q = 12, 4
    hi, jij = _planted_model(L, q)
    a = plm.sample(hi, jij, q, 4096, burn_in=20, seed=1, energies=False)[0][0]
    b = plm.sample(hi, jij, q, 4096, burn_in=20, seed=2, energies=False)[0][0]
    res = correlations.compare_statistics(a, b, q, n_top=50)
    for key in ("f_i", "c_ij", "c_ijk"):
        assert np.isfinite(res[key]).all(), key
    assert res["triplets"].shape == (50, 3) and (np.diff(res["scores"]) <= 0).all()
    trip, norm2, maxabs, _, _ = twin.triplet_scan(a, q)
    where = {tuple(t): n for n, t in enumerate(trip)}
    chosen = np.array([where[tuple(t)] for t in res["triplets"]])
    assert len(set(chosen)) == 50
    np.testing.assert_allclose(res["scores"], norm2[chosen], rtol=q ** 3 * 2.0 ** -52, atol=1e-28)
    rest = np.delete(norm2, chosen)
    assert res["scores"].min() >= rest.max() * (1 - 1e-12)                 # the 50 largest, whatever the order of near-ties
    ca = twin.triplet_stats(a, q, res["triplets"])["connected"]
    cb = twin.triplet_stats(b, q, res["triplets"])["connected"]
    np.testing.assert_allclose(res["natural_norm2"], (ca ** 2).sum(axis=(1, 2, 3)), rtol=1e-12, atol=1e-28)
    np.testing.assert_allclose(res["sample_maxabs"], np.abs(cb).max(axis=(1, 2, 3)), rtol=0, atol=C_ATOL)
    r, slope = correlations.pearson_and_slope(ca, cb)
    assert abs(res["c_ijk"][0] - r) <= 1e-9 and abs(res["c_ijk"][1] - slope) <= 1e-9
    assert res["total"] == (4096, 4096)
    # the command line, once, through files (the protein alphabet: q = 21, states 0..3 are "-ACD")
    nat, sam, out = (str(tmp_path / n) for n in ("nat.a2m", "sam.a2m", "out.csv"))
    msa_to_a2m(a[:512], nat)
    msa_to_a2m(b[:512], sam)
    assert correlations.main([nat, sam, "--top", "20", "-o", out]) == 0
    lines = open(out).read().splitlines()
    assert len(lines) == 21 and lines[0].startswith("i,j,k,score")
    scores = [float(x.split(",")[3]) for x in lines[1:]]
    assert scores == sorted(scores, reverse=True)
