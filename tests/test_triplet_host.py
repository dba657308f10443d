"""CPU-side checks of the three-site statistics: the numpy twin (tests/triplet_twin.py) against a literal triple loop
and against hand calculations, the weight quantisation, the triplet table, the argument checks of the library that run
before it looks for a device, and the command line of evcouplings_amd.correlations on twin outputs."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import triplet_twin as twin  # noqa: E402

from evcouplings_amd import _lib, correlations, plm  # noqa: E402

HAND = np.array([[0, 1, 2, 0],
                 [0, 1, 2, 1],
                 [1, 1, 0, 2],
                 [2, 0, 2, 0],
                 [0, 1, 2, 0],
                 [1, 2, 1, 1],
                 [2, 2, 2, 2]], dtype=np.int8)
HAND_W = np.array([1.0, 0.5, 0.25, 1.0, 0.0, 0.125, 0.75], dtype=np.float32)


def _loops(msa, q, trip, wq, W):
    """The definitions of include/plm_hip.h as literal Python loops over exact integers."""
    i, j, k = trip
    cnt = [[[0] * q for _ in range(q)] for _ in range(q)]
    for n, row in enumerate(msa):
        cnt[row[i]][row[j]][row[k]] += int(wq[n])
    r = range(q)
    cij = [[sum(cnt[a][b][c] for c in r) for b in r] for a in r]
    cik = [[sum(cnt[a][b][c] for b in r) for c in r] for a in r]
    cjk = [[sum(cnt[a][b][c] for a in r) for c in r] for b in r]
    ci = [sum(cij[a]) for a in r]
    cj = [sum(cij[a][b] for a in r) for b in r]
    ck = [sum(cik[a][c] for a in r) for c in r]
    C = np.zeros((q, q, q))
    for a in r:
        for b in r:
            for c in r:
                C[a, b, c] = (cnt[a][b][c] / W - cij[a][b] / W * (ck[c] / W) - cik[a][c] / W * (cj[b] / W)
                              - cjk[b][c] / W * (ci[a] / W) + 2 * (ci[a] / W) * (cj[b] / W) * (ck[c] / W))
    return np.array(cnt, dtype=np.int64), C


@pytest.mark.parametrize("weights", [None, HAND_W])
@pytest.mark.parametrize("trip", [(0, 1, 2), (1, 2, 3), (0, 1, 3), (0, 2, 3)])
def test_twin_equals_the_literal_loops_on_hand_written_rows(weights, trip):
    wq, W = twin.quantise(weights, len(HAND))
    cnt, C = _loops(HAND.tolist(), 3, trip, wq, W)
    got = twin.triplet_stats(HAND, 3, [trip], weights)
    np.testing.assert_array_equal(got["counts"][0], cnt)
    assert got["total"] == W and got["counts"].sum() == W
    np.testing.assert_allclose(got["connected"][0], C, rtol=0, atol=4e-15)
    np.testing.assert_array_equal(got["freq"][0], cnt / float(W))


def test_a_conserved_triplet_has_no_connected_correlation():
    msa = np.full((9, 3), 2, np.int8)
    r = twin.triplet_stats(msa, 4, [(0, 1, 2)])
    assert r["counts"][0][2, 2, 2] == 9 and r["counts"].sum() == 9
    assert (r["connected"] == 0).all()


@pytest.mark.parametrize("q", [2, 3, 4, 5])
def test_a_full_product_design_has_no_connected_correlation(q):
    msa = np.array(list(itertools.product(range(q), repeat=3)), dtype=np.int8)
    r = twin.triplet_stats(msa, q, [(0, 1, 2)])
    assert (r["counts"] == 1).all()
    if q in (2, 4):     # every frequency is a power of two, every product exact: C is 0 to the last bit
        assert (r["connected"] == 0).all()
    np.testing.assert_allclose(r["connected"], 0, rtol=0, atol=4e-15)      # else 1/q^3 - 3 (1/q^2)(1/q) + 2/q^3 rounds


def test_a_planted_xor_triplet_is_invisible_to_pairs_and_one_eighth_at_three_sites():
    msa = np.array([[0, 0, 0], [0, 1, 1], [1, 0, 1], [1, 1, 0]], dtype=np.int8)
    r = twin.triplet_stats(msa, 2, [(0, 1, 2)])
    cnt = r["counts"][0]
    for ax in (0, 1, 2):                       # every pair table is uniform: C_ij = 1/4 - 1/2 1/2 = 0
        assert (cnt.sum(axis=ax) == 1).all()
    want = np.array([[[1, -1], [-1, 1]], [[-1, 1], [1, -1]]]) / 8.0     # f_ijk - 3/8 + 2/8: +1/8 on the rows, -1/8 off them
    np.testing.assert_array_equal(r["connected"][0], want)
    norm2, maxabs, arg = twin.reductions(r["connected"][0])
    assert norm2 == 8 / 64 and maxabs == 0.125 and arg == 0
    assert twin.reductions(r["connected"][0], skip_state=0) == (1 / 64, 0.125, 7)


def test_quantisation_follows_the_stated_rule():
    wq, W = twin.quantise(np.ones(5, np.float32), 5)
    assert (wq == 2 ** 30).all() and W == 5 * 2 ** 30 and W >= 2 ** 32      # five rows reach the 64-bit counters
    wq, W = twin.quantise(None, 7)
    assert (wq == 1).all() and W == 7
    wq, W = twin.quantise(np.array([0.5, 0.25, 0.0], np.float32), 3)        # max 2^e <= 2^30 with e <= 30: e = 30
    assert list(wq) == [2 ** 29, 2 ** 28, 0] and W == 3 * 2 ** 28
    wq, W = twin.quantise(np.array([3.0, 1.0], np.float32), 2)              # 3 2^28 <= 2^30 < 3 2^29
    assert list(wq) == [3 * 2 ** 28, 2 ** 28]
    wq, _ = twin.quantise(np.array([4.0, 2.0 ** -29, 3 * 2.0 ** -30], np.float32), 3)    # e = 28: 0.5 and 0.75
    assert list(wq) == [2 ** 30, 0, 1]                                      # ties to even, as llrint


def test_a_zero_weight_contributes_nothing():
    w = HAND_W.copy()
    keep = w > 0
    a = twin.triplet_stats(HAND, 3, [(0, 1, 3)], w)
    b = twin.triplet_stats(HAND[keep], 3, [(0, 1, 3)], w[keep])
    np.testing.assert_array_equal(a["counts"], b["counts"])
    assert a["total"] == b["total"]


def test_a_total_weight_of_zero_is_refused():
    with pytest.raises(ValueError):
        twin.quantise(np.zeros(4, np.float32), 4)
    with pytest.raises(ValueError):
        twin.quantise(np.full(4, 1e-30, np.float32), 4)                     # e stops at 30: every wq rounds to 0
    _einval(lambda: plm.triplet_stats(HAND, 3, TRIP, weights=np.full(len(HAND), 1e-30, np.float32)), "W = 0")
    wq, W = twin.quantise(np.array([1e30, 1e-30], np.float32), 2)           # the tiny weight rounds to 0, W stays > 0
    assert wq[1] == 0 and W == wq[0] > 0


@pytest.mark.parametrize("sites", [3, 4, 7, [0, 2, 5, 6, 11], [4, 9, 10]])
def test_triplet_index_is_itertools_combinations(sites):
    seq = range(sites) if isinstance(sites, int) else sites
    got = plm.triplet_index(sites)
    assert got.dtype == np.int32 and got.shape == (len(list(itertools.combinations(seq, 3))), 3)
    np.testing.assert_array_equal(got, np.array(list(itertools.combinations(seq, 3))))


def test_the_scan_of_the_twin_is_the_listed_call_on_the_table():
    trip, norm2, maxabs, arg, _ = twin.triplet_scan(HAND, 3, HAND_W, skip_state=0)
    assert len(trip) == 4
    probed = twin.triplet_scan(HAND, 3, HAND_W, skip_state=0, probe=arg)[4]
    for t in range(4):
        want = twin.reductions(twin.triplet_stats(HAND, 3, [trip[t]], HAND_W)["connected"][0], 0)
        assert (norm2[t], maxabs[t], arg[t]) == want
        assert 0 not in (arg[t] // 9, arg[t] // 3 % 3, arg[t] % 3) and probed[t] == maxabs[t]


# ---- the library's argument checks: they run before the device is looked at, so they are the same on every machine

def _einval(call, word):
    with pytest.raises(_lib.PlmError) as err:
        call()
    assert err.value.code == -1 and word in str(err.value), str(err.value)


TRIP = [(0, 1, 2)]


def test_bad_arguments_are_refused_before_the_device_is_looked_at():
    q = 3
    for call in (lambda m, **kw: plm.triplet_stats(m, kw.pop("q", q), kw.pop("triplets", TRIP), **kw),
                 lambda m, **kw: plm.triplet_scan(m, kw.pop("q", q), **{k: v for k, v in kw.items() if k != "triplets"})):
        _einval(lambda: call(np.zeros((0, 4), np.int8)), "n_seqs")
        _einval(lambda: call(HAND[:, :2], triplets=[(0, 1, 2)]), "n_sites")
        _einval(lambda: call(HAND, q=1), "2..32")
        _einval(lambda: call(HAND, q=33), "2..32")
        _einval(lambda: call(HAND, q=2), "outside 0..1")                      # HAND holds state 2
        _einval(lambda: call(-HAND), "outside 0..2")
        _einval(lambda: call(HAND, skip_state=3), "skip_state")
        _einval(lambda: call(HAND, skip_state=-2), "skip_state")
        _einval(lambda: call(HAND, weights=-HAND_W), "negative")
        _einval(lambda: call(HAND, weights=np.where(HAND_W > 0.9, np.nan, HAND_W)), "finite")
        _einval(lambda: call(HAND, weights=np.where(HAND_W > 0.9, np.inf, HAND_W)), "finite")
        _einval(lambda: call(HAND, weights=np.zeros(len(HAND), np.float32)), "W = 0")


def test_bad_triplets_and_selections_are_refused_before_the_device_is_looked_at():
    for bad in ([(0, 0, 1)], [(0, 2, 1)], [(1, 0, 2)], [(0, 1, 4)], [(-1, 1, 2)], [(0, 1, 2), (2, 3, 3)]):
        _einval(lambda: plm.triplet_stats(HAND, 3, bad), "i < j < k")
    _einval(lambda: plm.triplet_stats(HAND, 3, np.zeros((0, 3), np.int32)), "n_triplets")
    for bad in ([0, 1], [0, 2, 2], [0, 2, 1], [1, 2, 4], [-1, 0, 1], []):
        _einval(lambda: plm.triplet_scan(HAND, 3, sites=bad), "sites" if len(bad) >= 3 else "fewer than 3")


def test_null_pointers_are_refused():
    lib = _lib.load()
    opts = _lib.PlmTripletOpts(-1, 7)
    trip = np.array(TRIP, np.int32)
    assert lib.plm_triplet_stats(None, None, 7, 4, 3, plm._ptr(trip), 1, opts, None, None, None, None, 0, None) == -1
    assert lib.plm_triplet_stats(plm._ptr(HAND), None, 7, 4, 3, plm._ptr(trip), 1, None, None, None, None, None, 0, None) == -1
    assert lib.plm_triplet_stats(plm._ptr(HAND), None, 7, 4, 3, None, 1, opts, None, None, None, None, 0, None) == -1
    assert lib.plm_triplet_scan(None, None, 7, 4, 3, None, 0, opts, None, None, None, None, 0, None) == -1
    assert lib.plm_triplet_scan(plm._ptr(HAND), None, 7, 4, 3, None, 0, None, None, None, None, None, 0, None) == -1


@pytest.mark.parametrize("value", ["", "w16", "w", "n0", "n-4", "c33", "c0", "k0", "k70000", "x4", "w32,", ",w32", "w32 n8",
                                   "w32;n8", "u1", "n12x"])
def test_a_bad_plan_hook_is_refused_before_the_device_is_looked_at(monkeypatch, value):
    monkeypatch.setenv("PLM_TRIPLET_PLAN", value)
    for call in (lambda: plm.triplet_stats(HAND, 3, TRIP), lambda: plm.triplet_scan(HAND, 3)):
        with pytest.raises(_lib.PlmError) as err:
            call()
        assert err.value.code == -1 and "PLM_TRIPLET_PLAN" in str(err.value)


def test_narrow_counters_cannot_be_forced_on_a_wide_total(monkeypatch):
    monkeypatch.setenv("PLM_TRIPLET_PLAN", "w32")
    _einval(lambda: plm.triplet_stats(HAND, 3, TRIP, weights=np.ones(len(HAND), np.float32)), "64-bit")


def test_no_cpu_fallback_without_a_gpu(monkeypatch):
    if _lib.load().plm_device_count() > 0:
        pytest.skip("GPU present")
    for plan in (None, "w64,n8,c2,k3,u"):
        if plan:
            monkeypatch.setenv("PLM_TRIPLET_PLAN", plan)
        for call in (lambda: plm.triplet_stats(HAND, 3, TRIP, weights=HAND_W), lambda: plm.triplet_scan(HAND, 3)):
            with pytest.raises(_lib.PlmError) as err:
                call()
            assert err.value.code == -3


# ---- evcouplings_amd.correlations: what runs without a device

def test_pearson_and_slope_by_hand():
    x = np.array([0.0, 1.0, 2.0, 3.0])
    r, s = correlations.pearson_and_slope(x, 2 * x + 1)
    assert abs(r - 1) < 1e-15 and abs(s - 2) < 1e-15
    r, s = correlations.pearson_and_slope(x, -0.5 * x)
    assert abs(r + 1) < 1e-15 and abs(s + 0.5) < 1e-15
    assert np.isnan(correlations.pearson_and_slope(x, np.ones(4))[0])


def test_connected_pairs_are_zero_for_independent_columns():
    fi = np.array([[0.25, 0.75], [0.5, 0.5], [1.0, 0.0]])
    i, j = np.triu_indices(3, 1)
    fij = fi[i][:, :, None] * fi[j][:, None, :]
    assert (correlations.connected_pairs(fi, fij) == 0).all()


def test_command_line_arguments():
    a = correlations.parse_args(["nat.a2m", "sam.a2m"])
    assert (a.natural, a.sample, a.theta, a.top, a.output, a.rank_by, a.skip_gap) == \
        ("nat.a2m", "sam.a2m", 0.8, 1000, None, "norm2", False)
    a = correlations.parse_args(["n", "s", "--theta", "0.9", "--top", "5", "-o", "out.csv", "--rank-by", "maxabs", "--skip-gap"])
    assert (a.theta, a.top, a.output, a.rank_by, a.skip_gap) == (0.9, 5, "out.csv", "maxabs", True)
    for bad in (["n"], ["n", "s", "--top", "0"], ["n", "s", "--theta", "0"], ["n", "s", "--rank-by", "sum"]):
        with pytest.raises(SystemExit):
            correlations.parse_args(bad)


def test_table_writer_on_twin_outputs(tmp_path):
    trip, norm2, maxabs, _, _ = twin.triplet_scan(HAND, 3, HAND_W)
    top = np.argsort(-norm2, kind="stable")[:3]
    res = {"triplets": trip[top], "scores": norm2[top], "natural_norm2": norm2[top], "sample_norm2": norm2[top] / 2,
           "natural_maxabs": maxabs[top], "sample_maxabs": maxabs[top] / 2}
    path = correlations.write_table(str(tmp_path / "t.csv"), res)
    lines = open(path).read().splitlines()
    assert lines[0] == "i,j,k,score,natural_norm2,sample_norm2,natural_maxabs,sample_maxabs" and len(lines) == 4
    for t, line in enumerate(lines[1:]):
        cells = line.split(",")
        assert [int(c) for c in cells[:3]] == list(trip[top][t])
        assert float(cells[3]) == norm2[top][t] == float(cells[4]) and float(cells[7]) == maxabs[top][t] / 2     # %.17g round-trips
    assert float(lines[1].split(",")[3]) >= float(lines[3].split(",")[3])
