"""plm_mutant_effects and plm_mutant_scan on the GPU (DESIGN_NEXT_ROWS.md section 9.16) against the numpy float64 twin
(tests/mutants_twin.py) and the reference's fixture (tests/golden/mutation_table_L24.npz).

Tolerance: no constant.  The library and the twin both sum, in float64, the same float32 values, each in its own order, so
|got - want| <= 2 n_terms 2^-53 sum_abs per variant (mutants_twin.bound), n_terms and sum_abs being the count and the
absolute sum of the h and J values that enter.  The same bound holds against the fixture: the reference sums the same
values in a third order."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mutants_twin as mt  # noqa: E402
from evcouplings_amd import model_io  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.abspath(__file__))
SHORT = 8                      # MU_SHORT of plm_mutants.hip: longer variants take the wave kernel


@pytest.fixture(scope="module")
def plm():
    from evcouplings_amd import plm as mod
    assert mod.device_count() >= 1
    return mod


def rand_model(L, q, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    h = rng.normal(size=(L, q)).astype(np.float32)
    J = (scale * rng.normal(size=(L * (L - 1) // 2, q, q))).astype(np.float32)
    return h, J, rng.integers(0, q, L).astype(np.int8)


def variant(rng, L, q, M):
    return rng.choice(L, M, replace=False).tolist(), rng.integers(0, q, M).tolist()


def mixed_variants(L, q, n, seed):
    """n variants of mixed length: 0, 1, the thread kernel's last length, the wave kernel's first, L; with n >= 63 a run
    of empty variants at both ends"""
    rng = np.random.default_rng(seed)
    lengths = sorted({min(L, M) for M in (0, 1, 2, 3, 5, SHORT, SHORT + 1)})     # and L itself at every 50th variant
    out = [variant(rng, L, q, lengths[(3 * k + k // 7) % len(lengths)] if k % 50 else L) for k in range(n)]
    if n == 1:
        return [variant(rng, L, q, min(L, 2))]
    if n >= 63:
        out[:3] = [([], [])] * 3
        out[-4:] = [([], [])] * 4
    return out


def assert_within_bound(got, status, variants, model, where=""):
    h, J, target = model
    q = h.shape[1]
    want, st, n_terms, sum_abs = mt.mutant_effects(target, q, h, J, *mt.csr(variants), info=True)
    assert np.array_equal(status, st), where
    ok = st == 0
    assert np.isnan(got[~ok]).all(), where
    err = np.abs(got[ok] - want[ok])
    bound = mt.bound(n_terms, sum_abs)[ok]
    print("%s: %d variants, largest error %.3g, largest share of the bound %.3g" % (
        where, len(variants), err.max(initial=0.0), (err.max(axis=1) / np.maximum(bound, 1e-300)).max(initial=0.0)))
    assert (err <= bound[:, None]).all(), where
    return want


# ---- the fixture ---------------------------------------------------------------------------------------------------

def test_golden_table_and_single_mutant_matrix(plm, golden_dir):
    z = np.load(os.path.join(golden_dir, "mutation_table_L24.npz"))
    m = model_io.read_model_file(os.path.join(golden_dir, "hip_fit_L24.model"))
    code = {a: k for k, a in enumerate(m["alphabet"])}
    target = np.array([code[c] for c in m["target_seq"]], np.int8)
    L, q = m["L"], m["q"]
    out, status, tab = plm.mutant_effects(target, q, m["hi"], m["jij"], z["offsets"], z["positions"], z["states"], tables=True)
    _, st, n_terms, sum_abs = mt.mutant_effects(target, q, m["hi"], m["jij"], z["offsets"], z["positions"], z["states"], info=True)
    assert np.array_equal(status, st)
    rejected = np.isnan(z["delta"][:, 0])
    assert np.array_equal(rejected, (status != 0) | z["from_mismatch"])      # the from-letter is the parser's business
    assert np.isnan(out[status != 0]).all() and not np.isnan(out[status == 0]).any()
    ok = ~rejected
    err = np.abs(out[ok] - z["delta"][ok])
    bound = mt.bound(n_terms, sum_abs)[ok]
    print("fixture: largest error %.3g, largest share of the bound %.3g" % (
        err.max(), (err.max(axis=1) / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound[:, None]).all()
    # tables_out against the reference's single-mutant matrix.  Its J part is float64 arithmetic; its field part is
    # h_i(a) - h_i(t_i) subtracted in float32 (the reference's h_i array is float32), i.e. the exact difference, which
    # S_h holds, rounded once to float32: the test rounds S_h the same way, and the bound stays the twin's.
    smm = np.load(os.path.join(golden_dir, "model_analysis_L24.npz"))["single_mut_mat"]
    singles = [([i], [a]) for i in range(L) for a in range(q)]
    _, _, n1, s1 = mt.mutant_effects(target, q, m["hi"], m["jij"], *mt.csr(singles), info=True)
    got = tab[:, :, 0] + tab[:, :, 1].astype(np.float32).astype(np.float64)
    err = np.abs(got - smm)
    print("single-mutant matrix: largest error %.3g" % err.max())
    assert (err <= mt.bound(n1, s1).reshape(L, q)).all()
    assert (np.abs(tab - mt.single_tables(target, q, m["hi"], m["jij"])) <= mt.bound(n1, s1).reshape(L, q, 1)).all()
    # the rows as the model level sees them: the parser's NaN rows are the reference's
    from evcouplings_amd import model_accel, sample
    model = sample.model_from_file(os.path.join(golden_dir, "hip_fit_L24.model"))
    table = model_accel._effects(model, model_accel.parse_mutations(model, list(z["mutants"])))
    assert np.array_equal(np.isnan(table[:, 0]), rejected) and np.array_equal(table[ok], out[ok])


# ---- exhaustive ----------------------------------------------------------------------------------------------------

def test_every_sequence_of_a_small_model(plm):
    L, q = 5, 3
    model = h, J, target = rand_model(L, q, 11)
    seqs = np.array(list(itertools.product(range(q), repeat=L)), np.int8)
    differing = [(np.nonzero(s != target)[0].tolist(), s[s != target].tolist()) for s in seqs]
    explicit = [(list(range(L)), s.tolist()) for s in seqs]
    H = plm.hamiltonians(np.vstack([target[None], seqs]), q, h, J)
    # plm_hamiltonians works in float32 products: tests/test_gpu_parity.py holds it to rtol 2e-5 and atol 2e-5 max|H|
    # against float64; a difference of two such energies errs by at most twice that
    tol = 2 * 2e-5 * np.abs(H).max()
    for name, variants in (("differing sites", differing), ("all sites named", explicit)):
        out, status = plm.mutant_effects(target, q, h, J, *mt.csr(variants))
        assert_within_bound(out, status, variants, model, name)
        np.testing.assert_allclose(out, H[1:] - H[0], rtol=2e-5, atol=tol)
    k = int(np.nonzero((seqs == target).all(axis=1))[0][0])
    assert np.array_equal(plm.mutant_effects(target, q, h, J, *mt.csr(differing))[0][k], np.zeros(3))


# ---- shapes --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,q", [(2, 2), (33, 21), (65, 32), (24, 21)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_shapes_and_mixed_lengths(plm, L, q, n):
    model = h, J, target = rand_model(L, q, 100 * L + q)
    variants = mixed_variants(L, q, n, seed=n)
    lens = {len(p) for p, _ in variants}
    assert n < 63 or {0, 1, L} <= lens
    out, status = plm.mutant_effects(target, q, h, J, *mt.csr(variants))
    assert out.shape == (n, 3) and status.dtype == np.uint8 and not status.any()
    assert_within_bound(out, status, variants, model, "L=%d q=%d n=%d" % (L, q, n))
    empty = np.array([len(p) == 0 for p, _ in variants])
    assert np.array_equal(out[empty], np.zeros((empty.sum(), 3)))


def test_malformed_rows_leave_their_neighbours_alone(plm):
    L, q = 12, 4
    model = h, J, target = rand_model(L, q, 5)
    rng = np.random.default_rng(6)
    good = [variant(rng, L, q, M) for M in (0, 1, 2, 3, 8, 9, 12, 5, 1, 10, 2, 4, 11, 3)]
    long_p, long_s = variant(rng, L, q, 10)
    bad = {
        1: (mt.ETOOMANY, (list(range(L)) + [0], [1] * (L + 1))),
        3: (mt.EPOSITION, ([2, L, 5], [1, 1, 1])),
        4: (mt.EPOSITION, ([3, -1], [0, 0])),
        6: (mt.ESTATE, ([2, 7], [1, q])),
        7: (mt.ESTATE, ([4], [-1])),
        9: (mt.EREPEAT, ([2, 7, 2], [1, 0, 3])),
        # the same causes in variants long enough for the wave kernel
        10: (mt.EPOSITION, (long_p[:-1] + [L + 3], long_s)),
        11: (mt.ESTATE, (long_p, long_s[:-1] + [q + 1])),
        12: (mt.EREPEAT, (long_p[:-1] + [long_p[0]], long_s)),
        13: (mt.EPOSITION, ([L] + long_p[1:], [q] + long_s[1:])),            # position and state: the position is named
    }
    mixed, is_bad = [], []
    for k, g in enumerate(good):
        if k in bad:
            mixed.append(bad[k][1])
            is_bad.append(bad[k][0])
        mixed.append(g)
        is_bad.append(0)
    is_bad = np.array(is_bad)
    alone, st_alone = plm.mutant_effects(target, q, h, J, *mt.csr(good))
    out, status = plm.mutant_effects(target, q, h, J, *mt.csr(mixed))        # returns: the call is PLM_OK
    assert not st_alone.any() and np.array_equal(status, is_bad)
    assert {mt.ETOOMANY, mt.EPOSITION, mt.ESTATE, mt.EREPEAT} <= set(status.tolist())
    assert np.isnan(out[is_bad != 0]).all()
    assert out[is_bad == 0].tobytes() == alone.tobytes()                     # bit for bit
    assert_within_bound(out, status, mixed, model, "malformed rows")


def test_two_calls_return_the_same_bits(plm):
    h, J, target = rand_model(33, 21, 9)
    args = mt.csr(mixed_variants(33, 21, 1000, seed=3))
    a, b = plm.mutant_effects(target, 21, h, J, *args, tables=True), plm.mutant_effects(target, 21, h, J, *args, tables=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    scan = [plm.mutant_scan(target, 21, h, J, [30, 2, 17], energies=True, edges=np.linspace(-9, 9, 50), threshold=1.0,
                            capacity=9261) for _ in range(2)]
    for key in ("energies", "histogram", "kept_index", "kept_energies"):
        assert scan[0][key].tobytes() == scan[1][key].tobytes()
    assert (scan[0]["dh_min"], scan[0]["dh_max"], scan[0]["n_kept"]) == (scan[1]["dh_min"], scan[1]["dh_max"], scan[1]["n_kept"])


def test_independent_model_has_no_coupling_part(plm):
    h, J, target = rand_model(24, 21, 4, scale=0.0)
    variants = mixed_variants(24, 21, 200, seed=1)
    out, status = plm.mutant_effects(target, 21, h, J, *mt.csr(variants))
    assert not status.any() and np.array_equal(out[:, 1], np.zeros(200)) and np.array_equal(out[:, 0], out[:, 2])
    assert np.abs(out[:, 2]).max() > 0
    res = plm.mutant_scan(target, 21, h, J, [3, 20], energies=True)
    assert np.array_equal(res["energies"][:, 1], np.zeros(441))


# ---- the scan --------------------------------------------------------------------------------------------------------

def check_scan(plm, model, sites, letters=None, first=0, count=None, where="", **kw):
    """a scan against the twin and against plm.mutant_effects on the same combinations written out"""
    h, J, target = model
    q = h.shape[1]
    res = plm.mutant_scan(target, q, h, J, sites, letters=letters, first=first, count=count, energies=True, **kw)
    variants = mt.scan_variants(q, sites, letters, first, count)
    assert res["count"] == len(variants) and res["energies"].shape == (len(variants), 3)
    assert_within_bound(res["energies"], np.zeros(len(variants), np.uint8), variants, model, where)
    out, status = plm.mutant_effects(target, q, h, J, *mt.csr(variants))
    _, _, n_terms, sum_abs = mt.mutant_effects(target, q, h, J, *mt.csr(variants), info=True)
    assert not status.any() and (np.abs(out - res["energies"]) <= mt.bound(n_terms, sum_abs)[:, None]).all(), where
    assert res["dh_min"] == res["energies"][:, 0].min() and res["dh_max"] == res["energies"][:, 0].max()
    return res


def test_scan_of_one_site_is_the_single_table(plm):
    model = h, J, target = rand_model(24, 21, 31)
    _, _, tab = plm.mutant_effects(target, 21, h, J, [0], [], [], tables=True)
    for site in (0, 7, 23):
        en = check_scan(plm, model, [site], where="k=1 site %d" % site)["energies"]
        assert np.array_equal(en[:, 1], tab[site, :, 0]) and np.array_equal(en[:, 2], tab[site, :, 1])
        assert np.array_equal(en[:, 0], tab[site, :, 0] + tab[site, :, 1])


def test_scan_of_two_sites_is_the_double_mutant_block(plm, golden_dir):
    m = model_io.read_model_file(os.path.join(golden_dir, "hip_fit_L24.model"))
    z = np.load(os.path.join(golden_dir, "model_analysis_L24.npz"))
    code = {a: k for k, a in enumerate(m["alphabet"])}
    target = np.array([code[c] for c in m["target_seq"]], np.int8)
    L, q = m["L"], m["q"]
    model = (m["hi"], m["jij"], target)
    _, _, tab = plm.mutant_effects(target, q, m["hi"], m["jij"], [0], [], [], tables=True)
    dense = mt.dense(m["hi"], m["jij"], q)[1]
    D = plm.double_mutant_matrix(dense, tab[:, :, 0] + tab[:, :, 1], target)
    for i, j in z["dmm_pairs"][[0, 1, 2, 17, 40]]:
        res = check_scan(plm, model, [int(i), int(j)], where="k=2 pair (%d, %d)" % (i, j))
        en = res["energies"][:, 0].reshape(q, q)
        variants = mt.scan_variants(q, [int(i), int(j)])
        _, _, n_terms, sum_abs = mt.mutant_effects(target, q, m["hi"], m["jij"], *mt.csr(variants), info=True)
        bound = mt.bound(n_terms, sum_abs).reshape(q, q)
        assert (np.abs(en - D[i, j]) <= bound).all()                          # the same values in plm_double_mutants' order
        # the fixture's block is built on the reference's single-mutant matrix, whose two field differences were each
        # rounded to float32 (relative 2^-24 at most); everything else is the float64 sum the bound covers
        k = int(np.nonzero((z["dmm_pairs"] == (i, j)).all(axis=1))[0][0])
        rounding = 2.0 ** -24 * (np.abs(tab[i, :, 1])[:, None] + np.abs(tab[j, :, 1])[None, :])
        assert (np.abs(en - z["dmm_blocks"][k]) <= bound + rounding).all()


@pytest.mark.parametrize("first,count", [(0, None), (1, 4), (3, 3)])
def test_scan_of_three_sites_with_letter_lists(plm, first, count):
    model = rand_model(9, 6, 41)
    check_scan(plm, model, [4, 0, 8], letters=[[5, 1], [0, 2, 3], [4]], first=first, count=count, where="k=3 lists (2,3,1)")


@pytest.mark.parametrize("first,count", [(0, None), (37, 300), (250, 270), (64, 256), (511, 114), (624, 1)])
def test_scan_of_four_sites_in_ranges(plm, first, count):
    """625 combinations; ranges that start and end off the multiples of 64 and 256"""
    model = rand_model(11, 7, 43)
    letters = [[0, 1, 2, 3, 4], [6, 5, 4, 3, 2], [1, 3, 5, 0, 6], [2, 0, 6, 4, 1]]
    check_scan(plm, model, [2, 9, 5, 7], letters=letters, first=first, count=count, where="k=4 [%d, +%s)" % (first, count))


def test_scan_of_eight_sites(plm):
    """q = 21, two letters per site (256 combinations); then all 21 letters (28 pair tables, 99 KB) and q = 32 (229 KB):
    ranges deep inside the library"""
    model = h, J, target = rand_model(10, 21, 47)
    sites = [9, 0, 3, 7, 1, 8, 5, 2]                          # not in order
    rng = np.random.default_rng(2)
    letters = [rng.choice(21, 2, replace=False).tolist() for _ in sites]
    check_scan(plm, model, sites, letters=letters, where="k=8 two letters")
    first = 21 ** 8 - 30000 - 77
    a = check_scan(plm, model, sites, first=first, count=300, where="k=8 all letters")
    assert a["n_combinations"] == 21 ** 8
    last = check_scan(plm, model, sites, first=21 ** 8 - 5, count=5, where="k=8 the last five")
    assert last["first"] + last["count"] == 21 ** 8
    model32 = rand_model(8, 32, 48)
    wide = check_scan(plm, model32, list(range(7, -1, -1)), first=32 ** 8 - 123456789, count=300, where="k=8 q=32")
    assert wide["n_combinations"] == 32 ** 8


def test_scan_with_sites_in_descending_order(plm):
    model = rand_model(12, 5, 53)
    down = check_scan(plm, model, [10, 6, 1], where="descending sites")["energies"]
    up = check_scan(plm, model, [1, 6, 10], where="ascending sites")["energies"]
    # the same library in another order: combination (a, b, c) of one is (c, b, a) of the other
    want = up.reshape(5, 5, 5, 3).transpose(2, 1, 0, 3).reshape(125, 3)
    variants = mt.scan_variants(5, [10, 6, 1])
    _, _, n_terms, sum_abs = mt.mutant_effects(model[2], 5, model[0], model[1], *mt.csr(variants), info=True)
    assert (np.abs(down - want) <= mt.bound(n_terms, sum_abs)[:, None]).all()


def test_histogram_extremes_and_compaction(plm):
    """9^4 = 6561 combinations: more than one workgroup"""
    h, J, target = rand_model(14, 9, 59)
    sites = [13, 4, 8, 0]
    en = plm.mutant_scan(target, 9, h, J, sites, energies=True)["energies"]
    dH = en[:, 0]
    # edges: a grid, two of the energies themselves (an edge equal to a value counts as <= it), a repeated edge
    edges = np.sort(np.concatenate([np.linspace(dH.min() - 1, dH.max() + 1, 200), dH[[5, 4000]], [dH[77], dH[77]]]))
    thr = float(np.sort(dH)[-500])
    for first, count in ((0, 6561), (100, 5000), (6000, 561)):
        res = plm.mutant_scan(target, 9, h, J, sites, first=first, count=count, energies=True, edges=edges, threshold=thr,
                              capacity=count)
        part = dH[first:first + count]
        assert res["energies"].tobytes() == en[first:first + count].tobytes()
        want = np.bincount(np.searchsorted(edges, part, side="right"), minlength=len(edges) + 1)
        assert res["histogram"].dtype == np.uint64 and np.array_equal(res["histogram"], want.astype(np.uint64))
        assert int(res["histogram"].sum()) == count
        assert res["dh_min"] == part.min() and res["dh_max"] == part.max()
        keep = np.nonzero(part >= thr)[0]
        assert res["n_kept"] == len(keep) and np.array_equal(res["kept_index"], keep + first)
        assert res["kept_energies"].tobytes() == en[keep + first].tobytes()
    assert res["n_kept"] < 500 <= plm.mutant_scan(target, 9, h, J, sites, threshold=thr, capacity=0)["n_kept"]
    # a buffer that is too small: the call returns, n_kept is the true number, the buffer is not handed out
    small = plm.mutant_scan(target, 9, h, J, sites, threshold=thr, capacity=499)
    assert small["n_kept"] == 500 and small["kept_index"] is None
    exact = plm.mutant_scan(target, 9, h, J, sites, threshold=thr, capacity=500)
    assert np.array_equal(exact["kept_index"], np.nonzero(dH >= thr)[0])
    # histogram alone, and with no edge at all
    only = plm.mutant_scan(target, 9, h, J, sites, edges=edges[:3])
    assert np.array_equal(only["histogram"], np.bincount(np.searchsorted(edges[:3], dH, side="right"), minlength=4).astype(np.uint64))
    assert plm.mutant_scan(target, 9, h, J, sites, edges=[])["histogram"].tolist() == [6561]
    assert plm.mutant_scan(target, 9, h, J, sites, first=17, count=0)["dh_min"] == np.inf


# ---- top_combinations ------------------------------------------------------------------------------------------------

TOP_SEED, TOP_K = 61, 10


def test_top_combinations_on_a_model_of_three_sites(plm):
    L, q = 3, 5
    h, J, target = rand_model(L, q, TOP_SEED)
    info = mt.mutant_scan(target, q, h, J, [0, 1, 2], energies=True, info=True)
    dH = info["energies"][:, 0]
    order = np.lexsort((np.arange(125), -dH))
    gaps = -np.diff(dH[order[:TOP_K + 1]])
    bound = mt.bound(info["n_terms"], info["sum_abs"]).max()
    assert gaps.min() > 4 * bound                              # the order of the best K + 1 cannot depend on the rounding
    idx, en = plm.top_combinations(target, q, h, J, [0, 1, 2], top=TOP_K)
    assert idx.dtype == np.int64 and np.array_equal(idx, order[:TOP_K])
    assert (np.abs(en - info["energies"][order[:TOP_K]]) <= bound).all()
    # the refinement path: no threshold may keep more than 12 combinations
    idx2, en2 = plm.top_combinations(target, q, h, J, [0, 1, 2], top=TOP_K, max_keep=12)
    assert np.array_equal(idx2, idx) and en2.tobytes() == en.tobytes()
    everything, _ = plm.top_combinations(target, q, h, J, [0, 1, 2], top=1000)
    assert np.array_equal(everything[:TOP_K], idx) and sorted(everything.tolist()) == list(range(125))


def test_top_combinations_returns_exact_ties_in_index_order(plm):
    L, q = 3, 5
    h, J, target = rand_model(L, q, 67, scale=0.0)
    h[:, 3] = h[:, 1] = h.max(axis=1) + 1                      # two best letters with identical fields at every site
    target[:] = 0
    idx, en = plm.top_combinations(target, q, h, J, [0, 1, 2], top=6)
    digits = plm.scan_digits(idx, [5, 5, 5])
    assert np.isin(digits, (1, 3)).all() and idx.tolist() == sorted(idx.tolist()) and len(set(en[:, 0].tolist())) == 1
    assert idx.tolist() == [1 * 25 + 1 * 5 + 1, 1 * 25 + 1 * 5 + 3, 1 * 25 + 3 * 5 + 1, 1 * 25 + 3 * 5 + 3, 3 * 25 + 1 * 5 + 1,
                            3 * 25 + 1 * 5 + 3]
    idx2, _ = plm.top_combinations(target, q, h, J, [0, 1, 2], top=6, max_keep=6, chunk=50)
    assert idx2.tolist() == idx.tolist()
