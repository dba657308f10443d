"""Inter-protein energies and paralog matching (plm_cross_energies, plm_group_assignment; DESIGN_NEXT_ROWS.md section
9.23) without a GPU: the binding, the validation that comes before the device check, inter_blocks, the numpy twin
(tests/cross_twin.py), the assignment (host code of the library, so it runs here), and match_by_species and the command
line with plm.cross_energies replaced by the twin."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cross_twin as tw  # noqa: E402
from evcouplings_amd import _lib, complex_accel, model_io, pairing, plm  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
OK, EINVAL, EDEVICE, EUNSUPPORTED = 0, -1, -3, -4


# ---- binding and validation --------------------------------------------------------------------------------------

def test_binding_is_declared_and_matches_the_header_layout():
    names = {name for name, _, _ in _lib.SYMBOLS}
    assert {"plm_cross_energies", "plm_group_assignment"} <= names
    lib = _lib.load()
    assert hasattr(lib, "plm_cross_energies") and hasattr(lib, "plm_group_assignment")
    o, b = _lib.PlmCrossOpts, _lib.PlmCrossBest
    assert (o.skip_state.offset, o.want_best.offset, C.sizeof(o)) == (0, 4, 8)
    assert (b.index.offset, b.best.offset, b.second.offset, C.sizeof(b)) == (0, 8, 16, 24)
    assert plm.CROSS_BEST.itemsize == 24 and plm.CROSS_BEST.names == ("index", "best", "second")
    assert [plm.CROSS_BEST.fields[n][1] for n in plm.CROSS_BEST.names] == [0, 8, 16] and tw.BEST == plm.CROSS_BEST
    text = open(os.path.join(os.path.dirname(ROOT), "include", "plm_hip.h")).read()
    assert "} plm_cross_opts;" in text and "} plm_cross_best;" in text
    flat = " ".join(text.split())
    assert "typedef struct { int32_t skip_state;" in flat and "int32_t want_best;" in flat
    assert "typedef struct { int64_t index; double best; double second; } plm_cross_best;" in flat


def _valid(LA=2, LB=3, q=4, n_a=3, n_b=5):
    rng = np.random.default_rng(1)
    return dict(jab=rng.normal(size=(LA, LB, q, q)).astype(np.float32), LA=LA, LB=LB, q=q,
                a=rng.integers(0, q, (n_a, LA)).astype(np.int8), n_a=n_a, b=rng.integers(0, q, (n_b, LB)).astype(np.int8),
                n_b=n_b, n_groups=2, ao=np.array([0, 1, n_a], np.int64), bo=np.array([0, 2, n_b], np.int64), skip=-1, want=1,
                opts=True, matrix=True, rows=True, cols=True)


def _call(**kw):
    lib = _lib.load()
    v = _valid()
    v.update(kw)
    p = plm._ptr
    opts = _lib.PlmCrossOpts(v["skip"], v["want"])
    m = np.zeros(64)
    rows, cols = np.zeros(16, plm.CROSS_BEST), np.zeros(16, plm.CROSS_BEST)
    return lib.plm_cross_energies(p(v["jab"]), v["LA"], v["LB"], v["q"], p(v["a"]), v["n_a"], p(v["b"]), v["n_b"], v["n_groups"],
                                  p(v["ao"]), p(v["bo"]), C.byref(opts) if v["opts"] else None, 0, None,
                                  p(m) if v["matrix"] else None, p(rows) if v["rows"] else None, p(cols) if v["cols"] else None)


def test_cross_validation_comes_before_the_device():
    lib = _lib.load()
    for name in ("jab", "a", "b", "ao", "bo"):
        assert _call(**{name: None}) == EINVAL, name
    assert _call(opts=False) == EINVAL
    assert _call(matrix=False, rows=False, cols=False) == EINVAL
    assert _call(matrix=False, want=0) == EINVAL                               # the best arrays are not asked for
    assert _call(LA=0) == EINVAL and _call(LB=0) == EINVAL and _call(LA=-1) == EINVAL
    assert _call(n_a=-1) == EINVAL and _call(n_b=-1) == EINVAL and _call(n_groups=-1) == EINVAL
    assert _call(q=1) == EUNSUPPORTED and _call(q=33) == EUNSUPPORTED
    assert _call(ao=np.array([1, 1, 3], np.int64)) == EINVAL                   # does not start at 0
    assert _call(ao=np.array([0, 2, 1], np.int64), n_a=1) == EINVAL            # decreases
    assert _call(ao=np.array([0, 1, 2], np.int64)) == EINVAL                   # ends before the rows do
    assert _call(bo=np.array([0, 2, 6], np.int64)) == EINVAL and _call(bo=np.array([-1, 2, 5], np.int64)) == EINVAL
    assert b"b_offsets" in lib.plm_last_error()
    bad = _valid()["a"].copy()
    bad[2, 1] = 4
    assert _call(a=bad) == EINVAL and b"seqs_a[2][1]" in lib.plm_last_error()
    bad = _valid()["b"].copy()
    bad[4, 0] = -1
    assert _call(b=bad) == EINVAL and b"seqs_b[4][0]" in lib.plm_last_error()
    assert _call(skip=-2) == EINVAL and _call(skip=4) == EINVAL
    if lib.plm_device_count() <= 0:                                            # valid calls: no CPU path
        assert _call() == EDEVICE and _call(skip=3) == EDEVICE and _call(skip=0, matrix=False) == EDEVICE
        assert _call(rows=False, cols=False, want=0) == EDEVICE and _call(matrix=False, cols=False) == EDEVICE
        assert _call(n_groups=0, n_a=0, n_b=0, ao=np.zeros(1, np.int64), bo=np.zeros(1, np.int64)) == EDEVICE
        with pytest.raises(_lib.PlmError):
            plm.cross_energies(_valid()["jab"], _valid()["a"], _valid()["b"])
    v = _valid()
    with pytest.raises(ValueError):
        plm.cross_energies(v["jab"], v["a"][:, :1], v["b"])
    with pytest.raises(ValueError):
        plm.cross_energies(v["jab"], v["a"], v["b"], a_offsets=[0, 3])
    with pytest.raises(ValueError):
        plm.cross_energies(v["jab"], v["a"], v["b"], matrix=False, best=False)
    with pytest.raises(ValueError):
        plm.cross_energies(v["jab"][0], v["a"], v["b"])


@pytest.mark.parametrize("name", ["PLM_CROSS_TILE", "PLM_CROSS_VCHUNK"])
@pytest.mark.parametrize("value", ["0", "abc", "-3", "12x", ""])
def test_a_bad_plan_hook_is_refused_before_the_device_is_looked_at(monkeypatch, name, value):
    monkeypatch.setenv(name, value)
    assert _call() == EINVAL
    assert name.encode() in _lib.load().plm_last_error()
    v = _valid()
    with pytest.raises(_lib.PlmError) as err:
        plm.cross_energies(v["jab"], v["a"], v["b"])
    assert err.value.code == EINVAL and name in str(err.value)


def test_a_good_plan_hook_passes_the_validation(monkeypatch):
    monkeypatch.setenv("PLM_CROSS_TILE", "1")
    monkeypatch.setenv("PLM_CROSS_VCHUNK", "7")
    assert _call() == (EDEVICE if _lib.load().plm_device_count() <= 0 else OK)


def _assign(scores, ao, bo, maximize=1, partner=True, totals=True):
    lib = _lib.load()
    p = plm._ptr
    scores = None if scores is None else np.ascontiguousarray(scores, np.float64)
    ao, bo = (None if o is None else np.asarray(o, np.int64) for o in (ao, bo))
    n_groups = (len(ao) if ao is not None else len(bo)) - 1
    out, tot = np.zeros(64, np.int64), np.zeros(16)
    return lib.plm_group_assignment(p(scores), n_groups, p(ao), p(bo), maximize, p(out) if partner else None,
                                    p(tot) if totals else None)


def test_assignment_validation():
    E = np.arange(6.0)
    assert _assign(E, [0, 2], [0, 3]) == OK and _assign(E, [0, 2], [0, 3], totals=False) == OK
    assert _assign(None, [0, 2], [0, 3]) == EINVAL and _assign(E, None, [0, 3]) == EINVAL and _assign(E, [0, 2], None) == EINVAL
    assert _assign(E, [0, 2], [0, 3], partner=False) == EINVAL
    assert _assign(E, [1, 2], [0, 3]) == EINVAL and _assign(E, [0, 2, 1], [0, 3, 3]) == EINVAL
    assert _assign(E, [0, 2, 2], [0, 3, 1]) == EINVAL and _assign(E, [0, 2], [-1, 2]) == EINVAL
    assert _lib.load().plm_group_assignment(None, -1, None, None, 1, None, None) == EINVAL
    for bad in (np.nan, np.inf, -np.inf):
        F = E.copy()
        F[4] = bad
        assert _assign(F, [0, 2], [0, 3]) == EINVAL and b"scores[4]" in _lib.load().plm_last_error()
        with pytest.raises(_lib.PlmError):
            plm.group_assignment(F, [0, 2], [0, 3])
    assert _assign(None, [0, 0], [0, 0]) == OK and _assign(None, [0], [0]) == OK   # nothing to assign
    with pytest.raises(ValueError):
        plm.group_assignment(E, [0, 2], [0, 2])


# ---- inter_blocks ------------------------------------------------------------------------------------------------

def _dense(jij, L, q):
    J = np.zeros((L, L, q, q), np.float32)
    iu, ju = np.triu_indices(L, 1)
    J[iu, ju], J[ju, iu] = jij, jij.transpose(0, 2, 1)
    return J


@pytest.mark.parametrize("sites_a,sites_b", [([0, 1, 2], [3, 4, 5, 6]), ([0, 2, 4, 6], [1, 3, 5]), ([6, 5, 4], [2, 1, 0]),
                                             ([3], [0, 6, 1]), ([5, 0, 3], [4, 2])])
def test_inter_blocks_against_the_dense_array(sites_a, sites_b):
    L, q = 7, 5
    rng = np.random.default_rng(2)
    jij = rng.normal(size=(L * (L - 1) // 2, q, q)).astype(np.float32)
    J = _dense(jij, L, q)
    sel_a, sel_b = np.eye(L)[sites_a], np.eye(L)[sites_b]
    want = np.einsum("ki,lj,ijab->klab", sel_a, sel_b, J.astype(np.float64))
    got = plm.inter_blocks(jij, L, q, sites_a, sites_b, gauge=None)
    assert got.dtype == np.float32 and got.shape == (len(sites_a), len(sites_b), q, q) and got.flags["C_CONTIGUOUS"]
    assert np.array_equal(got, want.astype(np.float32))
    row = np.einsum("klab->kla", want)[..., None] / q
    col = np.einsum("klab->klb", want)[:, :, None, :] / q
    zs = want - row - col + np.einsum("klab->kl", want)[..., None, None] / (q * q)
    got = plm.inter_blocks(jij, L, q, sites_a, sites_b)
    assert np.abs(got - zs).max() <= 2.0 ** -22 * np.abs(zs).max()             # one float32 rounding of float64 values
    assert np.abs(got.astype(np.float64).sum(axis=2)).max() < 1e-5 and np.abs(got.astype(np.float64).sum(axis=3)).max() < 1e-5


def test_inter_blocks_refuses_bad_site_lists():
    jij = np.zeros((6, 3, 3), np.float32)
    for sa, sb in (([0, 1], [1, 2]), ([0, 0], [1]), ([0], [4]), ([-1], [1]), ([], [1]), ([0], [])):
        with pytest.raises(ValueError):
            plm.inter_blocks(jij, 4, 3, sa, sb)
    with pytest.raises(ValueError):
        plm.inter_blocks(jij, 4, 3, [0], [1], gauge="lattice")
    with pytest.raises(ValueError):
        plm.inter_blocks(jij[:5], 4, 3, [0], [1])


# ---- the twin ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1, 2), (5, 7, 21), (13, 40, 21), (9, 4, 32)])
@pytest.mark.parametrize("skip", [None, 0])
def test_the_twin_against_einsum_on_one_hot_arrays(shape, skip):
    LA, LB, q = shape
    rng = np.random.default_rng(3)
    jab = rng.normal(size=(LA, LB, q, q)).astype(np.float32)
    a, b = rng.integers(0, q, (12, LA)).astype(np.int8), rng.integers(0, q, (17, LB)).astype(np.int8)
    oa, ob = np.eye(q)[a], np.eye(q)[b]
    if skip is not None:
        oa[..., skip] = 0.0
        ob[..., skip] = 0.0
    want = np.einsum("sia,ijab,tjb->st", oa, jab.astype(np.float64), ob, optimize=True)
    got = tw.table(jab, a, b, skip)
    bound = tw.bound(LA * LB, tw.sum_abs(jab, a, b))
    print("largest |twin - einsum| %.3g, smallest bound %.3g" % (np.abs(got - want).max(), bound.min()))
    assert (np.abs(got - want) <= bound).all()
    full = tw.cross_energies(jab, a, b, skip_state=skip)
    assert np.array_equal(full["matrix"].reshape(12, 17), got)
    k = np.argmax(got, axis=1)
    assert np.array_equal(full["rows_best"]["index"], k) and np.array_equal(full["rows_best"]["best"], got.max(axis=1))
    assert np.array_equal(full["rows_best"]["second"], np.sort(got, axis=1)[:, -2])
    assert np.array_equal(full["cols_best"]["index"], np.argmax(got, axis=0))
    assert np.array_equal(full["cols_best"]["second"], np.sort(got, axis=0)[-2])


def test_the_twin_by_groups_and_its_conventions():
    rng = np.random.default_rng(4)
    jab = rng.integers(-1, 2, (2, 3, 2, 2)).astype(np.float32)                 # many exact ties
    a, b = rng.integers(0, 2, (6, 2)).astype(np.int8), rng.integers(0, 2, (7, 3)).astype(np.int8)
    ao, bo = [0, 0, 2, 3, 6, 6], [0, 2, 2, 3, 7, 7]
    res = tw.cross_energies(jab, a, b, ao, bo)
    E = tw.table(jab, a, b)
    assert res["block_offsets"].tolist() == [0, 0, 0, 1, 13, 13]
    assert res["matrix"][0] == E[2, 2] and np.array_equal(res["matrix"][1:].reshape(3, 4), E[3:6, 3:7])
    none = (-1, -np.inf, -np.inf)
    assert [tuple(r) for r in res["rows_best"][:2]] == [none, none] and [tuple(r) for r in res["cols_best"][:2]] == [none, none]
    assert tuple(res["rows_best"][2]) == (2, E[2, 2], -np.inf) and tuple(res["cols_best"][2]) == (2, E[2, 2], -np.inf)
    for s in range(3, 6):
        row = E[s, 3:7]
        first = 3 + int(np.nonzero(row == row.max())[0][0])
        assert res["rows_best"][s]["index"] == first and res["rows_best"][s]["second"] == np.sort(row)[-2]


# ---- the assignment ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("maximize", [True, False])
@pytest.mark.parametrize("shape", [(1, 1), (1, 5), (5, 1), (7, 7), (40, 23), (23, 40)])
def test_assignment_against_scipy(shape, maximize):
    from scipy.optimize import linear_sum_assignment
    n, m = shape
    E = np.random.default_rng(10 * n + m).normal(size=(n, m))
    partner, totals = plm.group_assignment(E, [0, n], [0, m], maximize=maximize)
    r, c = linear_sum_assignment(E, maximize=maximize)
    want = np.full(n, -1, np.int64)
    want[r] = c
    assert np.array_equal(partner, want) and (partner >= 0).sum() == min(n, m)
    assert totals[0] == pytest.approx(E[r, c].sum(), rel=1e-13)


@pytest.mark.parametrize("maximize", [True, False])
def test_assignment_in_batches_with_empty_groups(maximize):
    from scipy.optimize import linear_sum_assignment
    rng = np.random.default_rng(5)
    na = np.array([0, 3, 0, 5, 2, 0, 7, 4, 0])
    nb = np.array([2, 0, 0, 5, 6, 0, 3, 4, 1])
    ao, bo = np.concatenate([[0], np.cumsum(na)]), np.concatenate([[0], np.cumsum(nb)])
    blocks = [rng.normal(size=(x, y)) for x, y in zip(na, nb)]
    partner, totals = plm.group_assignment(np.concatenate([b.ravel() for b in blocks]), ao, bo, maximize=maximize)
    for g, E in enumerate(blocks):
        want = np.full(na[g], -1, np.int64)
        total = 0.0
        if E.size:
            r, c = linear_sum_assignment(E, maximize=maximize)
            want[r] = c + bo[g]
            total = E[r, c].sum()
        assert np.array_equal(partner[ao[g]:ao[g + 1]], want), g
        assert totals[g] == pytest.approx(total, rel=1e-13, abs=0.0)


@pytest.mark.parametrize("maximize", [True, False])
def test_assignment_against_brute_force(maximize):
    rng = np.random.default_rng(6)
    for n in range(1, 7):
        for m in range(1, 7):
            E = rng.normal(size=(n, m))
            partner, totals = plm.group_assignment(E, [0, n], [0, m], maximize=maximize)
            want, total = tw.brute_assignment(E, maximize)
            assert np.array_equal(partner, want), (n, m)
            assert totals[0] == pytest.approx(total, rel=1e-13)


# ---- match_by_species on the twin -----------------------------------------------------------------------------------

def _match(c, method, **kw):
    args = dict(ids_a=c["ids_a"], ids_b=c["ids_b"], sites_a=c["sites_a"], sites_b=c["sites_b"], gauge=None)
    args.update(kw)
    return complex_accel.match_by_species(c["model"], c["a"], c["b"], c["species_a"], c["species_b"], method=method, **args)


@pytest.mark.parametrize("method", ["assignment", "reciprocal_best"])
@pytest.mark.parametrize("seed", range(5))
def test_the_planted_pairs_are_all_recovered(monkeypatch, seed, method):
    monkeypatch.setattr(plm, "cross_energies", tw.cross_energies)
    c = tw.planted_case(seed)
    assert c["jab"].shape == (8, 6, 21, 21) and len(c["a"]) == 60 and not np.array_equal(c["ids_b"], np.sort(c["ids_b"]))
    out = _match(c, method)
    assert list(out.columns) == ["id_1", "id_2", "species", "energy", "gap"] and len(out) == 60
    assert all(c["truth"][i] == j for i, j in zip(out["id_1"], out["id_2"]))
    assert (out["gap"] > 0).all() and out["species"].tolist() == sorted(out["species"].tolist())
    E = tw.table(c["jab"], c["a"], c["b"])
    for _, r in out.iterrows():
        s, t = int(np.nonzero(c["ids_a"] == r["id_1"])[0][0]), int(np.nonzero(c["ids_b"] == r["id_2"])[0][0])
        same = c["species_b"] == c["species_a"][s]
        alt = max(np.delete(E[s][same], np.nonzero(np.nonzero(same)[0] == t)[0]).max(),
                  np.delete(E[:, t][c["species_a"] == c["species_b"][t]], s % 5).max())
        assert r["energy"] == E[s, t] and r["gap"] == E[s, t] - alt
    # the same pairs whatever the gauge of the inter block (an assignment does not see terms of one row alone)
    if method == "assignment":
        again = _match(c, method, gauge="zero_sum")
        assert again["id_2"].tolist() == out["id_2"].tolist()


def test_a_model_with_segments_and_letters(monkeypatch):
    monkeypatch.setattr(plm, "cross_energies", tw.cross_energies)
    c = tw.planted_case(1)
    m = c["model"]
    alphabet = np.array(list(m["alphabet"]))
    index = [("B_1", k + 1) for k in range(8, 14)]                              # the sites of B first in the model
    index = [("A_1", k + 1) for k in range(8)] + index
    model = SimpleNamespace(J_ij=_dense(m["jij"], 14, 21), index_list=index, alphabet=alphabet)
    letters_a, letters_b = alphabet[c["a"]], ["".join(r) for r in alphabet[c["b"]]]
    want = _match(c, "assignment")
    got = complex_accel.match_by_species(model, letters_a, letters_b, c["species_a"], c["species_b"], ids_a=c["ids_a"],
                                         ids_b=c["ids_b"], gauge=None)
    assert got.equals(want)
    got = complex_accel.match_by_species(model, letters_a, letters_b, c["species_a"], c["species_b"], ids_a=c["ids_a"],
                                         ids_b=c["ids_b"], segment_a="A_1", segment_b="B_1", gauge=None)
    assert got.equals(want)
    swapped = complex_accel.interaction_energies(model, c["b"][:3], c["a"][:4], segment_a="B_1", segment_b="A_1", gauge=None)
    assert np.array_equal(swapped["matrix"].reshape(3, 4), tw.table(c["jab"], c["a"][:4], c["b"][:3]).T)
    with pytest.raises(ValueError):
        complex_accel.interaction_energies(model, c["a"], c["b"], segment_a="C_1")
    with pytest.raises(ValueError):
        complex_accel.interaction_energies(m, c["a"], c["b"])                   # a plain model has no segments
    with pytest.raises(ValueError):
        complex_accel.interaction_energies(model, letters_a[:, :7], letters_b)
    with pytest.raises(ValueError):
        complex_accel.interaction_energies(model, [["X"] * 8], letters_b)
    with pytest.raises(ValueError):
        complex_accel.match_by_species(model, letters_a, letters_b, c["species_a"], c["species_b"], method="greedy")
    gap = complex_accel.interaction_energies(m, c["a"], c["b"], sites_a=c["sites_a"], sites_b=c["sites_b"], gauge=None,
                                             skip_gap=True)
    assert np.array_equal(gap["matrix"].reshape(60, 60), tw.table(c["jab"], c["a"], c["b"], skip_state=0))


def test_species_on_one_side_unequal_counts_and_min_gap(monkeypatch):
    monkeypatch.setattr(plm, "cross_energies", tw.cross_energies)
    c = tw.planted_case(2)
    # species sp03 only in A, sp07 only in B; sp05 loses two of its B rows, sp09 three of its A rows
    keep_a = ~((c["species_a"] == "sp07") | np.isin(c["ids_a"], ["a045", "a047", "a049"]))
    keep_b = ~((c["species_b"] == "sp03") | np.isin(c["ids_b"], ["b026", "b028"]))
    d = dict(c, a=c["a"][keep_a], b=c["b"][keep_b], species_a=c["species_a"][keep_a], species_b=c["species_b"][keep_b],
             ids_a=c["ids_a"][keep_a], ids_b=c["ids_b"][keep_b])
    out = _match(d, "assignment")
    assert set(out["species"]) == {"sp%02d" % k for k in range(12)} - {"sp03", "sp07"}
    counts = out["species"].value_counts()
    assert counts["sp05"] == 3 and counts["sp09"] == 2 and len(out) == 8 * 5 + 3 + 2
    # the rows whose true partner is still there get it (margins of 18 and more against 60 terms of noise)
    present = set(d["ids_b"])
    both = [(i, j) for i, j in zip(out["id_1"], out["id_2"]) if c["truth"][i] in present]
    assert all(c["truth"][i] == j for i, j in both if i not in ("a025", "a026", "a027", "a028", "a029")) and len(both) >= 43
    recip = _match(d, "reciprocal_best")
    assert set(zip(recip["id_1"], recip["id_2"])) <= {(i, c["truth"][i]) for i in d["ids_a"]} | set(zip(out["id_1"], out["id_2"]))
    # min_gap keeps the rows at or above it, in order
    cut = float(np.sort(out["gap"].to_numpy())[len(out) // 2])
    kept = _match(d, "assignment", min_gap=cut)
    assert kept.equals(out[out["gap"] >= cut].reset_index(drop=True)) and 0 < len(kept) < len(out)
    # no common species at all
    empty = complex_accel.match_by_species(c["model"], c["a"][:5], c["b"][:5], ["x"] * 5, ["y"] * 5, sites_a=c["sites_a"],
                                           sites_b=c["sites_b"])
    assert list(empty.columns) == ["id_1", "id_2", "species", "energy", "gap"] and len(empty) == 0
    # a single sequence per species on each side: no alternative, the gap is +inf
    one = complex_accel.match_by_species(c["model"], c["a"][::5], c["b"][::5], c["species_a"][::5], c["species_b"][::5],
                                         sites_a=c["sites_a"], sites_b=c["sites_b"])
    assert len(one) == 12 and np.isposinf(one["gap"]).all()


# ---- the command line --------------------------------------------------------------------------------------------

def _write_case(tmp_path, c, insert_columns=False):
    m = c["model"]
    alphabet = np.array(list(m["alphabet"]))
    L, q = m["L"], m["q"]
    npair = L * (L - 1) // 2
    path = str(tmp_path / "pair.model")
    model_io.write_model_file(path, L, q, 1, 0, 1, 0.2, 0.01, 0.01, 0.0, 1.0, m["alphabet"], np.ones(1, np.float32), "A" * L,
                              m["index_list"], np.full((L, q), 1.0 / q), m["hi"], np.zeros((npair, q, q)), m["jij"])

    def a2m(name, ids, states):
        with open(str(tmp_path / name), "w") as f:
            for i, row in zip(ids, alphabet[states]):
                seq = "".join(row)
                if insert_columns:
                    seq = seq[:2] + ("kl" if i == ids[0] else "..") + seq[2:]
                f.write(">%s/1-%d\n%s\n" % (i, len(row), seq))
        return str(tmp_path / name)

    def species(name, ids, labels, header):
        with open(str(tmp_path / name), "w") as f:
            if header:
                f.write("id,species\n")
            for i, s in zip(ids, labels):
                f.write("%s/1-%d,%s\n" % (i, 8 if name[0] == "A" else 6, s))
        return str(tmp_path / name)

    ids_a = ["%s/1-8" % i for i in c["ids_a"]]
    ids_b = ["%s/1-6" % i for i in c["ids_b"]]
    return (path, a2m("A.a2m", c["ids_a"], c["a"]), a2m("B.a2m", c["ids_b"], c["b"]),
            species("A.csv", c["ids_a"], c["species_a"], True), species("B.csv", c["ids_b"], c["species_b"], False), ids_a, ids_b)


@pytest.mark.parametrize("argv", [
    ["m", "a", "b"],                                            # no -o
    ["m", "a", "b", "-o", "x"],                                 # neither species files nor --all-against-all
    ["m", "a", "b", "-o", "x", "--species-a", "s"],
    ["m", "a", "b", "-o", "x", "--all-against-all", "--species-a", "s"],
    ["m", "a", "b", "-o", "x", "--all-against-all", "--min-gap", "1"],
    ["m", "a", "b", "-o", "x", "--species-a", "s", "--species-b", "t", "--method", "greedy"],
    ["m", "a", "b", "-o", "x", "--species-a", "s", "--species-b", "t", "--min-gap", "nan"],
])
def test_arguments_that_are_refused(argv, capsys):
    with pytest.raises(SystemExit) as e:
        pairing.parse_args(argv)
    assert e.value.code == 2
    capsys.readouterr()


def _run_command_line(tmp_path, insert_columns=False):
    import pandas as pd
    c = tw.planted_case(3)
    model, fa, fb, sa, sb, ids_a, ids_b = _write_case(tmp_path, c, insert_columns)
    out = str(tmp_path / "pairs.csv")
    truth = {"%s/1-8" % i: "%s/1-6" % j for i, j in c["truth"].items()}
    for method in ("assignment", "reciprocal_best"):
        assert pairing.main([model, fa, fb, "--species-a", sa, "--species-b", sb, "--method", method, "--gauge", "none",
                             "-o", out]) == 0
        got = pd.read_csv(out)
        assert list(got.columns) == ["id_1", "id_2", "species", "energy", "gap"] and len(got) == 60
        assert all(truth[i] == j for i, j in zip(got["id_1"], got["id_2"])) and (got["gap"] > 0).all()
    cut = float(np.sort(got["gap"].to_numpy())[30])
    assert pairing.main([model, fa, fb, "--species-a", sa, "--species-b", sb, "--min-gap", repr(cut), "--gauge", "none",
                         "-o", out]) == 0
    assert len(pd.read_csv(out)) == 30
    assert pairing.main([model, fa, fb, "--species-a", sa, "--species-b", sb, "--skip-gap", "-o", out]) == 0
    assert len(pd.read_csv(out)) == 60
    table = str(tmp_path / "table.csv")
    assert pairing.main([model, fa, fb, "--all-against-all", "--gauge", "none", "-o", table]) == 0
    best = pd.read_csv(table, float_precision="round_trip")
    assert list(best.columns) == ["id_1", "id_2", "energy", "second", "reciprocal"] and len(best) == 60
    E = tw.table(c["jab"], c["a"], c["b"])
    assert best["id_2"].tolist() == [ids_b[k] for k in np.argmax(E, axis=1)]
    assert np.array_equal(best["energy"].to_numpy(), E.max(axis=1)) and np.array_equal(best["second"].to_numpy(), np.sort(E, axis=1)[:, -2])
    assert best["reciprocal"].tolist() == [int(np.argmax(E[:, t]) == s) for s, t in enumerate(np.argmax(E, axis=1))]
    return model, fa, fb, out, got


def test_command_line_on_the_twin(monkeypatch, tmp_path):
    monkeypatch.setattr(plm, "cross_energies", tw.cross_energies)
    _run_command_line(tmp_path)


def test_command_line_reduces_an_alignment_to_its_match_columns(monkeypatch, tmp_path):
    monkeypatch.setattr(plm, "cross_energies", tw.cross_energies)
    _run_command_line(tmp_path, insert_columns=True)


def test_command_line_refuses_alignments_that_do_not_fit_the_model(monkeypatch, tmp_path):
    monkeypatch.setattr(plm, "cross_energies", tw.cross_energies)
    c = tw.planted_case(3)
    model, fa, fb, sa, sb, _, _ = _write_case(tmp_path, c)
    with pytest.raises(SystemExit) as e:
        pairing.main([model, fa, fa, "--species-a", sa, "--species-b", sb, "-o", str(tmp_path / "x.csv")])
    assert "sites on this side" in str(e.value)


def test_the_pairs_pass_through_the_reference_concatenation(monkeypatch, tmp_path):
    """id_1 / id_2 of the pairing table are what the reference's write_concatenated_alignment(id_pairing, ...) takes"""
    import refstubs
    if not refstubs.reference_available():
        pytest.skip("reference tree not present")
    refstubs.install()
    from evcouplings.complex.alignment import write_concatenated_alignment
    import pandas as pd
    monkeypatch.setattr(plm, "cross_energies", tw.cross_energies)
    model, fa, fb, out, _ = _run_command_line(tmp_path)
    pairs = pd.read_csv(out)
    target_header, target_index, full, mono_1, mono_2 = write_concatenated_alignment(pairs, fa, fb, pairs["id_1"][0],
                                                                                    pairs["id_2"][0])
    assert target_index == 0 and full.matrix.shape == (61, 14) and mono_1.matrix.shape == (61, 8)
    assert mono_2.matrix.shape == (61, 6)
    c = tw.planted_case(3)
    alphabet = np.array(list(c["model"]["alphabet"]))
    row = {i: k for k, i in enumerate(c["ids_a"])}
    rowb = {i: k for k, i in enumerate(c["ids_b"])}
    for k, (i, j) in enumerate(zip(pairs["id_1"], pairs["id_2"])):
        want = "".join(alphabet[c["a"][row[i.split("/")[0]]]]) + "".join(alphabet[c["b"][rowb[j.split("/")[0]]]])
        assert "".join(full.matrix[k + 1]) == want


@pytest.mark.gpu
def test_command_line_on_the_gpu(tmp_path):
    _run_command_line(tmp_path)
