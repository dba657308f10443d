"""plm_cross_energies on the GPU (DESIGN_NEXT_ROWS.md section 9.23) against the numpy twin tests/cross_twin.py.  The
contract fixes the order of every sum, so every comparison is on the bits of the float64 values and on the best-partner
arrays as they are -- indices, best and second, the -inf and -1 conventions included; no tolerance applies, except
against plm.hamiltonians, which works in float32 products."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cross_twin as tw  # noqa: E402
from evcouplings_amd import _lib, complex_accel, plm  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 2), (2, 3, 2), (5, 7, 21), (13, 150, 21), (33, 31, 32), (65, 17, 4)]


def _small_groups():
    """200 groups of 0..5 rows per side; empty on one or both sides at the start, in the middle and at the end"""
    rng = np.random.default_rng(200)
    na, nb = rng.integers(0, 6, 200), rng.integers(0, 6, 200)
    for g, (x, y) in {0: (0, 3), 1: (2, 0), 2: (0, 0), 100: (0, 0), 101: (0, 4), 102: (3, 0), 197: (0, 2), 198: (3, 0),
                      199: (0, 0)}.items():
        na[g], nb[g] = x, y
    return np.concatenate([[0], np.cumsum(na)]), np.concatenate([[0], np.cumsum(nb)])


STRUCTURES = {
    "1x1": ([0, 1], [0, 1]),
    "1xn": ([0, 1], [0, 37]),
    "nx1": ([0, 37], [0, 1]),
    "130x70+70x130": ([0, 130, 200], [0, 70, 200]),
    "200 small groups": _small_groups(),
}


def _case(shape, structure, seed=0, integers=False):
    LA, LB, q = shape
    ao, bo = (np.asarray(o, np.int64) for o in STRUCTURES[structure])
    rng = np.random.default_rng(seed + 1000 * LA + LB)
    if integers:
        jab = rng.integers(-1, 2, (LA, LB, q, q)).astype(np.float32)
    else:
        jab = rng.normal(size=(LA, LB, q, q)).astype(np.float32)
    a = rng.integers(0, q, (int(ao[-1]), LA)).astype(np.int8)
    b = rng.integers(0, q, (int(bo[-1]), LB)).astype(np.int8)
    return jab, a, b, ao, bo


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _assert_same(got, want, what):
    assert np.array_equal(got["block_offsets"], want["block_offsets"]), what
    if want["matrix"] is not None:
        assert np.array_equal(_bits(got["matrix"]), _bits(want["matrix"])), what + ": matrix"
    for key in ("rows_best", "cols_best"):
        if want[key] is None:
            assert got[key] is None
            continue
        assert np.array_equal(got[key]["index"], want[key]["index"]), "%s: %s index" % (what, key)
        assert np.array_equal(_bits(got[key]["best"]), _bits(want[key]["best"])), "%s: %s best" % (what, key)
        assert np.array_equal(_bits(got[key]["second"]), _bits(want[key]["second"])), "%s: %s second" % (what, key)


@pytest.mark.parametrize("structure", list(STRUCTURES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dq%d" % s)
def test_every_shape_and_group_structure_equals_the_twin(shape, structure):
    jab, a, b, ao, bo = _case(shape, structure)
    _assert_same(plm.cross_energies(jab, a, b, ao, bo), tw.cross_energies(jab, a, b, ao, bo), structure)


def test_no_groups_is_ok_and_writes_nothing():
    """n_groups = 0 with n_a = n_b = 0: PLM_OK (documented in include/plm_hip.h), empty outputs"""
    jab = np.ones((2, 3, 4, 4), np.float32)
    got = plm.cross_energies(jab, np.zeros((0, 2), np.int8), np.zeros((0, 3), np.int8), [0], [0])
    assert got["matrix"].size == 0 and got["rows_best"].size == 0 and got["cols_best"].size == 0
    assert got["block_offsets"].tolist() == [0]


@pytest.mark.parametrize("structure", list(STRUCTURES))
def test_the_forced_plans_change_no_bit(monkeypatch, structure):
    jab, a, b, ao, bo = _case((5, 7, 21), structure, seed=3)
    want = tw.cross_energies(jab, a, b, ao, bo)
    for tile in ("1", "7", "128", "1000"):
        monkeypatch.setenv("PLM_CROSS_TILE", tile)
        _assert_same(plm.cross_energies(jab, a, b, ao, bo), want, "PLM_CROSS_TILE=" + tile)
    for chunk in ("1", "2"):                                   # V in chunks of one and two tiles of 64 b-rows
        monkeypatch.setenv("PLM_CROSS_VCHUNK", chunk)
        _assert_same(plm.cross_energies(jab, a, b, ao, bo), want, "PLM_CROSS_TILE=1000 PLM_CROSS_VCHUNK=" + chunk)
    monkeypatch.delenv("PLM_CROSS_TILE")
    _assert_same(plm.cross_energies(jab, a, b, ao, bo), want, "PLM_CROSS_VCHUNK=2")
    monkeypatch.delenv("PLM_CROSS_VCHUNK")
    _assert_same(plm.cross_energies(jab, a, b, ao, bo), want, "unforced")


def test_forced_plans_at_a_shape_with_several_site_chunks(monkeypatch):
    """(65, 17, 4) and (33, 31, 32) take several LDS chunks of sites; a-ranges cut at 1, 16 and 129 rows"""
    for shape in ((65, 17, 4), (33, 31, 32)):
        jab, a, b, ao, bo = _case(shape, "130x70+70x130", seed=5)
        want = tw.cross_energies(jab, a, b, ao, bo)
        for tile, chunk in (("1", "1"), ("16", "3"), ("129", "1")):
            monkeypatch.setenv("PLM_CROSS_TILE", tile)
            monkeypatch.setenv("PLM_CROSS_VCHUNK", chunk)
            _assert_same(plm.cross_energies(jab, a, b, ao, bo), want, "%r tile %s chunk %s" % (shape, tile, chunk))


@pytest.mark.parametrize("skip", [0, 9, 20])
def test_a_skipped_state_equals_the_twin_and_zeroed_couplings(skip):
    jab, a, b, ao, bo = _case((5, 7, 21), "200 small groups", seed=7)
    got = plm.cross_energies(jab, a, b, ao, bo, skip_state=skip)
    _assert_same(got, tw.cross_energies(jab, a, b, ao, bo, skip_state=skip), "skip %d" % skip)
    zeroed = jab.copy()
    zeroed[:, :, skip, :] = 0.0
    zeroed[:, :, :, skip] = 0.0
    _assert_same(got, plm.cross_energies(zeroed, a, b, ao, bo), "skip %d against zeroed rows and columns" % skip)


def test_outputs_can_be_left_out_and_calls_repeat_to_the_byte():
    jab, a, b, ao, bo = _case((13, 150, 21), "130x70+70x130", seed=9)
    both = plm.cross_energies(jab, a, b, ao, bo)
    again = plm.cross_energies(jab, a, b, ao, bo)
    assert both["matrix"].tobytes() == again["matrix"].tobytes()
    assert both["rows_best"].tobytes() == again["rows_best"].tobytes()
    assert both["cols_best"].tobytes() == again["cols_best"].tobytes()
    only_best = plm.cross_energies(jab, a, b, ao, bo, matrix=False)
    assert only_best["matrix"] is None
    assert only_best["rows_best"].tobytes() == both["rows_best"].tobytes()
    assert only_best["cols_best"].tobytes() == both["cols_best"].tobytes()
    only_matrix = plm.cross_energies(jab, a, b, ao, bo, best=False)
    assert only_matrix["rows_best"] is None and only_matrix["cols_best"] is None
    assert only_matrix["matrix"].tobytes() == both["matrix"].tobytes()
    # one best array alone, through the C ABI
    lib = _lib.load()
    import ctypes as C
    rows = np.empty(len(a), plm.CROSS_BEST)
    opts = _lib.PlmCrossOpts(-1, 1)
    p = plm._ptr
    _lib.check(lib.plm_cross_energies(p(jab), 13, 150, 21, p(a), len(a), p(b), len(b), 2, p(ao), p(bo), C.byref(opts), 0, None,
                                      None, p(rows), None))
    assert rows.tobytes() == both["rows_best"].tobytes()


@pytest.mark.parametrize("structure", ["130x70+70x130", "200 small groups", "1xn", "nx1"])
def test_ties_go_to_the_smallest_index(structure):
    jab, a, b, ao, bo = _case((2, 3, 2), structure, seed=11, integers=True)
    want = tw.cross_energies(jab, a, b, ao, bo)
    tied = sum(int((np.diff(np.sort(want["matrix"][lo:hi])) == 0).any())
               for lo, hi in zip(want["block_offsets"][:-1], want["block_offsets"][1:]))
    assert tied >= 1                                           # energies do coincide
    _assert_same(plm.cross_energies(jab, a, b, ao, bo), want, "ties")


def test_zero_couplings_give_plus_zero_and_the_first_partner():
    jab, a, b, ao, bo = _case((5, 7, 21), "130x70+70x130")
    got = plm.cross_energies(np.zeros_like(jab), a, b, ao, bo)
    assert not _bits(got["matrix"]).any()                      # +0.0 everywhere, not -0.0
    assert got["rows_best"]["index"].tolist() == [0] * 130 + [70] * 70
    assert got["cols_best"]["index"].tolist() == [0] * 70 + [130] * 130
    assert not _bits(got["rows_best"]["best"]).any() and not _bits(got["rows_best"]["second"]).any()


def test_against_hamiltonians_of_the_concatenated_rows():
    """E(s,t) = H_J(concat) - H_J(A part under the A-A blocks) - H_J(B part under the B-B blocks)"""
    LA, LB, q = 5, 7, 21
    L = LA + LB
    rng = np.random.default_rng(13)
    jij = rng.normal(size=(L * (L - 1) // 2, q, q)).astype(np.float32)
    a = rng.integers(0, q, (11, LA)).astype(np.int8)
    b = rng.integers(0, q, (9, LB)).astype(np.int8)
    jab = plm.inter_blocks(jij, L, q, np.arange(LA), np.arange(LA, L), gauge=None)
    E = plm.cross_energies(jab, a, b)["matrix"].reshape(11, 9)
    pair = lambda i, j: i * (2 * L - i - 1) // 2 + (j - i - 1)
    jaa = np.array([jij[pair(i, j)] for i in range(LA) for j in range(i + 1, LA)])
    jbb = np.array([jij[pair(i, j)] for i in range(LA, L) for j in range(i + 1, L)])
    concat = np.concatenate([np.repeat(a, 9, axis=0), np.tile(b, (11, 1))], axis=1)
    H = plm.hamiltonians(concat, q, np.zeros((L, q), np.float32), jij)[:, 1].reshape(11, 9)
    HA = plm.hamiltonians(a, q, np.zeros((LA, q), np.float32), jaa)[:, 1]
    HB = plm.hamiltonians(b, q, np.zeros((LB, q), np.float32), jbb)[:, 1]
    # plm_hamiltonians works in float32 products: tests/test_gpu_parity.py holds it to rtol 2e-5 and atol 2e-5 max|H|
    # against float64; the bound expression of tests/test_gpu_mutants.py for a difference of such energies
    tol = 2 * 2e-5 * max(np.abs(H).max(), np.abs(HA).max(), np.abs(HB).max())
    np.testing.assert_allclose(E, H - HA[:, None] - HB[None, :], rtol=2e-5, atol=tol)


@pytest.mark.parametrize("method", ["assignment", "reciprocal_best"])
def test_the_planted_pairs_end_to_end(monkeypatch, method):
    import pandas as pd
    c = tw.planted_case(0)
    run = lambda: complex_accel.match_by_species(c["model"], c["a"], c["b"], c["species_a"], c["species_b"], method=method,
                                                 ids_a=c["ids_a"], ids_b=c["ids_b"], sites_a=c["sites_a"],
                                                 sites_b=c["sites_b"], gauge=None)
    got = run()
    monkeypatch.setattr(plm, "cross_energies", tw.cross_energies)
    want = run()
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    assert len(got) == 60 and all(c["truth"][i] == j for i, j in zip(got["id_1"], got["id_2"])) and (got["gap"] > 0).all()
