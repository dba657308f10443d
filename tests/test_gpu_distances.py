"""
Residue distance maps on the GPU (plm_residue_distances, plm_distance_maps_aggregate) against the numpy twin of
tests/distance_twin.py: equal bit for bit -- np.array_equal on the doubles, NaN in the same cells.  The contract
(include/plm_hip.h) fixes the order of every operation of a squared distance, and a minimum has no order, so there is
no tolerance to choose.  Only the comparisons with the recorded reference results allow 2 ulp: the reference sums the
three squares with np.sum (tests/test_distance_host.py states the bound).

Sizes: 1, 15, 16, 17, 33 and 65 residues sit below, at and above one and two default tiles of 16 and reach five tiles
a side; 70 atoms pass the default staging chunk of 16 five times, 300 atoms pass every chunk length the plan allows.
"""
import functools
import os
import types

import numpy as np
import pandas as pd
import pytest

import distance_twin as twin
from evcouplings_amd import _lib, plm, structure_accel as sa

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 17), (15, 16), (16, 15), (17, 33), (33, 65), (65, 1), (65, 65)]
ATOMS = ["ca", "mixed", "one70", "one300"]
RANGES = ["adjacent", "overlap", "gaps", "empty"]
COORDS = ["decimal", "double"]


def make_chain(seed, n, atoms="mixed", ranges="adjacent", coords="decimal"):
    """(xyz (A, 3), ranges (n, 2) int32) of a random chain"""
    rng = np.random.default_rng(seed)
    counts = np.ones(n, np.int64) if atoms == "ca" else rng.integers(1, 15, size=n)
    if atoms == "one70":
        counts[rng.integers(n)] = 70
    if atoms == "one300":
        counts[rng.integers(n)] = 300
    gap = 2 if ranges == "gaps" else 0
    first = np.cumsum(counts + gap) - counts - gap + gap // 2          # `gap` unused atoms around every residue
    last = first + counts - 1
    n_atoms = int(last[-1] + 1 + gap)
    if ranges == "overlap":                                            # every residue reaches into its neighbours
        first, last = np.maximum(first - 1, 0), np.minimum(last + 2, n_atoms - 1)
    if ranges == "empty":                                              # one residue without atoms, named oddly
        k = rng.integers(n)
        first[k], last[k] = (5, 2) if k % 2 else (2 ** 31 - 1, -2 ** 31)
    centres = np.cumsum(rng.normal(scale=3.0, size=(n_atoms, 3)), axis=0) * 0.3 + rng.uniform(-9000, 9000, size=3)
    xyz = np.clip(centres + rng.normal(scale=1.5, size=(n_atoms, 3)), -9999.999, 9999.999)
    if coords == "decimal":
        xyz = np.round(xyz, 3)
    return np.ascontiguousarray(xyz), np.stack((first, last)).T.astype(np.int32)


@functools.lru_cache(maxsize=None)
def pair_case(n_i, n_j, atoms, ranges, coords):
    xi, ri = make_chain(1000 + n_i, n_i, atoms, ranges, coords)
    xj, rj = make_chain(2000 + n_j, n_j, atoms, ranges, coords)
    xj = xj - (xj.mean(axis=0) - xi.mean(axis=0))                      # the two chains lie across each other
    if coords == "decimal":
        xj = np.round(xj, 3)
    want = twin.residue_distances(xi, ri, xj, rj)
    want.setflags(write=False)
    return xi, ri, xj, rj, want


def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and \
        np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])


@pytest.mark.parametrize("atoms", ATOMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_two_chains_equal_the_twin_bit_for_bit(shape, atoms):
    k = SHAPES.index(shape) + ATOMS.index(atoms)
    xi, ri, xj, rj, want = pair_case(*shape, atoms, RANGES[k % 4], COORDS[k % 2])
    got = plm.residue_distances(xi, ri, xj, rj)
    assert same_bits(got, want)


@pytest.mark.parametrize("coords", COORDS)
@pytest.mark.parametrize("ranges", RANGES)
def test_every_kind_of_range_and_coordinate(ranges, coords):
    xi, ri, xj, rj, want = pair_case(17, 33, "mixed", ranges, coords)
    got = plm.residue_distances(xi, ri, xj, rj)
    assert same_bits(got, want)
    if ranges == "empty":
        empty_i, empty_j = np.where(ri[:, 1] < ri[:, 0])[0], np.where(rj[:, 1] < rj[:, 0])[0]
        assert len(empty_i) == 1 and len(empty_j) == 1
        assert (got[empty_i[0]] == 1e6).all() and (got[:, empty_j[0]] == 1e6).all()
        assert (np.delete(np.delete(got, empty_i, 0), empty_j, 1) < 1e6).all()


@functools.lru_cache(maxsize=None)
def one_chain_case(n, atoms):
    x, r = make_chain(77 + n, n, atoms, RANGES[n % 4], COORDS[n % 2])
    want = twin.residue_distances(x, r)
    want.setflags(write=False)
    return x, r, want


@pytest.mark.parametrize("atoms", ["mixed", "one300"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33, 65])
def test_the_symmetric_call_is_the_unsymmetric_call_on_one_chain_twice(n, atoms):
    x, r, want = one_chain_case(n, atoms)
    sym = plm.residue_distances(x, r)
    assert same_bits(sym, want)
    assert np.array_equal(sym, plm.residue_distances(x, r, x, r))
    assert np.array_equal(sym, sym.T)
    with_atoms = r[:, 1] >= r[:, 0]
    assert (np.diag(sym)[with_atoms] == 0).all() and (np.diag(sym)[~with_atoms] == 1e6).all()


def test_far_atoms_are_capped_and_equal_atoms_are_at_zero():
    xyz = np.array([[-1e6, 0.25, 0.0], [1e6, 0.25, 0.0], [3.125, -7.5, 11.0], [3.125, -7.5, 11.0], [1e6 - 1.0, 0.25, 0.0],
                    [0.1, 0.2, 0.3]])
    ranges = np.array([[0, 0], [1, 1], [2, 2], [3, 3], [4, 4], [5, 5]], np.int32)
    got = plm.residue_distances(xyz, ranges)
    assert same_bits(got, twin.residue_distances(xyz, ranges))
    assert got[0, 1] == 1e6 and got[1, 0] == 1e6                  # 2e6 apart
    assert got[2, 3] == 0.0 and not np.signbit(got[2, 3])         # the same point in two residues
    assert got[1, 4] == 1.0 and got[0, 4] == 1e6
    # the largest finite coordinates: the squares overflow to +inf, which the cap takes
    huge = np.array([[1.7e308, 0, 0], [-1.7e308, 0, 0]])
    assert np.array_equal(plm.residue_distances(huge, ranges[:2]), [[0.0, 1e6], [1e6, 0.0]])


# ---- aggregation ---------------------------------------------------------------------------------------------------

LENGTHS = [17, 33, 5, 20, 16, 1, 40]
MAPS = {1: [(0, 0)], 2: [(0, 1), (1, 0)], 7: [(0, 0), (1, 1), (2, 2), (0, 1), (1, 0), (6, 3), (0, 0)]}


@functools.lru_cache(maxsize=None)
def chains_case():
    """seven chains of different lengths in one coordinate array; the slot sets overlap in part, some residues have
    no slot, and the last slots of both axes and 0, 1 of axis j belong to nobody"""
    rng = np.random.default_rng(4242)
    xyz, ranges, off = [], [], [0]
    for c, n in enumerate(LENGTHS):
        x, r = make_chain(300 + c, n, ATOMS[c % 4], RANGES[c % 4], COORDS[c % 2])
        x = x - np.round(x.mean(axis=0), 3)            # all chains around the origin: real minima between chains
        ok = r[:, 1] >= r[:, 0]
        r[ok] += sum(len(a) for a in xyz)
        xyz.append(x)
        ranges.append(r)
        off.append(off[-1] + n)
    starts = [0, 10, 30, 25, 41, 7, 3]
    slots_i = np.concatenate([s + np.arange(n) for s, n in zip(starts, LENGTHS)]).astype(np.int32)
    slots_j = (slots_i + 2).astype(np.int32)
    drop = rng.choice(len(slots_i), 9, replace=False)
    slots_i[drop[:5]] = -1
    slots_j[drop[4:]] = -1
    args = (np.concatenate(xyz), np.concatenate(ranges), np.array(off, np.int32), slots_i)
    return args, slots_j, 64, 70


@functools.lru_cache(maxsize=None)
def aggregate_want(S, two_tables):
    args, slots_j, m_i, m_j = chains_case()
    if two_tables:
        agg, count = twin.aggregate_distance_maps(*args, MAPS[S], m_i, slots_j, m_j)
    else:
        agg, count = twin.aggregate_distance_maps(*args, MAPS[S], m_i)
    agg.setflags(write=False)
    count.setflags(write=False)
    return agg, count


@pytest.mark.parametrize("two_tables", [False, True])
@pytest.mark.parametrize("S", [1, 2, 7])
def test_aggregate_equals_the_stacked_twin_bit_for_bit(S, two_tables):
    args, slots_j, m_i, m_j = chains_case()
    want_agg, want_count = aggregate_want(S, two_tables)
    kw = {"slots_j": slots_j, "m_j": m_j} if two_tables else {}
    agg, count = plm.aggregate_distance_maps(*args, MAPS[S], m_i, **kw)
    assert same_bits(agg, want_agg) and count.dtype == np.int32 and np.array_equal(count, want_count)
    assert np.array_equal(np.isnan(agg), count == 0) and (count == 0).any() and (count > 0).any()
    assert count.max() == (1 if S == 1 else 2 if S == 2 else want_count.max()) and want_count.max() <= S
    if S == 2 and not two_tables:            # (a, b) and (b, a) on one slot table: the result is symmetric
        assert np.array_equal(agg, agg.T, equal_nan=True)
    only_agg, none = plm.aggregate_distance_maps(*args, MAPS[S], m_i, count=False, **kw)
    assert none is None and same_bits(only_agg, want_agg)
    none, only_count = plm.aggregate_distance_maps(*args, MAPS[S], m_i, agg=False, **kw)
    assert none is None and np.array_equal(only_count, want_count)


def golden():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "distance_maps.npz")) as z:
        return {k: z[k] for k in z.files}


def golden_chain(gold, name):
    ids, ridx, xyz = gold[name + "_ids"], gold[name + "_residue_index"], gold[name + "_xyz"]
    return sa.Chain(pd.DataFrame({"id": [str(v) for v in ids]}),
                    pd.DataFrame({"residue_index": ridx, "x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2]}))


def within_2_ulp(got, want):
    ok = ~np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and \
        bool((np.abs(got[ok] - want[ok]) <= 2 * np.spacing(want[ok])).all())


@pytest.mark.parametrize("case", ["intra_union", "intra_intersect", "inter_union", "inter_intersect"])
def test_aggregate_chains_reproduces_the_reference_aggregate(case):
    gold = golden()
    chains = [golden_chain(gold, c) for c in "ABC"]
    pairs = None if case.startswith("intra") else gold["pairs_inter"].tolist()
    ids_i, ids_j, matrix, counts = sa.aggregate_chains(chains, pairs, intersect=case.endswith("intersect"))
    assert np.array_equal(ids_i, gold["agg_%s_ids_i" % case]) and np.array_equal(ids_j, gold["agg_%s_ids_j" % case])
    assert within_2_ulp(matrix, gold["agg_%s_matrix" % case])
    assert np.array_equal(counts == 0, np.isnan(matrix)) and counts.max() <= 3


def test_the_patched_reference_function_gives_the_recorded_maps():
    gold = golden()
    module = types.ModuleType("stand_in_distances")
    module._distances = None
    sa.install(module)
    try:
        ra, xa, _ = sa.chain_atoms(golden_chain(gold, "A"))
        rb, xb, _ = sa.chain_atoms(golden_chain(gold, "B"))
        intra = module._distances(ra, xa, ra, xa, True)
        inter = module._distances(ra, xa, rb, xb, False)
    finally:
        sa.uninstall(module)
    assert module._distances is None
    assert within_2_ulp(intra, gold["intra_A"]) and within_2_ulp(inter, gold["inter_AB"])
    assert np.array_equal(intra, intra.T)


# ---- the plan knob ----------------------------------------------------------------------------------------------------

PLANS = ["t%d,c%d" % (t, c) for t in (4, 8, 16, 32, 64) for c in (1, 5, 16, 32)] + ["t8", "c7", "c3,t64"]


@pytest.mark.parametrize("plan", PLANS)
def test_every_plan_gives_the_same_bits(monkeypatch, plan):
    monkeypatch.setenv("PLM_DIST_PLAN", plan)
    xi, ri, xj, rj, want = pair_case(33, 65, "one300", "overlap", "double")
    assert same_bits(plm.residue_distances(xi, ri, xj, rj), want)
    x, r, want_sym = one_chain_case(65, "one300")
    sym = plm.residue_distances(x, r)
    assert same_bits(sym, want_sym) and np.array_equal(sym, sym.T)
    args, slots_j, m_i, m_j = chains_case()
    want_agg, want_count = aggregate_want(7, True)
    agg, count = plm.aggregate_distance_maps(*args, MAPS[7], m_i, slots_j=slots_j, m_j=m_j)
    assert same_bits(agg, want_agg) and np.array_equal(count, want_count)


@pytest.mark.parametrize("plan", ["t5", "t128", "c0", "c33", "t16,", "k4", ""])
def test_a_plan_the_planner_rejects_is_einval(monkeypatch, plan):
    monkeypatch.setenv("PLM_DIST_PLAN", plan)
    xi, ri, xj, rj, _ = pair_case(1, 1, "ca", "adjacent", "decimal")
    args, _, m_i, _ = chains_case()
    for call in (lambda: plm.residue_distances(xi, ri, xj, rj), lambda: plm.aggregate_distance_maps(*args, MAPS[1], m_i)):
        with pytest.raises(_lib.PlmError) as err:
            call()
        assert err.value.code == -1 and "PLM_DIST_PLAN" in str(err.value)


# ---- the command line ---------------------------------------------------------------------------------------------------

def write_pdb(gold, path):
    """the three recorded chains as fixed-column ATOM records (their coordinates have three decimals)"""
    lines, serial = [], 0
    for name in "ABC":
        ids, ridx, xyz = gold[name + "_ids"], gold[name + "_residue_index"], gold[name + "_xyz"]
        for k, (r, (x, y, z)) in enumerate(zip(ridx, xyz)):
            serial += 1
            atom = "CA" if k == 0 or ridx[k - 1] != r else "C%d" % (k % 100)
            lines.append("ATOM  %5d %-4s %3s %s%4d    %8.3f%8.3f%8.3f  1.00  0.00           C  "
                         % (serial, " " + atom, "GLY", name, ids[r], x, y, z))
        lines.append("TER")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\nEND\n")


def test_the_command_line_writes_the_recorded_comparison(tmp_path, capsys):
    from evcouplings_amd import contacts as contacts_cli
    gold = golden()
    pdb, ecs, out = (str(tmp_path / n) for n in ("abc.pdb", "ecs.csv", "out.csv"))
    write_pdb(gold, pdb)
    pd.DataFrame({"i": gold["ec_i"], "j": gold["ec_j"], "cn": gold["ec_cn"]}).to_csv(ecs, index=False)
    assert contacts_cli.main([ecs, pdb, "-o", out]) == 0
    table = pd.read_csv(out, float_precision="round_trip")
    for col in ("i", "j", "cn", "precision"):
        assert np.array_equal(table[col].values, gold["cmp_" + col], equal_nan=True), col
    assert within_2_ulp(table.dist.values, gold["cmp_dist"])
    printed = capsys.readouterr().out
    assert "precision at L/2" in printed and "precision at 2L" in printed and "chains A,B,C" in printed
    # C-alpha only, one chain: the distances between the first atoms of the residues of chain A
    assert contacts_cli.main([ecs, pdb, "--chain", "A", "--ca-only", "--cutoff", "8", "-o", out]) == 0
    ca = gold["A_xyz"][np.r_[True, np.diff(gold["A_residue_index"]) != 0]]
    want = twin.residue_distances(ca, np.stack((np.arange(len(ca)), np.arange(len(ca)))).T)
    table = pd.read_csv(out, float_precision="round_trip").dropna(subset=["dist"])
    pos = {v: k for k, v in enumerate(gold["A_ids"].tolist())}
    assert len(table) > 20
    assert np.array_equal(table.dist.values, [want[pos[i], pos[j]] for i, j in zip(table.i, table.j)])
