"""
Residue distance maps, host side (no GPU): the numpy twin against the recorded reference results, the argument checks of
the two entry points, the PDB reader, contacts / compare_ecs against the recorded tables, the install hook and the
command line of evcouplings_amd.contacts.

Twin against golden: the twin adds (dx2 + dy2) + dz2, the reference np.sum's the three squares; the two can differ in
the association of a three-term sum of non-negative numbers, at most 2 ulp of d2, which is 1 ulp of d, plus the rounding
of the square root: 2 ulp (np.spacing) of the recorded value are allowed.
"""
import ctypes as C
import os
import types

import numpy as np
import pandas as pd
import pytest

import distance_twin as twin
from evcouplings_amd import _lib, contacts as contacts_cli, plm, protocol, structure_accel as sa

CHAINS = "ABC"


@pytest.fixture(scope="module")
def gold(golden_dir):
    with np.load(os.path.join(golden_dir, "distance_maps.npz")) as z:
        return {k: z[k] for k in z.files}


def chain_tables(gold, name):
    """the chain as the duck-typed object aggregate_chains takes"""
    ids, ridx, xyz = gold[name + "_ids"], gold[name + "_residue_index"], gold[name + "_xyz"]
    residues = pd.DataFrame({"id": [str(v) for v in ids]})
    coords = pd.DataFrame({"residue_index": ridx, "x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2]})
    return sa.Chain(residues, coords)


def within_2_ulp(got, want):
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    return bool((np.abs(got[ok] - want[ok]) <= 2 * np.spacing(want[ok])).all())


def test_twin_equals_the_reference_maps(gold):
    ra, xa, _ = sa.chain_atoms(chain_tables(gold, "A"))
    rb, xb, _ = sa.chain_atoms(chain_tables(gold, "B"))
    assert within_2_ulp(twin.residue_distances(xa, ra), gold["intra_A"])
    assert within_2_ulp(twin.residue_distances(xa, ra, xb, rb), gold["inter_AB"])
    sym = twin.residue_distances(xa, ra)
    assert np.array_equal(sym, sym.T) and np.array_equal(sym, twin.residue_distances(xa, ra, xa, ra))


def aggregate_inputs(gold, pairs, intersect):
    """what aggregate_chains hands to plm.aggregate_distance_maps, built with its own helpers"""
    parts = [sa.chain_atoms(chain_tables(gold, c)) for c in CHAINS]
    atom_off = np.cumsum([0] + [len(p[1]) for p in parts])
    res_off = np.cumsum([0] + [len(p[0]) for p in parts])
    ranges = np.concatenate([p[0] + np.int32(o) for p, o in zip(parts, atom_off)])
    coords = np.concatenate([p[1] for p in parts])
    ids = [p[2] for p in parts]
    ids_i = sa._axis_ids([ids[a] for a, _ in pairs], intersect)
    ids_j = sa._axis_ids([ids[b] for _, b in pairs], intersect)
    slots_i = sa._slots(ids_i, ids, [k in {a for a, _ in pairs} for k in range(3)])
    slots_j = sa._slots(ids_j, ids, [k in {b for _, b in pairs} for k in range(3)])
    return ids_i, ids_j, (coords, ranges, res_off, slots_i, pairs, len(ids_i), slots_j, len(ids_j))


@pytest.mark.parametrize("case", ["intra_union", "intra_intersect", "inter_union", "inter_intersect"])
def test_aggregation_twin_equals_the_reference_aggregate(gold, case):
    pairs = gold["pairs_" + case.split("_")[0]].tolist()
    ids_i, ids_j, args = aggregate_inputs(gold, pairs, case.endswith("intersect"))
    assert np.array_equal(ids_i, gold["agg_%s_ids_i" % case]) and np.array_equal(ids_j, gold["agg_%s_ids_j" % case])
    agg, count = twin.aggregate_distance_maps(*args)
    assert within_2_ulp(agg, gold["agg_%s_matrix" % case])
    assert np.array_equal(count == 0, np.isnan(agg)) and count.max() <= len(pairs)


def einval(call, word):
    with pytest.raises(_lib.PlmError) as err:
        call()
    assert err.value.code == -1 and word in str(err.value), str(err.value)


XYZ = np.arange(18, dtype=np.float64).reshape(6, 3)
RNG2 = np.array([[0, 2], [3, 5]], np.int32)


def test_residue_distances_refuses_bad_arguments_before_the_device_is_looked_at():
    lib = _lib.load()
    out = np.zeros((2, 2))
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    for args in ((None, 6, p(RNG2), 2, None, 0, None, 0, p(out)), (p(XYZ), 6, None, 2, None, 0, None, 0, p(out)),
                 (p(XYZ), 6, p(RNG2), 2, None, 0, None, 0, None), (p(XYZ), 6, p(RNG2), 2, p(XYZ), 6, None, 2, p(out)),
                 (p(XYZ), 6, p(RNG2), 2, None, 6, p(RNG2), 2, p(out))):
        assert lib.plm_residue_distances(*args, 0, None) == -1
    einval(lambda: plm.residue_distances(np.zeros((0, 3)), RNG2), "below 1")
    einval(lambda: plm.residue_distances(XYZ, np.zeros((0, 2), np.int32)), "below 1")
    einval(lambda: plm.residue_distances(XYZ, RNG2, XYZ, np.zeros((0, 2), np.int32)), "below 1")
    einval(lambda: plm.residue_distances(XYZ, [[0, 2], [3, 6]]), "outside")
    einval(lambda: plm.residue_distances(XYZ, [[-1, 2], [3, 5]]), "outside")
    einval(lambda: plm.residue_distances(XYZ, RNG2, XYZ[:3], RNG2), "outside")
    for bad in (np.nan, np.inf, -np.inf):
        x = XYZ.copy()
        x[4, 1] = bad
        einval(lambda: plm.residue_distances(x, RNG2), "not finite")
        einval(lambda: plm.residue_distances(XYZ, RNG2, x, RNG2), "not finite")
    with pytest.raises(ValueError):
        plm.residue_distances(XYZ, RNG2, XYZ, None)
    with pytest.raises(ValueError):
        plm.residue_distances(XYZ.reshape(9, 2), RNG2)


def test_aggregate_refuses_bad_arguments_before_the_device_is_looked_at():
    lib = _lib.load()
    off, slots, maps = np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32), np.array([[0, 1]], np.int32)
    agg = np.zeros((2, 2))
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    good = [p(XYZ), 6, p(RNG2), p(off), 2, p(slots), None, 2, 2, p(maps), 1, p(agg), None]
    for k in (0, 2, 3, 5, 9):
        args = list(good)
        args[k] = None
        assert lib.plm_distance_maps_aggregate(*args, 0, None) == -1
    call = plm.aggregate_distance_maps
    einval(lambda: call(np.zeros((0, 3)), RNG2, off, slots, maps, 2), "below 1")
    einval(lambda: call(XYZ, RNG2, off, slots, maps, 0), "below 1")
    einval(lambda: call(XYZ, RNG2, off, slots, maps, 2, m_j=0), "below 1")
    einval(lambda: call(XYZ, RNG2, off, slots, np.zeros((0, 2), np.int32), 2), "below 1")
    einval(lambda: call(XYZ, [[0, 2], [3, 6]], off, slots, maps, 2), "outside")
    x = XYZ.copy()
    x[0, 0] = np.nan
    einval(lambda: call(x, RNG2, off, slots, maps, 2), "not finite")
    einval(lambda: call(XYZ, RNG2, off, [0, 2], maps, 2), "outside -1..1")
    einval(lambda: call(XYZ, RNG2, off, [-2, 1], maps, 2), "outside -1..1")
    einval(lambda: call(XYZ, RNG2, off, slots, maps, 2, slots_j=[0, 5], m_j=3), "outside -1..2")
    einval(lambda: call(XYZ, RNG2, [0, 2], [1, 1], [[0, 0]], 2), "share slot")
    einval(lambda: call(XYZ, RNG2, [0, 2], [0, 1], [[0, 0]], 2, slots_j=[0, 0]), "share slot")
    einval(lambda: call(XYZ, RNG2, off, slots, [[0, 2]], 2), "chain outside")
    einval(lambda: call(XYZ, RNG2, off, slots, [[-1, 0]], 2), "chain outside")
    einval(lambda: call(XYZ, RNG2, [1, 1, 2], slots, maps, 2), "not 0")
    # two chains may share a slot: that is what the aggregation is for (refused only for lack of a device, if at all)
    try:
        call(XYZ, RNG2, off, [1, 1], maps, 2)
    except _lib.PlmError as e:
        assert e.code != -1


@pytest.mark.parametrize("value", ["", "t", "t5", "t16,", "c0", "c33", "x4", "t16;c4", "16", "t-4", "c4,,t8"])
def test_a_bad_plan_is_refused_before_the_device_is_looked_at(monkeypatch, value):
    monkeypatch.setenv("PLM_DIST_PLAN", value)
    off, slots = np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32)
    einval(lambda: plm.residue_distances(XYZ, RNG2), "PLM_DIST_PLAN")
    einval(lambda: plm.aggregate_distance_maps(XYZ, RNG2, off, slots, [[0, 1]], 2), "PLM_DIST_PLAN")


def test_no_cpu_fallback_without_a_gpu():
    if _lib.load().plm_device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(_lib.PlmError) as err:
        plm.residue_distances(XYZ, RNG2)
    assert err.value.code != -1
    with pytest.raises(_lib.PlmError):
        sa.residue_distances(RNG2, XYZ, RNG2, XYZ, True)


PDB_LINES = [
    "HEADER    HAND-WRITTEN FIXTURE",
    "ATOM      1  N   ALA A   1      11.104   6.134  -6.504  1.00  0.00           N  ",
    "ATOM      2  CA  ALA A   1      11.639   6.071  -5.147  1.00  0.00           C  ",
    "ATOM      3  H   ALA A   1      10.500   5.500  -7.000  1.00  0.00           H  ",
    "ATOM      4  N   GLY A   2      12.500   7.250  -4.000  1.00  0.00           N  ",
    "ATOM      5  CA AGLY A   2      13.250   8.125  -3.500  0.60  0.00           C  ",
    "ATOM      6  CA BGLY A   2      13.750   8.625  -3.250  0.40  0.00           C  ",
    "ATOM      7  O   GLY A   2      14.000   9.000  -2.000  1.00  0.00           O  ",
    "ATOM      8  CA  SER B   7       1.000   2.000   3.000  1.00  0.00           C  ",
    "TER",
    "HETATM    9  O   HOH A 101       0.000   0.000   0.000  1.00  0.00           O  ",
    "ATOM     10  C   ALA A   1      11.700   6.100  -5.100  1.00  0.00           C  ",
    "ENDMDL",
    "MODEL        2",
    "ATOM      1  N   ALA A   1      99.000  99.000  99.000  1.00  0.00           N  ",
    "ENDMDL",
]


def test_read_pdb_atoms_on_a_hand_written_file(tmp_path):
    path = tmp_path / "three.pdb"
    path.write_text("\n".join(PDB_LINES) + "\n")
    res, coords = sa.read_pdb_atoms(str(path), chain="A")
    assert res.id.tolist() == ["1", "2", "101"] and res.resname.tolist() == ["ALA", "GLY", "HOH"]
    assert res.hetatm.tolist() == [False, False, True]
    # no hydrogen, the first alternate location only, the late atom of residue 1 moved next to its residue, no model 2
    assert coords.residue_index.tolist() == [0, 0, 0, 1, 1, 1, 2]
    assert coords.atom_name.tolist() == ["N", "CA", "C", "N", "CA", "O", "O"]
    assert coords.x.tolist() == [11.104, 11.639, 11.7, 12.5, 13.25, 14.0, 0.0]
    assert coords.z.tolist()[:2] == [-6.504, -5.147]
    ranges, xyz, ids = sa.chain_atoms(sa.Chain(res, coords))
    assert ranges.tolist() == [[0, 2], [3, 5], [6, 6]] and ids.tolist() == [1, 2, 101] and xyz.shape == (7, 3)
    everything, _ = sa.read_pdb_atoms(str(path))
    assert everything.chain.tolist() == ["A", "A", "B", "A"]
    no_het, _ = sa.read_pdb_atoms(str(path), chain="A", hetatm=False)
    assert no_het.id.tolist() == ["1", "2"]
    chains, chain_ids = contacts_cli.load_chains(str(path), ca_only=True)
    assert chain_ids == ["A", "B"] and chains[0].residues.id.tolist() == ["1", "2"]
    assert chains[0].coords.atom_name.tolist() == ["CA", "CA"] and chains[1].coords.x.tolist() == [1.0]


def test_chain_atoms_gives_a_residue_without_atoms_an_empty_range():
    residues = pd.DataFrame({"id": ["4", "5", "6"]})
    coords = pd.DataFrame({"residue_index": [0, 0, 2], "x": [0.0, 1.0, 2.0], "y": 0.0, "z": 0.0})
    ranges, _, ids = sa.chain_atoms(sa.Chain(residues, coords))
    assert ranges.tolist() == [[0, 1], [1, 0], [2, 2]] and ids.tolist() == [4, 5, 6]
    with pytest.raises(ValueError):
        sa.chain_atoms(sa.Chain(pd.DataFrame({"id": ["4", "5A"]}), coords.iloc[:2]))


def test_contacts_equal_the_recorded_tables(gold):
    ids_i, ids_j, m = (gold["agg_intra_union_" + k] for k in ("ids_i", "ids_j", "matrix"))
    for key, kw in (("contacts_5", {}), ("contacts_3_8", {"max_dist": 8.0, "min_dist": 3.0})):
        got = sa.contacts(ids_i, ids_j, m, **kw)
        want = gold[key]
        assert len(want) > 50
        assert np.array_equal(got.i.values, want[:, 0]) and np.array_equal(got.j.values, want[:, 1])
        assert np.array_equal(got.dist.values, want[:, 2])


@pytest.mark.parametrize("prefix", ["cmp", "cmpm"])
def test_compare_ecs_equals_the_recorded_table(gold, prefix):
    table = pd.DataFrame({"i": gold["ec_i"], "j": gold["ec_j"], "cn": gold["ec_cn"]})
    ids = (gold["agg_intra_union_ids_i"], gold["agg_intra_union_ids_j"])
    multimer = None
    if prefix == "cmpm":
        multimer = ((gold["agg_inter_union_ids_i"], gold["agg_inter_union_ids_j"]), gold["agg_inter_union_matrix"])
    got = sa.compare_ecs(table, ids, gold["agg_intra_union_matrix"], multimer=multimer)
    columns = [k[len(prefix) + 1:] for k in gold if k.startswith(prefix + "_")]
    assert set(columns) >= {"i", "j", "cn", "dist", "precision"} and set(got.columns) == set(columns)
    assert np.isnan(gold[prefix + "_dist"]).any() and not np.isnan(gold[prefix + "_dist"]).all()
    for col in columns:
        assert np.array_equal(got[col].values, gold["%s_%s" % (prefix, col)], equal_nan=True), col
    assert (np.abs(got.i - got.j) >= 6).all() and (np.diff(got.cn.values) <= 0).all()
    assert len(table) == 400        # the caller's table is left alone
    # one id array for both axes, and no cutoff: no sort, no precision
    plain = sa.compare_ecs(table, ids[0], gold["agg_intra_union_matrix"], dist_cutoff=None, min_sequence_dist=None)
    assert "precision" not in plain.columns and np.array_equal(plain.i.values, table.i.values)


def test_install_and_uninstall_on_a_stand_in_module():
    def original(*a):
        return "original"
    module = types.ModuleType("stand_in_distances")
    module._distances = original
    assert sa.install(module) is module and module._distances is sa.residue_distances
    sa.install(module)                          # twice: the original is still remembered
    sa.uninstall(module)
    assert module._distances is original
    sa.uninstall(module)                        # and uninstalling twice is harmless
    assert module._distances is original
    sa.install(module)
    protocol_module = types.ModuleType("second_stand_in")
    protocol_module._distances = original
    sa.install(protocol_module)
    for m in list(sa._ORIGINAL):
        sa.uninstall(m)
    assert module._distances is original and protocol_module._distances is original
    import inspect
    assert "structures" in inspect.signature(protocol.install_all).parameters
    assert inspect.signature(protocol.install_all).parameters["structures"].default is False


def test_command_line_arguments():
    a = contacts_cli.parse_args(["ecs.csv", "s.pdb", "-o", "out.csv"])
    assert (a.ecs_file, a.structure, a.output) == ("ecs.csv", "s.pdb", "out.csv")
    assert a.chain is None and a.cutoff == 5.0 and a.min_seq_dist == 6 and not a.ca_only and a.score == "cn"
    a = contacts_cli.parse_args(["e", "s", "--chain", "A", "B", "--cutoff", "8", "--min-seq-dist", "4", "--ca-only",
                                 "-o", "x"])
    assert a.chain == ["A", "B"] and a.cutoff == 8.0 and a.min_seq_dist == 4 and a.ca_only
    for bad in (["e", "s"], ["e", "-o", "x"], ["e", "s", "-o", "x", "--cutoff", "0"],
                ["e", "s", "-o", "x", "--min-seq-dist", "-1"], ["e", "s", "-o", "x", "--cutoff", "near"]):
        with pytest.raises(SystemExit):
            contacts_cli.parse_args(bad)
    table = pd.DataFrame({"precision": [1.0, 0.5, 0.25]})
    assert contacts_cli.precision_at(table, 2) == 0.5 and contacts_cli.precision_at(table, 10) == 0.25
    assert np.isnan(contacts_cli.precision_at(table, 0)) and np.isnan(contacts_cli.precision_at(table.iloc[:0], 3))
