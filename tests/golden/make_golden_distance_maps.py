#!/usr/bin/env python3
"""
Golden vectors of the reference's compare stage (run in the build container only; the reference does not exist on the
GPU box).  Three synthetic chains A (33 residues), B (17) and C (24) of 1 to 14 atoms per residue, coordinates with
three decimals, go through the reference's own `Chain`, `DistanceMap.from_coords`, `DistanceMap.aggregate`,
`DistanceMap.contacts` and `ecs.coupling_scores_compared`.  numba is absent, so the @jit loop `_distances` runs as plain
Python under the identity stub of tests/refstubs.py; the structure parsers the reference imports at module level
(Bio.PDB and its submodules) are stubbed here.  No reference source is written into this repo; only the arrays are
committed.

Stored (chain X in A, B, C):
  X_ids, X_residue_index, X_xyz    the residue ids (numeric), and per atom its residue row and coordinates
  intra_A, inter_AB                from_coords(A) (symmetric) and from_coords(A, B)
  agg_<case>_ids_i / _ids_j / _matrix   DistanceMap.aggregate (nanmin) for the cases
        intra_union, intra_intersect   from_coords(A), from_coords(B), from_coords(C)
        inter_union, inter_intersect   from_coords(A, B), from_coords(C, B), from_coords(A, C)
  pairs_intra, pairs_inter         the (chain on i, chain on j) lists of those cases, chains numbered A B C = 0 1 2
  contacts_5, contacts_3_8         contacts() of agg_intra_union as rows (i, j, dist), max_dist 5 / min 3 and max 8
  ec_i, ec_j, ec_cn                a synthetic EC table (distinct scores; positions inside and outside the structure)
  cmp_*, cmpm_*                    coupling_scores_compared(table, intra_union) and (table, intra_union, inter_union):
                                   columns i, j, cn, dist, precision (and dist_intra, dist_multimer)

Usage:  python tests/golden/make_golden_distance_maps.py      (writes tests/golden/distance_maps.npz)
"""
import os
import sys
import types

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import refstubs  # noqa: E402


def stub_structure_parsers():
    """refstubs leaves a stubbed `Bio` a plain module; compare/pdb.py imports submodules of it"""
    for name in ("Bio", "Bio.PDB", "Bio.PDB.binary_cif", "Bio.PDB.Polypeptide", "Bio.PDB.MMCIF2Dict"):
        mod = sys.modules.get(name)
        if mod is None or isinstance(mod, refstubs._Anything):
            mod = refstubs._Anything(name)
            mod.__path__ = []
            sys.modules[name] = mod
    for name in ("Bio.PDB", "Bio.PDB.binary_cif", "Bio.PDB.Polypeptide", "Bio.PDB.MMCIF2Dict"):
        parent, _, child = name.rpartition(".")
        setattr(sys.modules[parent], child, sys.modules[name])
    assert isinstance(sys.modules["Bio"], types.ModuleType)


def make_chain(rng, ids, centre):
    """residue ids -> (ids, residue_index per atom, xyz): a random walk of residue centres, 1..14 atoms around each"""
    n = len(ids)
    centres = centre + np.cumsum(rng.normal(scale=2.2, size=(n, 3)), axis=0)
    counts = rng.integers(1, 15, size=n)
    counts[0], counts[-1] = 1, 14
    residue_index = np.repeat(np.arange(n), counts)
    xyz = np.round(centres[residue_index] + rng.normal(scale=1.3, size=(len(residue_index), 3)), 3)
    return np.asarray(ids, dtype=np.int64), residue_index, xyz


def main():
    refstubs.install()
    stub_structure_parsers()
    from evcouplings.compare.pdb import Chain
    from evcouplings.compare.distances import DistanceMap
    from evcouplings.compare import ecs

    rng = np.random.default_rng(918)
    raw = {
        "A": make_chain(rng, np.arange(5, 38), np.array([0.0, 0.0, 0.0])),
        "B": make_chain(rng, np.delete(np.arange(20, 39), [4, 11]), np.array([3.0, -2.0, 4.0])),
        "C": make_chain(rng, np.arange(30, 54), np.array([-4.0, 5.0, 1.0])),
    }
    out, chains = {}, {}
    for name, (ids, residue_index, xyz) in raw.items():
        out[name + "_ids"], out[name + "_residue_index"], out[name + "_xyz"] = ids, residue_index.astype(np.int32), xyz
        residues = pd.DataFrame({"id": [str(v) for v in ids]})
        coords = pd.DataFrame({"residue_index": residue_index, "x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2]})
        chains[name] = Chain(residues, coords)
    A, B, C = chains["A"], chains["B"], chains["C"]
    intra = [DistanceMap.from_coords(c) for c in (A, B, C)]
    inter = [DistanceMap.from_coords(A, B), DistanceMap.from_coords(C, B), DistanceMap.from_coords(A, C)]
    out["intra_A"], out["inter_AB"] = intra[0].dist_matrix, inter[0].dist_matrix
    out["pairs_intra"] = np.array([(0, 0), (1, 1), (2, 2)], np.int32)
    out["pairs_inter"] = np.array([(0, 1), (2, 1), (0, 2)], np.int32)
    agg = {}
    for case, maps, intersect in (("intra_union", intra, False), ("intra_intersect", intra, True),
                                  ("inter_union", inter, False), ("inter_intersect", inter, True)):
        m = agg[case] = DistanceMap.aggregate(*maps, intersect=intersect)
        out["agg_%s_ids_i" % case] = m.residues_i.id.astype(int).values.astype(np.int64)
        out["agg_%s_ids_j" % case] = m.residues_j.id.astype(int).values.astype(np.int64)
        out["agg_%s_matrix" % case] = m.dist_matrix

    def contact_rows(table):
        return np.stack((table.i.astype(float).values, table.j.astype(float).values, table.dist.values)).T.reshape(-1, 3)

    out["contacts_5"] = contact_rows(agg["intra_union"].contacts(5.0))
    out["contacts_3_8"] = contact_rows(agg["intra_union"].contacts(8.0, 3.0))

    # ECs: every pair i < j of the positions 1..58 drawn at random, distinct scores
    i, j = np.triu_indices(58, 1)
    pick = rng.choice(len(i), 400, replace=False)
    table = pd.DataFrame({"i": i[pick] + 1, "j": j[pick] + 1, "cn": np.round(rng.permutation(400) * 0.01 - 0.5, 2)})
    out["ec_i"], out["ec_j"], out["ec_cn"] = table.i.values, table.j.values, table.cn.values
    for prefix, multimer in (("cmp", None), ("cmpm", agg["inter_union"])):
        x = ecs.coupling_scores_compared(table, agg["intra_union"], multimer)
        for col in x.columns:
            out["%s_%s" % (prefix, col)] = x[col].values
    path = os.path.join(HERE, "distance_maps.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes): %d arrays; %d contacts within 5 A, %d ECs compared, %d without a distance" % (
        path, os.path.getsize(path), len(out), len(out["contacts_5"]), len(out["cmp_dist"]),
        int(np.isnan(out["cmp_dist"]).sum())))


if __name__ == "__main__":
    main()
