"""
Residue distance maps of 3D structures on the GPU, and the comparison of ECs with them: the arithmetic of the
reference's compare stage (evcouplings/compare/distances.py, compare/ecs.py) without its SIFTS lookup, structure
download and mmCIF / MMTF parsing.

- ``residue_distances`` has the signature of the reference's numba kernel ``_distances`` (distances.py:24-88);
  ``install()`` rebinds that one function, so ``DistanceMap.from_coords`` -- and with it ``intra_dists``,
  ``multimer_dists`` and ``inter_dists`` -- computes its maps through ``plm.residue_distances``.
- ``aggregate_chains`` computes the minimum over many chains and chain pairs in one call
  (``plm.aggregate_distance_maps``): what the reference gets from one ``from_coords`` per chain (pair) followed by
  ``DistanceMap.aggregate`` with its default ``nanmin``, without the stack of maps.
- ``contacts`` and ``compare_ecs`` mirror ``DistanceMap.contacts`` and ``coupling_scores_compared``: host arithmetic on a
  few thousand rows, in numpy and pandas.
- ``read_pdb_atoms`` is a minimal reader of fixed-column PDB files for the command line tool
  (``python -m evcouplings_amd.contacts``).

Chains are duck-typed: ``.residues`` is a table with an ``id`` column, ``.coords`` one with ``residue_index``, ``x``,
``y``, ``z``, as the reference's ``Chain`` has them.  Nothing here imports the reference.  There is no CPU path: the
distances come from libplm_hip.so or the call raises.
"""
import collections

import numpy as np

Chain = collections.namedtuple("Chain", "residues coords")


def residue_distances(residues_i, coords_i, residues_j, coords_j, symmetric):
    """Drop-in for evcouplings.compare.distances._distances: residues_* (N, 2) first and last atom (inclusive) of every
    residue in coords_* (atoms, 3); returns the (N_i, N_j) matrix of minimum atom distances.  `symmetric`: axis j is
    axis i (the reference then reads only the upper triangle of the pairs, and so does this).  Differences: the
    operations are in one fixed order (at most 2 ulp from the reference's np.sum), and a residue without atoms is at
    1e6 from itself too, where the reference leaves 0 on the diagonal of a symmetric map."""
    from evcouplings_amd import plm
    if symmetric:
        return plm.residue_distances(coords_i, residues_i)
    return plm.residue_distances(coords_i, residues_i, coords_j, residues_j)


_ORIGINAL = {}


def install(distances_module=None):
    """Rebind `_distances` in evcouplings.compare.distances (or the module given) to `residue_distances`.
    `DistanceMap.aggregate` is not touched.  Returns the patched module."""
    if distances_module is None:
        import evcouplings.compare.distances as distances_module
    if distances_module not in _ORIGINAL:
        _ORIGINAL[distances_module] = distances_module._distances
    distances_module._distances = residue_distances
    return distances_module


def uninstall(distances_module=None):
    if distances_module is None:
        import evcouplings.compare.distances as distances_module
    if distances_module in _ORIGINAL:
        distances_module._distances = _ORIGINAL.pop(distances_module)


def chain_atoms(chain):
    """(ranges (N, 2) int32, xyz (atoms, 3) float64, ids (N,) int64) of a chain.  The atoms are grouped by
    `residue_index` in ascending order, as DistanceMap._extract_coords does, and group k belongs to row k of
    `.residues`; when the two counts differ, the groups are matched to the index of `.residues` instead and a residue
    without atoms gets an empty range.  The ids must be numeric (no insertion codes), as for DistanceMap.aggregate."""
    import pandas as pd
    coords = chain.coords.reset_index(drop=True)
    xyz = np.stack((coords.x.values, coords.y.values, coords.z.values)).T.astype(np.float64).reshape(-1, 3)
    pos = pd.Series(np.arange(len(coords)), index=coords.residue_index.values)
    grouped = pos.groupby(level=0)
    first, last = grouped.first(), grouped.last()
    try:
        ids = pd.to_numeric(chain.residues.id).astype(int).values.astype(np.int64)
    except ValueError as e:
        raise ValueError("residue ids must be numeric (no insertion codes allowed)") from e
    if len(first) == len(ids):
        ranges = np.stack((first.values, last.values)).T
    else:
        if not set(first.index).issubset(set(chain.residues.index)):
            raise ValueError("the atoms name residues that the residue table does not have")
        ranges = np.stack((first.reindex(chain.residues.index, fill_value=1).values,
                           last.reindex(chain.residues.index, fill_value=0).values)).T
    return ranges.astype(np.int32).reshape(-1, 2), xyz, ids


def _axis_ids(id_lists, intersect):
    sets = [set(ids.tolist()) for ids in id_lists]
    ids = set.intersection(*sets) if intersect else set.union(*sets)
    if not ids:
        raise ValueError("Intersection of positions on axis is empty, try intersect=False instead")
    return np.array(sorted(ids), dtype=np.int64)


def _slots(axis_ids, chain_ids, used):
    """the position of every residue id in the sorted axis ids, -1 where the axis lacks it or the chain is not on it"""
    out = []
    for ids, on_axis in zip(chain_ids, used):
        k = np.searchsorted(axis_ids, ids)
        hit = on_axis & (axis_ids[np.minimum(k, len(axis_ids) - 1)] == ids)
        out.append(np.where(hit, k, -1))
    return np.concatenate(out).astype(np.int32)


def aggregate_chains(chains, pairs=None, intersect=False, device=0):
    """
    The minimum distance map over many chains: `pairs` lists (index of the chain on axis i, index of the chain on axis
    j); None means every chain with itself, which is what the reference's intra_dists aggregates.  The axes are built
    as DistanceMap.aggregate builds them: the numeric residue ids of the chains on the axis, their sorted union, or
    their intersection with intersect=True.  Returns (ids_i, ids_j, matrix, counts): the ids of both axes (int64),
    the (len(ids_i), len(ids_j)) float64 minimum over the maps -- NaN where no map has the pair -- and the int32
    number of maps that have it.
    """
    from evcouplings_amd import plm
    chains = list(chains)
    if not chains:
        raise ValueError("no chains")
    pairs = [(k, k) for k in range(len(chains))] if pairs is None else [(int(a), int(b)) for a, b in pairs]
    if not pairs:
        raise ValueError("no chain pairs")
    for a, b in pairs:
        if not (0 <= a < len(chains) and 0 <= b < len(chains)):
            raise ValueError("pair (%d, %d) names a chain outside 0..%d" % (a, b, len(chains) - 1))
    parts = [chain_atoms(c) for c in chains]
    atom_off = np.cumsum([0] + [len(p[1]) for p in parts])
    res_off = np.cumsum([0] + [len(p[0]) for p in parts])
    ranges = np.concatenate([p[0] + np.int32(o) for p, o in zip(parts, atom_off)])
    coords = np.concatenate([p[1] for p in parts])
    chain_ids = [p[2] for p in parts]
    # one id set per map, as the reference has one per matrix
    ids_i = _axis_ids([chain_ids[a] for a, _ in pairs], intersect)
    ids_j = _axis_ids([chain_ids[b] for _, b in pairs], intersect)
    on_i, on_j = {a for a, _ in pairs}, {b for _, b in pairs}
    slots_i = _slots(ids_i, chain_ids, [k in on_i for k in range(len(chains))])
    slots_j = _slots(ids_j, chain_ids, [k in on_j for k in range(len(chains))])
    matrix, counts = plm.aggregate_distance_maps(coords, ranges, res_off, slots_i, pairs, len(ids_i), slots_j, len(ids_j),
                                                 device=device)
    return ids_i, ids_j, matrix, counts


def read_pdb_atoms(path, chain=None, hetatm=True):
    """
    Minimal reader of the fixed-column ATOM / HETATM records of a PDB file -> (residues, coords), the two tables a
    chain object carries.  residues: one row per residue in order of appearance, columns id (residue number plus
    insertion code, a string), resname, chain, hetatm; coords: residue_index (row of `residues`), atom_name, element,
    x, y, z, the atoms of a residue next to each other.  Only the first model is read; of alternate locations the first
    one of every atom stays; hydrogens (element column H or D) are dropped.  `chain`: keep this chain id only.
    This is not the reference's structure path (mmCIF / MMTF through compare/pdb.py): no SEQRES mapping, no
    secondary structure, no modified-residue translation.
    """
    import pandas as pd
    residues, atoms, index, seen = [], [], {}, set()
    with open(path) as f:
        for line in f:
            record = line[:6]
            if record.startswith("ENDMDL"):
                break
            if record not in ("ATOM  ", "HETATM") or (record == "HETATM" and not hetatm):
                continue
            chain_id = line[21]
            if chain is not None and chain_id != chain:
                continue
            if line[76:78].strip().upper() in ("H", "D"):
                continue
            key = (chain_id, line[22:27])            # residue number and insertion code
            name = line[12:16].strip()
            if (key, name) in seen:                  # a later alternate location of this atom
                continue
            seen.add((key, name))
            if key not in index:
                index[key] = len(residues)
                residues.append((line[22:27].strip(), line[17:20].strip(), chain_id, record == "HETATM"))
            atoms.append((index[key], name, line[76:78].strip(), float(line[30:38]), float(line[38:46]),
                          float(line[46:54])))
    res = pd.DataFrame(residues, columns=["id", "resname", "chain", "hetatm"])
    coords = pd.DataFrame(atoms, columns=["residue_index", "atom_name", "element", "x", "y", "z"])
    coords = coords.sort_values("residue_index", kind="stable").reset_index(drop=True)
    return res, coords


def _by_id(ids):
    return {str(v): k for k, v in enumerate(np.asarray(ids).tolist())}


def _pair_ids(ids):
    if isinstance(ids, (tuple, list)) and len(ids) == 2 and np.ndim(ids[0]) == 1:
        return ids[0], ids[1]
    return ids, ids


def contacts(ids_i, ids_j, matrix, max_dist=5.0, min_dist=None):
    """DistanceMap.contacts: the table (i, j, dist) of the pairs with dist <= max_dist (and dist > min_dist when given),
    the diagonal left out, in row-major order of the matrix."""
    import pandas as pd
    matrix = np.asarray(matrix)
    with np.errstate(invalid="ignore"):
        cond = matrix <= max_dist
        if min_dist is not None:
            cond &= matrix > min_dist
    i, j = np.where(cond)
    keep = i != j
    i, j = i[keep], j[keep]
    return pd.DataFrame({"i": np.asarray(ids_i)[i], "j": np.asarray(ids_j)[j], "dist": matrix[i, j]})


def _distances_of(ec_table, ids, matrix):
    ids_i, ids_j = _pair_ids(ids)
    map_i, map_j = _by_id(ids_i), _by_id(ids_j)
    matrix = np.asarray(matrix, dtype=np.float64)
    out = np.full(len(ec_table), np.nan)
    for k, (i, j) in enumerate(zip(ec_table.i, ec_table.j)):
        a, b = map_i.get(str(i)), map_j.get(str(j))
        if a is not None and b is not None:
            out[k] = matrix[a, b]
    return out


def compare_ecs(ec_table, ids, matrix, multimer=None, dist_cutoff=5, score="cn", min_sequence_dist=6):
    """
    coupling_scores_compared of compare/ecs.py on a distance matrix: a copy of `ec_table` (columns i, j and the score)
    with `dist` -- NaN where the structure lacks a residue of the pair --, without the pairs nearer than
    min_sequence_dist in sequence, and, when dist_cutoff is given, sorted by score (descending) with `precision`, the
    share of pairs within dist_cutoff among the pairs with a distance so far.  `ids`: the residue ids of the matrix
    axes, one array for both or a pair (ids_i, ids_j).  `multimer`: (ids, matrix) of a second map; then `dist_intra`,
    `dist_multimer` and dist = fmin of the two.
    """
    x = ec_table.copy()
    if multimer is None:
        x.loc[:, "dist"] = _distances_of(x, ids, matrix)
    else:
        x.loc[:, "dist_intra"] = _distances_of(x, ids, matrix)
        x.loc[:, "dist_multimer"] = _distances_of(x, multimer[0], multimer[1])
        x.loc[:, "dist"] = np.fmin(x.dist_intra, x.dist_multimer)
    if min_sequence_dist is not None:
        x = x.loc[(x.i - x.j).abs() >= min_sequence_dist]
    if dist_cutoff is not None:
        x = x.sort_values(by=score, ascending=False).copy()
        true_pos = (x.loc[:, "dist"] <= dist_cutoff).cumsum()
        with_dist = x.loc[:, "dist"].notnull().cumsum()
        x.loc[:, "precision"] = true_pos / with_dist
    return x
