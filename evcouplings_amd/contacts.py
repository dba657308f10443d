"""
Hold a list of ECs against a structure.

    python -m evcouplings_amd.contacts ECS_FILE STRUCTURE.pdb [--chain A ...] [--cutoff 5] [--min-seq-dist 6]
                                       [--ca-only] [--score cn] [--device 0] -o OUT.csv

ECS_FILE is a CouplingScores-style CSV (columns i, j and the score).  The residue numbers of the PDB file are taken as
the positions of the ECs: there is no SIFTS mapping here.  The minimum atom distances of every listed chain (default:
every chain of the first model) are computed on the GPU and merged by their minimum (`structure_accel.aggregate_chains`,
the intra-chain maps only); residues with an insertion code and waters are left out.  --ca-only measures between C-alpha
atoms.  OUT.csv is the EC table with `dist` and `precision` added, sorted by score; the precision of the first L/2, L
and 2L ECs (L = the number of positions the EC table covers) is printed.
"""
import argparse
import sys


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m evcouplings_amd.contacts", description=__doc__,
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("ecs_file")
    p.add_argument("structure")
    p.add_argument("--chain", nargs="+", default=None, metavar="ID", help="chain ids to use (default: all)")
    p.add_argument("--cutoff", type=float, default=5.0, help="contact distance in Angstrom (default 5)")
    p.add_argument("--min-seq-dist", type=int, default=6, help="least |i - j| of an EC (default 6)")
    p.add_argument("--ca-only", action="store_true", help="distances between C-alpha atoms")
    p.add_argument("--score", default="cn", help="score column (default cn)")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("-o", "--output", required=True, metavar="OUT.csv")
    args = p.parse_args(argv)
    if args.cutoff <= 0:
        p.error("--cutoff must be positive")
    if args.min_seq_dist < 0:
        p.error("--min-seq-dist must not be negative")
    return args


def load_chains(path, chain_ids=None, ca_only=False):
    """The chains of a PDB file as structure_accel.Chain objects (and their ids), ready for aggregate_chains: waters
    and residues with an insertion code dropped, with ca_only every residue reduced to its CA atom."""
    from evcouplings_amd import structure_accel as sa
    residues, coords = sa.read_pdb_atoms(path)
    if chain_ids is None:
        chain_ids = list(dict.fromkeys(residues.chain.tolist()))
    chains = []
    for cid in chain_ids:
        res = residues.loc[(residues.chain == cid) & (residues.resname != "HOH") & residues.id.str.fullmatch(r"-?\d+")]
        atoms = coords.loc[coords.residue_index.isin(res.index)]
        if ca_only:
            atoms = atoms.loc[atoms.atom_name == "CA"]
            res = res.loc[res.index.isin(atoms.residue_index)]
        if len(res) == 0:
            raise ValueError("chain %r has no usable residue in %s" % (cid, path))
        chains.append(sa.Chain(res, atoms))
    return chains, chain_ids


def precision_at(table, n):
    """precision of the first n rows of a compared EC table (NaN when it has none)"""
    if len(table) == 0 or n < 1:
        return float("nan")
    return float(table.precision.values[min(n, len(table)) - 1])


def main(argv=None):
    import pandas as pd
    from evcouplings_amd import structure_accel as sa
    args = parse_args(argv)
    ecs = pd.read_csv(args.ecs_file)
    for col in ("i", "j", args.score):
        if col not in ecs.columns:
            sys.stderr.write("contacts: %s has no column %r\n" % (args.ecs_file, col))
            return 1
    chains, chain_ids = load_chains(args.structure, args.chain, args.ca_only)
    ids_i, ids_j, matrix, _ = sa.aggregate_chains(chains, device=args.device)
    table = sa.compare_ecs(ecs, (ids_i, ids_j), matrix, dist_cutoff=args.cutoff, score=args.score,
                           min_sequence_dist=args.min_seq_dist)
    table.to_csv(args.output, index=False)
    L = len(set(ecs.i.tolist()) | set(ecs.j.tolist()))
    print("chains %s: %d residues, %d ECs compared, L = %d" % (",".join(chain_ids), len(ids_i), len(table), L))
    for label, n in (("L/2", L // 2), ("L", L), ("2L", 2 * L)):
        print("precision at %-3s (%d ECs): %.4f" % (label, min(n, len(table)), precision_at(table, n)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
