"""
Pair the sequences of two monomer alignments by their inter-protein energy under a model fitted on the concatenation:

    python -m evcouplings_amd.pairing MODEL A.a2m B.a2m --species-a A.csv --species-b B.csv [--method assignment|reciprocal_best]
                                      [--min-gap G] [--skip-gap] [--gauge zero_sum|none] -o PAIRS.csv
    python -m evcouplings_amd.pairing MODEL A.a2m B.a2m --all-against-all [--skip-gap] [--gauge zero_sum|none] -o TABLE.csv

MODEL is a plmc_v2 `.model` file of a concatenated alignment, the sites of A first: its first L_A sites are matched with
the columns of A.a2m, the remaining L_B with those of B.a2m (an alignment wider than its side is reduced to its match
columns, the upper-case and '-' columns of its first record).  The annotation files are two-column CSV files, id then
species, with or without a header line "id,species"; sequences without a species are left out.
PAIRS.csv holds id_1, id_2, species, energy, gap (`complex_accel.match_by_species`): its first two columns are what the
reference's write_concatenated_alignment(id_pairing, ...) takes.  --min-gap keeps the pairs whose energy beats every
alternative of either partner by G at least.  --all-against-all writes, for every sequence of A, its best partner among
all sequences of B: id_1, id_2, energy, second, reciprocal (1 when id_1 is also the best partner of id_2).
"""
import argparse
import sys

import numpy as np

from evcouplings_amd import alignment_io, complex_accel, model_io


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m evcouplings_amd.pairing", description=__doc__.split("\n\n")[0])
    ap.add_argument("model")
    ap.add_argument("alignment_a")
    ap.add_argument("alignment_b")
    ap.add_argument("-o", required=True, help="output CSV file")
    ap.add_argument("--species-a", default=None, metavar="CSV", help="id,species of the sequences of A")
    ap.add_argument("--species-b", default=None, metavar="CSV", help="id,species of the sequences of B")
    ap.add_argument("--method", choices=("assignment", "reciprocal_best"), default="assignment")
    ap.add_argument("--min-gap", type=float, default=None, metavar="G")
    ap.add_argument("--skip-gap", action="store_true", help="leave out every term with a gap on either side")
    ap.add_argument("--gauge", choices=("zero_sum", "none"), default="zero_sum")
    ap.add_argument("--all-against-all", action="store_true", help="best-partner table over all sequences, no species")
    a = ap.parse_args(argv)
    if a.all_against_all:
        if a.species_a or a.species_b or a.min_gap is not None or a.method != "assignment":
            ap.error("--all-against-all takes no species files, --method or --min-gap")
    elif not a.species_a or not a.species_b:
        ap.error("give --species-a and --species-b, or --all-against-all")
    if a.min_gap is not None and not np.isfinite(a.min_gap):
        ap.error("--min-gap takes a finite number")
    return a


def read_side(path, n_sites=None):
    """(ids, letter matrix) of a monomer alignment, upper case, '.' as '-': every column when the file has exactly n_sites
    of them, else its match columns (the upper-case and '-' columns of the first record)"""
    ids, mat = alignment_io.read_fasta_matrix(path)
    if mat.shape[1] != n_sites:
        first = mat[0]
        match = ((first >= ord("A")) & (first <= ord("Z"))) | (first == ord("-"))
        if n_sites is not None and int(match.sum()) != n_sites:
            sys.exit("%s: %d columns, %d of them match columns; the model has %d sites on this side" % (
                path, mat.shape[1], int(match.sum()), n_sites))
        mat = mat[:, match]
    letters = np.char.upper(np.ascontiguousarray(mat, dtype=np.uint8).view("S1").astype("U1"))
    letters[letters == "."] = "-"
    return [i.split()[0] if i.split() else i for i in ids], letters


def read_species(path):
    """{id: species} of a two-column CSV file"""
    import pandas as pd
    table = pd.read_csv(path, header=None, dtype=str, keep_default_na=False)
    if table.shape[1] < 2:
        sys.exit("%s: expected two columns, id and species" % path)
    if len(table) and (table.iloc[0, 0].strip().lower(), table.iloc[0, 1].strip().lower()) == ("id", "species"):
        table = table.iloc[1:]
    return {i.strip(): s.strip() for i, s in zip(table.iloc[:, 0], table.iloc[:, 1]) if s.strip()}


def main(argv=None):
    import pandas as pd
    a = parse_args(argv)
    model = model_io.read_model_file(a.model)
    L = model["L"]
    ids_a, mat_a = read_side(a.alignment_a)
    n_a_sites = mat_a.shape[1]
    if not 1 <= n_a_sites < L:
        sys.exit("%s has %d match columns, the model %d sites in all" % (a.alignment_a, n_a_sites, L))
    ids_b, mat_b = read_side(a.alignment_b, L - n_a_sites)
    sides = dict(sites_a=np.arange(n_a_sites), sites_b=np.arange(n_a_sites, L),
                 gauge=None if a.gauge == "none" else a.gauge, skip_gap=a.skip_gap)
    try:
        if a.all_against_all:
            res = complex_accel.interaction_energies(model, mat_a, mat_b, matrix=False, best=True, **sides)
            rows, cols = res["rows_best"], res["cols_best"]
            t = rows["index"]
            out = pd.DataFrame({"id_1": ids_a, "id_2": np.asarray(ids_b, dtype=object)[t], "energy": rows["best"],
                                "second": rows["second"], "reciprocal": (cols["index"][t] == np.arange(len(t))).astype(int)})
        else:
            sp_a, sp_b = read_species(a.species_a), read_species(a.species_b)
            keep_a = [k for k, i in enumerate(ids_a) if i in sp_a]
            keep_b = [k for k, i in enumerate(ids_b) if i in sp_b]
            out = complex_accel.match_by_species(
                model, mat_a[keep_a], mat_b[keep_b], [sp_a[ids_a[k]] for k in keep_a], [sp_b[ids_b[k]] for k in keep_b],
                method=a.method, ids_a=[ids_a[k] for k in keep_a], ids_b=[ids_b[k] for k in keep_b], min_gap=a.min_gap,
                **sides)
    except ValueError as e:
        sys.exit(str(e))
    out.to_csv(a.o, index=False)
    return 0


if __name__ == "__main__":
    sys.exit(main())
