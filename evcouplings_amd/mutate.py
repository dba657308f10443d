"""
Score mutants under a fitted Potts model on the GPU:

    python -m evcouplings_amd.mutate MODEL --table IN.csv -o OUT.csv [--column mutant] [--hamiltonian full|couplings|fields]
                                     [--independent] [--segment ID]
    python -m evcouplings_amd.mutate MODEL --scan POS,POS,... -o OUT.csv [--exclude -] [--top K] [--histogram BINS]

MODEL is a plmc_v2 `.model` file.  --table reads a CSV file of mutants in the notation of the mutate stage ("K50R",
"K50R,I100V", "wild"), in the column named by --column, and writes it back with the column `prediction_epistatic`: the
difference in statistical energy to the model's target sequence (--hamiltonian selects the full difference, or its
coupling or field part).  Rows that cannot be scored (a position or letter the model does not have, a from-letter that
is not the target's, a position named twice) get NaN.  --independent adds `prediction_independent`, the same table
under the independent-site model of the file's frequencies, as the mutate protocol does.  A `segment` column in the
table, or --segment, addresses the positions of a model with segments.
--scan enumerates every combination of letters at the listed positions (the model's numbering; at most 8), without the
letters of --exclude, and writes the K best (default 100), best first: index, letters, mutant, dH, dH_J, dH_h.
--histogram BINS also writes OUT.csv.hist.csv: BINS equal bins between the smallest and the largest dH of the whole
library (lower, upper, count).
"""
import argparse
import sys
from types import SimpleNamespace

import numpy as np

from evcouplings_amd import model_accel, model_io, sample

EPISTATIC, INDEPENDENT = "prediction_epistatic", "prediction_independent"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m evcouplings_amd.mutate", description=__doc__.split("\n\n")[0])
    ap.add_argument("model")
    ap.add_argument("-o", required=True, help="output CSV file")
    ap.add_argument("--table", default=None, metavar="CSV", help="table of mutants to score")
    ap.add_argument("--column", default="mutant", help="column of the table that holds the mutants")
    ap.add_argument("--hamiltonian", choices=tuple(model_accel.COMPONENT_TO_INDEX), default="full")
    ap.add_argument("--independent", action="store_true", help="add the independent-model column")
    ap.add_argument("--segment", default=None, help="segment identifier of every position of the table")
    ap.add_argument("--scan", default=None, metavar="POS,...", help="positions whose letter combinations are enumerated")
    ap.add_argument("--exclude", default="-", help="letters left out of a scan")
    ap.add_argument("--top", type=int, default=100, metavar="K", help="write the K best combinations")
    ap.add_argument("--histogram", type=int, default=None, metavar="BINS")
    a = ap.parse_args(argv)
    if (a.table is None) == (a.scan is None):
        ap.error("give either --table or --scan")
    if a.scan is not None:
        try:
            a.positions = [int(p) for p in a.scan.split(",") if p.strip()]
        except ValueError:
            ap.error("--scan takes comma-separated integer positions")
        if not 1 <= len(a.positions) <= 8 or len(set(a.positions)) != len(a.positions):
            ap.error("--scan takes between 1 and 8 distinct positions")
        if a.top < 1:
            ap.error("--top K >= 1")
        if a.histogram is not None and not 1 <= a.histogram <= 1025:
            ap.error("--histogram takes between 1 and 1025 bins")
        if a.independent:
            ap.error("--independent goes with --table")
    elif a.histogram is not None:
        ap.error("--histogram goes with --scan")
    return a


def independent_model(model, path):
    """The independent-site model of the file's frequencies (`plm.independent_fields`), no couplings."""
    from evcouplings_amd import plm
    m = model_io.read_model_file(path)
    if not float(m["lambda_h"]) > 0.0:
        sys.exit("%s: lambda_h = %g, the independent model needs lambda_h > 0" % (path, m["lambda_h"]))
    h, _ = plm.independent_fields(m["fi"], m["lambda_h"], m["n_eff"])
    return SimpleNamespace(J_ij=np.zeros_like(model.J_ij), h_i=h, alphabet=model.alphabet, target_seq=model.target_seq,
                           index_list=model.index_list, L=model.L, q=model.q)


def library_histogram(model, positions, exclude, bins):
    """(lower, upper, count) of `bins` equal bins over [min dH, max dH] of the whole library."""
    from evcouplings_amd import plm
    h_i = np.asarray(model.h_i)
    q = h_i.shape[1]
    index_map, alphabet_map = model_accel._model_maps(model)
    _, code = model_accel._letters_and_code(model, q)
    allowed = model_accel._allowed_flags(exclude, code, q)
    states = np.arange(q) if allowed is None else np.nonzero(allowed)[0]
    args = (model_accel._target_states(model, alphabet_map), q, h_i, model_accel._pairs_from_dense(np.asarray(model.J_ij)),
            [index_map[p] for p in positions])
    ext = plm.mutant_scan(*args, letters=[states] * len(positions))
    bounds = np.linspace(ext["dh_min"], ext["dh_max"], bins + 1)
    res = plm.mutant_scan(*args, letters=[states] * len(positions), edges=np.maximum.accumulate(bounds[1:-1]))
    return bounds[:-1], bounds[1:], res["histogram"]


def main(argv=None):
    import pandas as pd
    a = parse_args(argv)
    model = sample.model_from_file(a.model)
    if a.scan is not None:
        try:
            out = model_accel.scan_library(model, a.positions, exclude=a.exclude, top=a.top)
        except ValueError as e:
            sys.exit(str(e))
        out.to_csv(a.o, index=False)
        if a.histogram is not None:
            lower, upper, count = library_histogram(model, a.positions, a.exclude, a.histogram)
            pd.DataFrame({"lower": lower, "upper": upper, "count": count}).to_csv(a.o + ".hist.csv", index=False)
        return 0
    table = pd.read_csv(a.table, keep_default_na=False)
    if a.column not in table.columns:
        sys.exit("%s has no column %r" % (a.table, a.column))
    parsed = model_accel.parse_table(model, table, mutant_column=a.column, segment=a.segment)
    out = model_accel.predict_mutation_table(model, table, EPISTATIC, a.column, a.hamiltonian, parsed=parsed)
    if a.independent:
        out = model_accel.predict_mutation_table(independent_model(model, a.model), out, INDEPENDENT, a.column,
                                                 a.hamiltonian, parsed=parsed)
    out.to_csv(a.o, index=False)
    return 0


if __name__ == "__main__":
    sys.exit(main())
