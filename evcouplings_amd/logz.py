"""
Estimate log Z of a fitted Potts model on the GPU by annealed importance sampling:

    python -m evcouplings_amd.logz MODEL [-n CHAINS] [-k TEMPS] [--sweeps N] [--seed S] [--sequences A2M -o OUT.csv]

MODEL is a plmc_v2 `.model` file.  CHAINS chains are annealed from the independent-site model of the fields to the full
model over TEMPS temperatures with N Gibbs sweeps at each.  Prints log Z, its standard error, the effective sample size
of the chains and the entropy of the model.  With --sequences, every record of the A2M / FASTA file (the model's columns:
lower-case letters and dots are dropped) gets a line id, H, log P = H - log Z in OUT.csv.
"""
import argparse
import sys

import numpy as np

from evcouplings_amd import model_accel
from evcouplings_amd.sample import model_from_file


def read_a2m(path, L):
    """[(id, match columns)] of a FASTA / A2M file; every record must hold L match columns."""
    records, name, parts = [], None, []

    def close():
        if name is not None:
            seq = "".join(c for c in "".join(parts) if not (c.islower() or c == "."))
            if len(seq) != L:
                raise ValueError("record %s has %d match columns, the model %d" % (name, len(seq), L))
            records.append((name, seq))

    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                close()
                name, parts = line[1:].split()[0] if len(line) > 1 else "", []
            elif line and name is not None:
                parts.append(line)
    close()
    return records


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m evcouplings_amd.logz", description=__doc__.split("\n\n")[0])
    ap.add_argument("model")
    ap.add_argument("-n", type=int, default=4096, help="number of chains")
    ap.add_argument("-k", type=int, default=1000, help="number of temperatures")
    ap.add_argument("--sweeps", type=int, default=1, help="Gibbs sweeps per temperature")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sequences", default=None, help="A2M / FASTA file of sequences to score")
    ap.add_argument("-o", default=None, help="CSV file for id, H, log P of the sequences")
    a = ap.parse_args(argv)
    if (a.sequences is None) != (a.o is None):
        ap.error("--sequences and -o go together")
    model = model_from_file(a.model)
    records = read_a2m(a.sequences, model.L) if a.sequences else []
    res = model_accel.log_partition(model, n_chains=a.n, n_temps=a.k, sweeps_per_temp=a.sweeps, seed=a.seed)
    print("log Z = %.6f +- %.6f (log Z0 = %.6f), ESS = %.1f of %d chains, entropy = %.6f" % (
        res["log_z"], res["log_z_se"], res["log_z0"], res["ess"], a.n, res["entropy"]))
    if records:
        logp = model_accel.log_probabilities(model, [seq for _, seq in records], res["log_z"])
        with open(a.o, "w") as f:
            f.write("id,H,logP\n")
            for (name, _), lp in zip(records, logp):
                f.write("%s,%.6f,%.6f\n" % (name, lp + res["log_z"], lp))
    return 0


if __name__ == "__main__":
    sys.exit(main())
