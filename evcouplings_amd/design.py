"""
Search a fitted Potts model for its highest-scoring sequences on the GPU:

    python -m evcouplings_amd.design MODEL -n N -o OUT.a2m [--steps K] [--beta-min B] [--beta-max B] [--sweeps n]
                                     [--greedy G] [--seed S] [--no-gaps] [--fix POS,...] [--start target|random]
                                     [--from A2M] [--top M] [--energies OUT.csv]

MODEL is a plmc_v2 `.model` file.  N chains are annealed over K inverse temperatures from --beta-min to --beta-max in
geometric progression (n Gibbs sweeps at each), then make at most G greedy sweeps, which move a position to its best
letter while that raises the statistical energy H.  The distinct best sequences of the chains are written to OUT.a2m,
highest H first, at most M of them, after the model's target sequence (named ID/start-end with the model's numbering).
--no-gaps never proposes the first letter of the alphabet (the gap); --fix keeps the target's residue at the listed
positions (the model's numbering); --start target starts every chain from the target sequence instead of a random
draw from the fields.
--from A2M runs no annealing: every sequence of that alignment (same columns as the model) climbs by greedy sweeps to
the local optimum it runs into (--steps must be 0 or absent, -n is not needed; --fix then keeps the sequence's own
residue), and all optima are written in the order of the input.
--energies writes one line per sequence written: id, H, H_J, H_h, chains (how many chains, or input sequences, ended
there) and mutations (positions that differ from the target).
"""
import argparse
import sys

import numpy as np

from evcouplings_amd import alignment_io, model_accel, sample

DEFAULT_STEPS = 100


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m evcouplings_amd.design", description=__doc__.split("\n\n")[0])
    ap.add_argument("model")
    ap.add_argument("-n", type=int, default=None, help="number of chains")
    ap.add_argument("-o", required=True, help="output A2M file")
    ap.add_argument("--steps", type=int, default=None, help="annealing steps (default %d)" % DEFAULT_STEPS)
    ap.add_argument("--beta-min", type=float, default=0.1)
    ap.add_argument("--beta-max", type=float, default=4.0)
    ap.add_argument("--sweeps", type=int, default=1, help="sweeps per annealing step")
    ap.add_argument("--greedy", type=int, default=100, help="greedy sweeps at most")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-gaps", action="store_true")
    ap.add_argument("--fix", default="", help="comma-separated positions that are not changed")
    ap.add_argument("--start", choices=("target", "random"), default="random")
    ap.add_argument("--from", dest="from_a2m", default=None, metavar="A2M", help="greedy ascent from these sequences")
    ap.add_argument("--top", type=int, default=None, metavar="M", help="write the M best sequences only")
    ap.add_argument("--energies", default=None, help="CSV file for the energies of the sequences written")
    ap.add_argument("--id", default="DESIGNED", help="identifier of the first record")
    a = ap.parse_args(argv)
    if a.from_a2m is not None:
        if a.steps not in (None, 0):
            ap.error("--from runs greedy sweeps only: --steps must be 0")
        if a.start != "random" or a.top is not None:
            ap.error("--from goes without --start and --top")
        a.steps = 0
    else:
        if a.n is None or a.n < 1:
            ap.error("-n N >= 1 chains are needed")
        a.steps = DEFAULT_STEPS if a.steps is None else a.steps
    if a.steps < 0 or a.sweeps < 1 or a.greedy < 0 or (a.steps == 0 and a.greedy == 0):
        ap.error("need --steps >= 0, --sweeps >= 1, --greedy >= 0, and not both --steps 0 and --greedy 0")
    if not (0.0 < a.beta_min <= a.beta_max < float("inf")):
        ap.error("need 0 < --beta-min <= --beta-max")
    if a.top is not None and a.top < 1:
        ap.error("--top M >= 1")
    try:
        a.fixed = [int(p) for p in a.fix.split(",") if p.strip()]
    except ValueError:
        ap.error("--fix takes comma-separated integer positions")
    return a


def main(argv=None):
    from evcouplings_amd import plm
    a = parse_args(argv)
    model = sample.model_from_file(a.model)
    exclude = model.alphabet[0] if a.no_gaps else ""
    target = np.array(list(model.target_seq)).astype("U1")
    if a.from_a2m is not None:
        _, seqs = alignment_io.read_fasta_records(a.from_a2m)
        rows = [s.decode("ascii") for s in seqs]
        if any(len(r) != model.L for r in rows):
            sys.exit("%s: every sequence must have the model's %d columns" % (a.from_a2m, model.L))
        out, en, _, _ = model_accel.local_optima(model, rows, fixed=a.fixed or None, exclude=exclude, max_sweeps=a.greedy)
        chains = np.ones(len(out), np.int64)
    else:
        betas = plm.annealing_schedule(a.steps, a.beta_min, a.beta_max)
        out, en, chains = model_accel.optimize_sequences(
            model, a.n, betas=betas, sweeps_per_step=a.sweeps, max_greedy=a.greedy, seed=a.seed,
            start="target" if a.start == "target" else None, fixed=a.fixed or None, exclude=exclude, top=a.top)
    sample.write_a2m(a.o, model, out, focus_id=a.id)
    if a.energies is not None:
        with open(a.energies, "w") as f:
            f.write("id,H,H_J,H_h,chains,mutations\n")
            for s, row in enumerate(en):
                f.write("sample%d,%.6f,%.6f,%.6f,%d,%d\n" % (s + 1, row[0], row[1], row[2], chains[s],
                                                             int((out[s] != target).sum())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
