"""
Sample sequences from a fitted Potts model on the GPU:

    python -m evcouplings_amd.sample MODEL -n N -o OUT.a2m [--beta B] [--burn-in S] [--thin T] [--snapshots K]
                                     [--seed SEED] [--no-gaps] [--fix POS,POS,...] [--energies OUT.csv]
                                     [--tempering R [--beta-max B]]

MODEL is a plmc_v2 `.model` file (what `plmc -o` / `bin/plmc_hip -o` write).  N independent Gibbs chains run S burn-in
sweeps; K snapshots of all chains, T sweeps apart, are written (N x K sequences).  The first record of OUT.a2m is the
model's target sequence, named ID/start-end with the model's numbering, the samples follow.  --no-gaps never draws the
first letter of the alphabet (the gap); --fix keeps the target's residue at the listed positions (the model's numbering).
--energies writes one line per sample: id, H, H_J, H_h at beta = 1.
--tempering R samples by parallel tempering instead: N independent ladders of R walkers at inverse temperatures on the
couplings from 0 to B (--beta-max, default 1) that exchange after every sweep; S and T then count rounds, and the
sequences written are those of the walker at B.  The acceptance rate of every pair of neighbouring temperatures goes to
standard error.  It takes all letters at all positions: not with --no-gaps, --fix or --beta.
"""
import argparse
import sys
from types import SimpleNamespace

import numpy as np

from evcouplings_amd import model_accel, model_io


def model_from_file(path):
    """The attributes `model_accel.sample_sequences` reads, from a plmc_v2 file (i<j blocks -> dense J_ij)."""
    m = model_io.read_model_file(path)
    L, q = m["L"], m["q"]
    J = np.zeros((L, L, q, q), np.float32)
    if L > 1:
        iu, ju = np.triu_indices(L, 1)
        J[iu, ju] = m["jij"]
        J[ju, iu] = m["jij"].transpose(0, 2, 1)
    return SimpleNamespace(J_ij=J, h_i=m["hi"], alphabet=m["alphabet"], target_seq=m["target_seq"],
                           index_list=m["index_list"], L=L, q=q)


def write_a2m(path, model, samples, focus_id="SAMPLED"):
    """First record: the target as focus_id/start-end (the layout of synthetic.msa_to_a2m); then sample1/1-L ..."""
    L = model.L
    idx = np.asarray(model.index_list)
    with open(path, "w") as f:
        f.write(">%s/%d-%d\n%s\n" % (focus_id, int(idx[0]), int(idx[-1]), "".join(model.target_seq)))
        for s, row in enumerate(samples):
            f.write(">sample%d/1-%d\n%s\n" % (s + 1, L, "".join(row)))
    return path


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m evcouplings_amd.sample", description=__doc__.split("\n\n")[0])
    ap.add_argument("model")
    ap.add_argument("-n", type=int, required=True, help="number of chains")
    ap.add_argument("-o", required=True, help="output A2M file")
    ap.add_argument("--beta", type=float, default=1.0)
    ap.add_argument("--burn-in", type=int, default=100)
    ap.add_argument("--thin", type=int, default=1)
    ap.add_argument("--snapshots", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-gaps", action="store_true")
    ap.add_argument("--fix", default="", help="comma-separated positions that keep the target's residue")
    ap.add_argument("--energies", default=None, help="CSV file for the energies of the samples")
    ap.add_argument("--id", default="SAMPLED", help="identifier of the first record")
    ap.add_argument("--tempering", type=int, default=0, metavar="R",
                    help="parallel tempering over R inverse temperatures on the couplings")
    ap.add_argument("--beta-max", type=float, default=None, metavar="B", help="the top of the ladder (default 1)")
    a = ap.parse_args(argv)
    if a.beta_max is not None and not a.tempering:
        ap.error("--beta-max goes with --tempering")
    if a.tempering and (a.tempering < 1 or a.no_gaps or a.fix.strip() or a.beta != 1.0):
        ap.error("--tempering takes R >= 1 and goes without --no-gaps, --fix and --beta")
    model = model_from_file(a.model)
    fixed = [int(p) for p in a.fix.split(",") if p.strip()]
    if a.tempering:
        res = model_accel.sample_tempered(model, a.n, n_rungs=a.tempering,
                                          beta_max=1.0 if a.beta_max is None else a.beta_max, burn_in=a.burn_in,
                                          n_snapshots=a.snapshots, thin=a.thin, seed=a.seed,
                                          energies=a.energies is not None, info=True)
        sys.stderr.write("acceptance between neighbouring temperatures: %s\n"
                         % " ".join("%.3f" % v for v in res[-1]["acceptance"]))
        res = res[:-1] if a.energies is not None else res[0]
    else:
        res = model_accel.sample_sequences(model, a.n, burn_in=a.burn_in, n_snapshots=a.snapshots, thin=a.thin,
                                           beta=a.beta, seed=a.seed, fixed=fixed or None,
                                           exclude=model.alphabet[0] if a.no_gaps else "",
                                           energies=a.energies is not None)
    samples, en = res if a.energies is not None else (res, None)
    write_a2m(a.o, model, samples, focus_id=a.id)
    if en is not None:
        with open(a.energies, "w") as f:
            f.write("id,H,H_J,H_h\n")
            for s, row in enumerate(en):
                f.write("sample%d,%.6f,%.6f,%.6f\n" % (s + 1, row[0], row[1], row[2]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
