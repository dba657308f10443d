"""
Refine a fitted Potts model on the GPU so that its samples reproduce the alignment's frequencies:

    python -m evcouplings_amd.bm_refine MODEL -o OUT.model [--epochs E] [--chains C] [--sweeps K] [--lr LR]
                                              [--decay-after T] [--seed SEED]

MODEL is a plmc_v2 `.model` file (what `plmc -o` / `bin/plmc_hip -o` write).  C persistent Gibbs chains make K sweeps per
epoch; after every epoch the fields and couplings move by LR times the difference between the file's f_i, f_ij and the
chains' frequencies, less the file's regularisers over N_eff (DESIGN_NEXT_ROWS.md section 9.7).  From epoch T on the step
decays as T / epoch (default: half the epochs).  OUT.model is MODEL with h_i and J_ij replaced; every other field is copied.
"""
import argparse
import sys

from evcouplings_amd import model_accel, model_io


def parser():
    ap = argparse.ArgumentParser(prog="python -m evcouplings_amd.bm_refine", description=__doc__.split("\n\n")[0])
    ap.add_argument("model")
    ap.add_argument("-o", required=True, help="output plmc_v2 model file")
    ap.add_argument("--epochs", type=int, default=120)
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--sweeps", type=int, default=2, help="sweeps per epoch")
    ap.add_argument("--lr", type=float, default=0.5)
    ap.add_argument("--decay-after", type=int, default=None, help="epoch after which the step decays (default: epochs / 2)")
    ap.add_argument("--seed", type=int, default=0)
    return ap


def write_refined(path, m, hi, jij):
    """The file of `m` (a `model_io.read_model_file` dict) with other fields and couplings."""
    return model_io.write_model_file(path, m["L"], m["q"], m["n_valid"], m["n_invalid"], m["num_iter"], m["theta"],
                                     m["lambda_h"], m["lambda_j"], m["lambda_group"], m["n_eff"], m["alphabet"],
                                     m["weights"], m["target_seq"], m["index_list"], m["fi"], hi, m["fij"], jij)


def _row(r):
    return "max|fi-pi| %.5f  max|fij-pij| %.5f  rms(fij-pij) %.6f  lr %.4f" % tuple(r)


def main(argv=None):
    a = parser().parse_args(argv)
    m = model_io.read_model_file(a.model)
    res = model_accel.refine_model(m, n_chains=a.chains, n_epochs=a.epochs, sweeps_per_epoch=a.sweeps, lr=a.lr,
                                   lr_decay_after=a.decay_after, seed=a.seed)
    write_refined(a.o, m, res["hi"], res["jij"])
    trace = res["trace"]
    print("epoch %4d: %s" % (0, _row(trace[0])))
    print("epoch %4d: %s" % (len(trace) - 1, _row(trace[-1])))
    print("%s after %d updates; wrote %s" % (res["status"], res["epochs_done"], a.o))
    return 0


if __name__ == "__main__":
    sys.exit(main())
