"""
Do generated sequences cover the natural family?  Principal components of the natural alignment's one-hot features and
the projections of any set of sequences on them -- the figure of the bmDCA / arDCA papers, the one check that sees
subfamilies and modes a sampler did not cross (the site statistics of `correlations` cannot).

    python -m evcouplings_amd.pca NATURAL.a2m [SAMPLE.a2m ...] -k 2 [--theta 0.8] [--skip-gap] -o OUT.csv [--model OUT.npz]

The components come from `plm.pca_fit` (block subspace iteration, the covariance is never formed), the projections from
`plm.pca_project`; both run in libplm_hip on the GPU.  What happens here is bookkeeping, histograms and files.
"""
import numpy as np

from evcouplings_amd import alignment_io

MODEL_KEYS = ("mean", "components", "eigenvalues", "explained", "total_variance", "residuals", "iterations", "converged",
              "total", "q", "skip_state")


def fit_alignment(natural, q, weights=None, k=2, skip_state=None, device=0, **kw):
    """The model of the natural alignment: the dict of `plm.pca_fit` (with the scores of the natural rows) plus "q" and
    "skip_state" (-1 for none), which `project` needs.  kw: oversample, max_iter, tol, seed, callback."""
    from evcouplings_amd import plm
    model = plm.pca_fit(natural, q, k=k, weights=weights, skip_state=skip_state, scores=True, device=device, **kw)
    model["q"] = int(q)
    model["skip_state"] = -1 if skip_state is None else int(skip_state)
    return model


def project(model, seqs, device=0):
    """(n, k) projections of the sequences on the components of `model`."""
    from evcouplings_amd import plm
    skip = int(model["skip_state"])
    return plm.pca_project(seqs, int(model["q"]), model["mean"], model["components"],
                           skip_state=None if skip < 0 else skip, device=device)


def weighted_moments(t, weights=None):
    """Weighted mean and variance (about that mean) of every column of t (n, k), in float64."""
    t = np.asarray(t, np.float64)
    w = np.ones(len(t)) if weights is None else np.asarray(weights, np.float64)
    mean = (w[:, None] * t).sum(axis=0) / w.sum()
    var = (w[:, None] * (t - mean) ** 2).sum(axis=0) / w.sum()
    return mean, var


def histogram_overlap(t_nat, t_sam, weights=None, bins=40):
    """2-D histograms of the first two components of both sets on one grid that covers both, each normalised to 1, and
    their overlap sum(min(h_nat, h_sam)) in [0, 1].  Returns (h_nat, h_sam, overlap, edges_1, edges_2).  With a single
    component the second axis has one bin."""
    t_nat, t_sam = np.asarray(t_nat, np.float64), np.asarray(t_sam, np.float64)
    both = np.concatenate([t_nat[:, :2], t_sam[:, :2]])
    edges = []
    for c in range(both.shape[1]):
        lo, hi = float(both[:, c].min()), float(both[:, c].max())
        if not hi > lo:
            lo, hi = lo - 0.5, hi + 0.5
        edges.append(np.linspace(lo, hi, int(bins) + 1))
    if len(edges) == 1:
        edges.append(np.array([-0.5, 0.5]))

    def hist(t, w):
        y = t[:, 1] if t.shape[1] > 1 else np.zeros(len(t))
        h = np.histogram2d(t[:, 0], y, bins=edges, weights=w)[0]
        return h / h.sum()

    h_nat = hist(t_nat, None if weights is None else np.asarray(weights, np.float64))
    h_sam = hist(t_sam, None)
    return h_nat, h_sam, float(np.minimum(h_nat, h_sam).sum()), edges[0], edges[1]


def compare_projections(model, natural, weights, sample, bins=40, device=0):
    """
    Project `natural` (weights, or None for unit weights) and `sample` (unit weights) on the components of `model`.
    Returns a dict: "natural", "sample" the projections; "natural_mean", "natural_var", "sample_mean", "sample_var" per
    component; "hist_natural", "hist_sample" the normalised 2-D histograms of the first two components on a common grid
    ("edges_1", "edges_2"), and "overlap" = sum(min(hist_natural, hist_sample)).
    """
    t_nat, t_sam = project(model, natural, device=device), project(model, sample, device=device)
    out = {"natural": t_nat, "sample": t_sam}
    out["natural_mean"], out["natural_var"] = weighted_moments(t_nat, weights)
    out["sample_mean"], out["sample_var"] = weighted_moments(t_sam)
    (out["hist_natural"], out["hist_sample"], out["overlap"], out["edges_1"],
     out["edges_2"]) = histogram_overlap(t_nat, t_sam, weights, bins)
    return out


def save(path, model):
    """The model as .npz (the scores of the natural rows are not kept)."""
    np.savez(path, **{key: np.asarray(model[key]) for key in MODEL_KEYS})
    return path


def load(path):
    with np.load(path) as z:
        model = {key: z[key] for key in MODEL_KEYS}
    for key in ("total_variance",):
        model[key] = float(model[key])
    for key in ("iterations", "total", "q", "skip_state"):
        model[key] = int(model[key])
    model["converged"] = bool(model["converged"])
    return model


def write_table(path, sets):
    """One row per sequence: set, index, t_1 .. t_k.  sets: [(name, projections (n, k)), ...]."""
    k = sets[0][1].shape[1]
    with open(path, "w") as f:
        f.write("set,index," + ",".join("t_%d" % (c + 1) for c in range(k)) + "\n")
        for name, t in sets:
            for n, row in enumerate(t):
                f.write("%s,%d,%s\n" % (name, n, ",".join("%.17g" % x for x in row)))
    return path


def parse_args(argv=None):
    import argparse
    p = argparse.ArgumentParser(prog="python -m evcouplings_amd.pca", description=__doc__.split("\n\n")[0])
    p.add_argument("natural", help="FASTA / A2M alignment of natural sequences (reweighted at --theta)")
    p.add_argument("samples", nargs="*", help="further alignments with the same columns, projected on the components")
    p.add_argument("-k", "--components", type=int, default=2, help="principal components (2)")
    p.add_argument("--theta", type=float, default=0.8, help="identity threshold of the reweighting (0.8)")
    p.add_argument("--skip-gap", action="store_true", help="leave the features of the gap state out")
    p.add_argument("-o", "--output", required=True, help="table of projections (CSV): set, index, t_1..t_k")
    p.add_argument("--model", help="save mean, components and eigenvalues (.npz)")
    args = p.parse_args(argv)
    if not 1 <= args.components <= 64:
        p.error("-k must lie in 1..64")
    if not 0.0 < args.theta <= 1.0:
        p.error("--theta must lie in (0, 1]")
    return args


def main(argv=None):
    from evcouplings_amd import plm
    args = parse_args(argv)
    nat = alignment_io.encode_alignment(args.natural)
    q = len(nat.alphabet)
    weights = (1.0 / plm.reweight(nat.msa, args.theta)).astype(np.float32)
    model = fit_alignment(nat.msa, q, weights, k=args.components, skip_state=0 if args.skip_gap else None)
    for c in range(args.components):
        print("component %d: eigenvalue %.10g  explained %.6f  residual %.3g" % (
            c + 1, model["eigenvalues"][c], model["explained"][c], model["residuals"][c]))
    print("%s after %d iterations" % ("converged" if model["converged"] else "NOT converged", model["iterations"]))
    sets = [("natural", model["scores"])]
    for path in args.samples:
        sets.append((path, project(model, alignment_io.encode_alignment(path).msa)))
    write_table(args.output, sets)
    if args.model:
        save(args.model, model)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
