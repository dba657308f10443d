"""
Does a sample reproduce the statistics of the natural alignment?  One-, two- and three-site comparison of two
alignments, the check of the generative-Potts literature: a Boltzmann-machine fit matches f_i and f_ij by construction,
the connected three-site correlations C_ijk are the lowest order it never saw.

    python -m evcouplings_amd.correlations NATURAL.a2m SAMPLE.a2m [--theta 0.8] [--top 1000] [-o OUT.csv]

f_i and f_ij come from `plm.marginals`, the triplets from `plm.triplet_scan` (every triplet of the natural set, ranked)
and `plm.triplet_stats` (the chosen ones, on both sets); all of them run in libplm_hip on the GPU.  What happens here is
selection and a few correlation coefficients over the results.
"""
import numpy as np

from evcouplings_amd import alignment_io

RANKS = ("norm2", "maxabs")


def pearson_and_slope(x, y):
    """Pearson r and the least-squares slope of y against x (with intercept); nan where x or y is constant."""
    x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    dx, dy = x - x.mean(), y - y.mean()
    sxx, syy, sxy = float(dx @ dx), float(dy @ dy), float(dx @ dy)
    r = sxy / np.sqrt(sxx * syy) if sxx > 0 and syy > 0 else float("nan")
    return r, (sxy / sxx if sxx > 0 else float("nan"))


def connected_pairs(fi, fij):
    """C_ij(a,b) = f_ij(a,b) - f_i(a) f_j(b) for the i < j blocks of `plm.marginals`, in float64."""
    fi, fij = np.asarray(fi, np.float64), np.asarray(fij, np.float64)
    i, j = np.triu_indices(fi.shape[0], 1)
    return fij - fi[i][:, :, None] * fi[j][:, None, :]


def _keep(q, skip_state, order):
    m = np.ones((q,) * order, bool)
    if skip_state is not None and skip_state >= 0:
        for ax in range(order):
            m[(slice(None),) * ax + (skip_state,)] = False
    return m


def compare_statistics(natural, sample, q, weights=None, n_top=1000, rank_by="norm2", skip_state=None, device=0):
    """
    Compare `sample` (unit weights) with `natural` (weights, or None for unit weights), both (n, L) states 0..q-1.
    Returns a dict: "f_i", "c_ij", "c_ijk" -> (Pearson r, slope of sample against natural) over the cells that do not
    involve `skip_state`; "triplets" (n_top, 3) the triplets of the natural set with the largest `rank_by` ("norm2" or
    "maxabs") in descending order, "scores" their values, "norm2" / "maxabs" of each chosen triplet in both sets
    ("natural_norm2", "sample_norm2", ...), and "total" the fixed-point weight sums of the two triplet calls.
    """
    from evcouplings_amd import plm
    if rank_by not in RANKS:
        raise ValueError("rank_by must be one of %s (got %r)" % (RANKS, rank_by))
    natural, sample = plm._msa(natural), plm._msa(sample)
    if natural.shape[1] != sample.shape[1]:
        raise ValueError("natural has %d columns, sample has %d" % (natural.shape[1], sample.shape[1]))
    w_nat = np.ones(len(natural), np.float32) if weights is None else np.asarray(weights, np.float32)
    fi_n, fij_n = plm.marginals(natural, w_nat, q)
    fi_s, fij_s = plm.marginals(sample, np.ones(len(sample), np.float32), q)
    k1, k2, k3 = _keep(q, skip_state, 1), _keep(q, skip_state, 2), _keep(q, skip_state, 3)
    out = {"f_i": pearson_and_slope(fi_n[:, k1], fi_s[:, k1]),
           "c_ij": pearson_and_slope(connected_pairs(fi_n, fij_n)[:, k2], connected_pairs(fi_s, fij_s)[:, k2])}
    trip, norm2, maxabs, _ = plm.triplet_scan(natural, q, weights=weights, skip_state=skip_state, device=device)
    score = norm2 if rank_by == "norm2" else maxabs
    top = np.argsort(-score, kind="stable")[:max(1, int(n_top))]
    chosen = trip[top]
    nat = plm.triplet_stats(natural, q, chosen, weights=weights, skip_state=skip_state, device=device)
    sam = plm.triplet_stats(sample, q, chosen, skip_state=skip_state, device=device)
    cn, cs = nat["connected"][:, k3], sam["connected"][:, k3]
    out["c_ijk"] = pearson_and_slope(cn, cs)
    out.update(triplets=chosen, scores=score[top], total=(nat["total"], sam["total"]),
               natural_norm2=(cn ** 2).sum(axis=1), sample_norm2=(cs ** 2).sum(axis=1),
               natural_maxabs=np.abs(cn).max(axis=1), sample_maxabs=np.abs(cs).max(axis=1))
    return out


def write_table(path, result):
    """The per-triplet table of compare_statistics as CSV."""
    with open(path, "w") as f:
        f.write("i,j,k,score,natural_norm2,sample_norm2,natural_maxabs,sample_maxabs\n")
        for t, (i, j, k) in enumerate(result["triplets"]):
            f.write("%d,%d,%d,%.17g,%.17g,%.17g,%.17g,%.17g\n" % (
                i, j, k, result["scores"][t], result["natural_norm2"][t], result["sample_norm2"][t],
                result["natural_maxabs"][t], result["sample_maxabs"][t]))
    return path


def parse_args(argv=None):
    import argparse
    p = argparse.ArgumentParser(prog="python -m evcouplings_amd.correlations", description=__doc__.split("\n\n")[0])
    p.add_argument("natural", help="FASTA / A2M alignment of natural sequences (reweighted at --theta)")
    p.add_argument("sample", help="FASTA / A2M alignment of sampled sequences (unit weights), same columns")
    p.add_argument("--theta", type=float, default=0.8, help="identity threshold of the reweighting (0.8)")
    p.add_argument("--top", type=int, default=1000, help="triplets compared (1000)")
    p.add_argument("--rank-by", choices=RANKS, default="norm2")
    p.add_argument("--skip-gap", action="store_true", help="leave the gap state out of every comparison")
    p.add_argument("-o", "--output", help="per-triplet table (CSV)")
    args = p.parse_args(argv)
    if args.top < 1:
        p.error("--top must be at least 1")
    if not 0.0 < args.theta <= 1.0:
        p.error("--theta must lie in (0, 1]")
    return args


def main(argv=None):
    from evcouplings_amd import plm
    args = parse_args(argv)
    nat = alignment_io.encode_alignment(args.natural)
    sam = alignment_io.encode_alignment(args.sample)
    q = len(nat.alphabet)
    weights = (1.0 / plm.reweight(nat.msa, args.theta)).astype(np.float32)
    res = compare_statistics(nat.msa, sam.msa, q, weights=weights, n_top=args.top, rank_by=args.rank_by,
                             skip_state=0 if args.skip_gap else None)
    for key in ("f_i", "c_ij", "c_ijk"):
        print("%-6s r = %.6f  slope = %.6f" % (key, res[key][0], res[key][1]))
    if args.output:
        write_table(args.output, res)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
