"""
Autoregressive Potts model of an alignment (arDCA, Trinquier et al. 2021; DESIGN_NEXT_ROWS.md section 9.19):

    P(x) = prod_k P(x_o(k) | x_o(0), ..., x_o(k-1)),   each conditional a softmax of a field plus couplings to the
                                                       earlier sites of the order o

    python -m evcouplings_amd.ar_model fit IN.a2m -o OUT.npz [--focus ID] [--order entropic|natural] [--theta T]
                                           [--lambda-h X] [--lambda-j X] [--max-iter K] [--epsilon E]
    python -m evcouplings_amd.ar_model sample MODEL.npz -n N -o OUT.a2m [--beta B] [--no-gaps] [--seed S]
    python -m evcouplings_amd.ar_model score MODEL.npz --sequences IN.a2m -o OUT.csv

The model is normalised by construction: `score` writes exact log-probabilities, `sample` independent exact samples (one
pass over the sites each).  The library only ever sees the sites in the order they are conditioned in; a site order is a
permutation of the columns applied here, on the way in, and inverted on the way out.

The file is an .npz with kind="ar".  It is NOT a plmc_v2 `.model`: block (j, i) couples a state of the earlier site with a
state of the later one and enters the later site's conditional only; these are not symmetric-gauge Potts couplings and
must not be read as such.

The defaults (entropic order, lambda_h = 1e-4, lambda_j = 1e-2 in per-sequence units, theta 0.8) are this project's
choice, not taken from a reference implementation.
"""
import argparse
import sys
from types import SimpleNamespace

import numpy as np

from evcouplings_amd import alignment_io, plm

FIELDS = ("hi", "jij", "order", "alphabet", "index_list", "target_seq", "lambda_h", "lambda_j", "n_eff", "theta")


def site_entropies(fi):
    """Shannon entropy (nats) of each row of the (L, q) frequencies, rows normalised first"""
    fi = np.asarray(fi, np.float64)
    p = fi / fi.sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(p > 0, p * np.log(p), 0.0)
    return -t.sum(axis=1)


def entropic_order(fi):
    """The sites by increasing entropy of their weighted frequencies, ties by index"""
    return np.argsort(site_entropies(fi), kind="stable").astype(np.int64)


def weighted_frequencies(msa, weights, q):
    msa = np.asarray(msa, np.int64)
    w = np.asarray(weights, np.float64)
    fi = np.zeros((msa.shape[1], q))
    for a in range(q):
        fi[:, a] = (w[:, None] * (msa == a)).sum(axis=0)
    return fi / w.sum()


def _resolve_order(order, msa, weights, q):
    L = msa.shape[1]
    if isinstance(order, str):
        if order == "natural":
            return np.arange(L, dtype=np.int64)
        if order == "entropic":
            return entropic_order(weighted_frequencies(msa, weights, q))
        raise ValueError("order must be 'entropic', 'natural' or a permutation of the sites")
    order = np.asarray(order, np.int64)
    if order.shape != (L,) or not np.array_equal(np.sort(order), np.arange(L)):
        raise ValueError("order must be a permutation of 0 .. %d" % (L - 1))
    return order


def fit_alignment(msa, q=21, theta_id=0.8, order="entropic", lambda_h=1e-4, lambda_j=1e-2, weights=None, max_iter=1000,
                  epsilon=1e-4, lbfgs_m=6, callback=None, alphabet=None, index_list=None, target_seq=None, device=0):
    """
    Fit the autoregressive model to an (N, L) matrix of states.  weights: None (1 / cluster size at identity theta_id,
    plm.reweight) or one weight per sequence.  Returns the model, a namespace with the FIELDS of the file plus `fit`, the
    dict of plm.ar_fit without the parameters.
    """
    msa = np.ascontiguousarray(msa, dtype=np.int8)
    if weights is None:
        weights = 1.0 / plm.reweight(msa, theta_id)
    weights = np.asarray(weights, np.float32)
    order = _resolve_order(order, msa, weights, q)
    res = plm.ar_fit(np.ascontiguousarray(msa[:, order]), weights, q, lambda_h, lambda_j, max_iter=max_iter,
                     epsilon=epsilon, lbfgs_m=lbfgs_m, callback=callback, device=device)
    L = msa.shape[1]
    alphabet = alignment_io.ALPHABET_PROTEIN[:q] if alphabet is None else alphabet
    return SimpleNamespace(
        hi=res.pop("hi"), jij=res.pop("jij"), order=order, alphabet=str(alphabet), L=L, q=int(q),
        index_list=np.arange(1, L + 1, dtype=np.int32) if index_list is None else np.asarray(index_list, np.int32),
        target_seq="".join(alphabet[k] for k in msa[0]) if target_seq is None else str(target_seq),
        lambda_h=float(lambda_h), lambda_j=float(lambda_j), n_eff=float(np.asarray(weights, np.float64).sum()),
        theta=float(theta_id), fit=res)


def log_probabilities(model, seqs, site_terms=False, device=0):
    """Exact log P of (n, L) states in the alignment's column order; with site_terms also [n, L] in that order"""
    seqs = np.ascontiguousarray(np.asarray(seqs, np.int8)[:, model.order])
    if not site_terms:
        return plm.ar_logprob(seqs, model.q, model.hi, model.jij, device=device)
    lp, site = plm.ar_logprob(seqs, model.q, model.hi, model.jij, site_terms=True, device=device)
    out = np.empty_like(site)
    out[:, model.order] = site
    return lp, out


def sample_sequences(model, n, seed=0, beta=1.0, exclude="", first_chain=0, device=0):
    """n independent samples, (n, L) states in the alignment's column order; exclude: letters never drawn"""
    allowed = None
    if exclude:
        allowed = np.array([ch not in exclude for ch in model.alphabet])
    x = plm.ar_sample(model.hi, model.jij, model.q, n, seed=seed, beta=beta, allowed=allowed, first_chain=first_chain,
                      device=device)
    out = np.empty_like(x)
    out[:, model.order] = x
    return out


def entropy_estimate(model, n, seed=0, device=0):
    """(-mean log P over n samples of the model, its standard error): the model's entropy in nats"""
    lp = log_probabilities(model, sample_sequences(model, n, seed=seed, device=device), device=device)
    return float(-lp.mean()), float(lp.std(ddof=1) / np.sqrt(n)) if n > 1 else float("nan")


def save(path, model):
    with open(path, "wb") as f:
        np.savez(f, kind="ar", **{k: getattr(model, k) for k in FIELDS})
    return path


def load(path):
    with np.load(path, allow_pickle=False) as z:
        if "kind" not in z.files or str(z["kind"]) != "ar":
            raise ValueError("%s is not an autoregressive model file (no kind=\"ar\")" % path)
        missing = [k for k in FIELDS if k not in z.files]
        if missing:
            raise ValueError("%s lacks %s" % (path, ", ".join(missing)))
        d = {k: z[k] for k in FIELDS}
    hi = np.asarray(d["hi"], np.float32)
    m = SimpleNamespace(hi=hi, jij=np.asarray(d["jij"], np.float32), order=np.asarray(d["order"], np.int64),
                        alphabet=str(d["alphabet"]), index_list=np.asarray(d["index_list"], np.int32),
                        target_seq=str(d["target_seq"]), L=hi.shape[0], q=hi.shape[1])
    for k in ("lambda_h", "lambda_j", "n_eff", "theta"):
        setattr(m, k, float(d[k]))
    return m


def _letters(model, states):
    table = np.array(list(model.alphabet))
    return ["".join(row) for row in table[np.asarray(states, np.int64)]]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m evcouplings_amd.ar_model", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    f = sub.add_parser("fit")
    f.add_argument("alignment")
    f.add_argument("-o", required=True)
    f.add_argument("--focus", default=None, help="focus sequence identifier (default: every column is a model column)")
    f.add_argument("--order", default="entropic", choices=["entropic", "natural"])
    f.add_argument("--theta", type=float, default=0.8)
    f.add_argument("--lambda-h", type=float, default=1e-4)
    f.add_argument("--lambda-j", type=float, default=1e-2)
    f.add_argument("--max-iter", type=int, default=1000)
    f.add_argument("--epsilon", type=float, default=1e-4)
    s = sub.add_parser("sample")
    s.add_argument("model")
    s.add_argument("-n", type=int, required=True)
    s.add_argument("-o", required=True)
    s.add_argument("--beta", type=float, default=1.0)
    s.add_argument("--no-gaps", action="store_true")
    s.add_argument("--seed", type=int, default=0)
    c = sub.add_parser("score")
    c.add_argument("model")
    c.add_argument("--sequences", required=True)
    c.add_argument("-o", required=True)
    a = ap.parse_args(argv)
    if a.cmd == "fit":
        enc = alignment_io.encode_alignment(a.alignment, focus_seq=a.focus)
        model = fit_alignment(enc.msa, q=len(enc.alphabet), theta_id=a.theta, order=a.order, lambda_h=a.lambda_h,
                              lambda_j=a.lambda_j, max_iter=a.max_iter, epsilon=a.epsilon, alphabet=enc.alphabet,
                              index_list=enc.index_list, target_seq=enc.target_seq)
        save(a.o, model)
        sys.stderr.write("%s after %d iterations: F = %.6f, |g| = %.3e, N_eff = %.1f\n"
                         % (model.fit["status"], model.fit["iterations"], model.fit["fx"], model.fit["gnorm"], model.n_eff))
        return 0
    model = load(a.model)
    if a.cmd == "sample":
        from evcouplings_amd.sample import write_a2m
        x = sample_sequences(model, a.n, seed=a.seed, beta=a.beta, exclude=model.alphabet[0] if a.no_gaps else "")
        write_a2m(a.o, model, _letters(model, x))
        return 0
    enc = alignment_io.encode_alignment(a.sequences, alphabet=model.alphabet)
    if enc.msa.shape[1] != model.L:
        ap.error("%s has %d columns, the model %d sites" % (a.sequences, enc.msa.shape[1], model.L))
    lp = log_probabilities(model, enc.msa)
    ids = [h for h, ok in zip(enc.ids, enc.valid) if ok]
    with open(a.o, "w") as out:
        out.write("id,log_p\n")
        for h, v in zip(ids, lp):
            out.write("%s,%.17g\n" % (h.split()[0], v))
    return 0


if __name__ == "__main__":
    sys.exit(main())
